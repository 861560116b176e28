"""The numeric contract of mi_icp_create_from_depth (include/mi_icp.h) restated in numpy fp32: the pose of an extrinsic,
the U16 depth rule, the point, colour and normal of every pixel and the compaction, word for word; the scenes and the
case lists that test_depth_exact_cpu.py (against the C oracle and hand-worked images) and test_gpu_depth.py (against
the kernel) share.  A helper, not a test."""
import numpy as np

F = np.float32


def invert4(E):
    """the pose of an extrinsic as the library computes it: Gauss-Jordan with partial pivoting in double, rounded to
    float at the end (row-major in, row-major out)"""
    a = [[float(E[r][k]) for k in range(4)] + [1.0 if r == k else 0.0 for k in range(4)] for r in range(4)]
    for col in range(4):
        piv = col
        for r in range(col + 1, 4):
            if abs(a[r][col]) > abs(a[piv][col]):
                piv = r
        assert abs(a[piv][col]) > 0.0, "singular extrinsic"
        a[piv], a[col] = a[col], a[piv]
        d = a[col][col]
        a[col] = [v / d for v in a[col]]
        for r in range(4):
            if r != col and a[r][col] != 0.0:
                f = a[r][col]
                a[r] = [a[r][k] - f * a[col][k] for k in range(8)]
    return np.array([[a[r][4 + k] for k in range(4)] for r in range(4)], np.float64).astype(F)


def pose_of(extrinsic):
    E = np.eye(4, dtype=F) if extrinsic is None else np.asarray(extrinsic, F).reshape(4, 4)
    return invert4(E)


def u16_to_float(depth, depth_scale, depth_trunc):
    """Image::ConvertDepthToFloatImage as the entry applies it: both parameters held as int, the division a product with
    the correctly rounded reciprocal (the reference's vector TEST(Image, ConvertDepthToFloatImage) pins it at 1000)"""
    with np.errstate(all="ignore"):
        f = np.asarray(depth, np.uint16).astype(F) * F(np.float64(1.0) / np.float64(F(int(depth_scale))))
    return np.where(f >= F(int(depth_trunc)), F(0), f).astype(F)


def structured(depth, intrinsic4, extrinsic, *, color=None, stride=1, rgbd=False, depth_cutoff=-1.0,
               compute_normals=False):
    """one entry per sampled pixel, in pixel order: dict(pix, accepted, points, normals | None, colors | None,
    flipped | None, zeroed | None).  flipped: the normal was multiplied by -1; zeroed: the pixel has a neighbour that
    counted as (0, 0, 0) because its point is not finite (not: because it lies past the image)."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (F(v) for v in intrinsic4)
    pose = pose_of(extrinsic)
    sw, sh = w // stride, h // stride
    row, col = np.meshgrid(np.arange(sh) * stride, np.arange(sw) * stride, indexing="ij")
    row, col = row.reshape(-1), col.reshape(-1)
    pix = row * w + col
    d = depth.reshape(-1)[pix]
    cut = F(depth_cutoff)
    with np.errstate(all="ignore"):
        ok = ((d > F(0)) & ((cut <= F(0)) | (cut > d))) if rgbd else ~(d <= F(0))
        x = (col.astype(F) - cx) * d / fx
        y = (row.astype(F) - cy) * d / fy
        P = np.stack([((pose[r, 0] * x + pose[r, 1] * y) + pose[r, 2] * d) + pose[r, 3] for r in range(3)], 1).astype(F)
    P[~ok] = F(np.inf)
    out = dict(pix=pix, accepted=ok, points=P, normals=None, colors=None, flipped=None, zeroed=None)
    if color is not None:
        color = np.asarray(color)
        if color.dtype == np.uint8:
            Cc = color.reshape(-1, 3)[pix].astype(F) / F(255.0)
        else:
            v = color.astype(F).reshape(-1)[pix] / F(1.0)
            Cc = np.stack([v, v, v], 1)
        Cc = Cc.astype(F)
        Cc[~ok] = F(np.inf)
        out["colors"] = Cc
    if compute_normals:
        assert stride == 1
        total = w * h
        fin = np.isfinite(P).all(1)
        Z = np.concatenate([np.where(fin[:, None], P, F(0)), np.zeros((w + 1, 3), F)])     # past the image: zero
        finz = np.concatenate([fin, np.ones(w + 1, bool)])
        inner = (row >= 1) & (col >= 1)
        idx = np.where(inner, pix, 0)                       # (elsewhere any index will do: the result is not used)
        l, r, u, lo = Z[idx - 1], Z[idx + 1], Z[idx - w], Z[idx + w]
        with np.errstate(all="ignore"):
            hh, vv = l - r, u - lo
            c = np.stack([hh[:, 1] * vv[:, 2] - hh[:, 2] * vv[:, 1],
                          hh[:, 2] * vv[:, 0] - hh[:, 0] * vv[:, 2],
                          hh[:, 0] * vv[:, 1] - hh[:, 1] * vv[:, 0]], 1).astype(F)
            norm = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
            n = np.where((norm == F(0))[:, None], F(0), c / norm[:, None]).astype(F)
            flip = n[:, 2] > F(0)
            n = np.where(flip[:, None], n * F(-1.0), n).astype(F)
        n[~inner] = F(0)
        assert total == len(pix)
        out["normals"] = n
        out["flipped"] = flip & inner
        out["zeroed"] = inner & ~(finz[idx - 1] & finz[idx + 1] & finz[idx - w] & finz[idx + w])
    return out


def cloud(depth, intrinsic4, extrinsic, *, color=None, stride=1, rgbd=False, depth_cutoff=-1.0, compute_normals=False,
          valid_only=True):
    """-> (points, normals | None, colors | None, pixel_index): what mi_icp_create_from_depth writes for a float depth
    image, and row * width + col of every point written"""
    s = structured(depth, intrinsic4, extrinsic, color=color, stride=stride, rgbd=rgbd, depth_cutoff=depth_cutoff,
                   compute_normals=compute_normals)
    keep = np.isfinite(s["points"]).all(1) if valid_only else np.ones(len(s["pix"]), bool)
    pick = lambda a: None if a is None else np.ascontiguousarray(a[keep])
    return pick(s["points"]), pick(s["normals"]), pick(s["colors"]), s["pix"][keep]


def depth_points(depth, width, height, fx, fy, cx, cy, extrinsic, stride):
    """the world points of the sampled pixels (PointCloud::CreateFromDepthImage, depth_scale 1000, depth_trunc 1000,
    project_valid_depth_only), in pixel order"""
    return cloud(np.asarray(depth, F).reshape(height, width), [fx, fy, cx, cy], extrinsic, stride=stride)[0]


def _words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_words(a, b):
    """equal shapes, NaN in the same places, every other word equal (+-inf and -0 included)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (_words(a)[~na] == _words(b)[~na]).all())


def difference(what, got, want, pixel_index, width):
    """None when same_words(got, want); else a message that names the first differing pixel and shows both values"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return "%s: %d rows, the restatement has %d" % (what, len(got), len(want))
    if same_words(got, want):
        return None
    na, nb = np.isnan(got), np.isnan(want)
    bad = ((na != nb) | (~na & ~nb & (_words(got) != _words(want)))).reshape(len(got), -1).any(1)
    k = int(np.flatnonzero(bad)[0])
    p = int(pixel_index[k])
    return "%s differs at %d of %d entries, first at entry %d = pixel %d (row %d, col %d of width %d): got %r (%s), want %r (%s)" % (
        what, int(bad.sum()), len(got), k, p, p // width, p % width, width, got[k].tolist(),
        " ".join("%08x" % v for v in _words(got[k])), want[k].tolist(), " ".join("%08x" % v for v in _words(want[k])))


# ---- scenes ----------------------------------------------------------------------------------------------------------
DEFECTS = (0.0, -1.0, np.nan, np.inf)
CUTOFF = 1.8                    # cuts the far band and the far corner of scene()


def scene(w, h, seed):
    """a float depth: a slanted plane, a curved part on the left, a band 0.9 farther in the middle (two step edges),
    and npix // 40 pixels of each defect kind (0, -1, NaN, +inf) at seeded places.  Below 40 pixels: no defects, no
    band and a gentler slope that stays inside CUTOFF, so that the few pixels there are all points."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    small = w * h < 40
    d = 1.2 + (0.2 * u + 0.15 * v if small else 0.5 * u + 0.3 * v)
    d = d + np.where(u < 0.45, 0.25 * np.sin(3.0 * u + 1.0) * np.cos(2.5 * v), 0.0)
    d = d + np.where((u > 0.45) & (u < 0.7) & (not small), 0.9, 0.0)
    d = (d + 0.002 * rng.standard_normal((h, w))).astype(F)
    k = (w * h) // 40
    at = rng.permutation(w * h)[:4 * k]
    for i, bad in enumerate(DEFECTS):
        d.reshape(-1)[at[i * k:(i + 1) * k]] = F(bad)
    return d


def colors_of(kind, w, h, seed):
    rng = np.random.default_rng(seed + 100)
    if kind == "u8":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "f32":
        return rng.random((h, w), dtype=F)
    return None


def intrinsic_of(w, h, integral=False):
    """fx != fy, the principal point off the pixel grid unless `integral`"""
    if integral:
        return [F(0.83 * w + 1.7), F(0.79 * w + 2.3), F(w // 2), F(h // 2)]
    return [F(0.83 * w + 1.7), F(0.79 * w + 2.3), F((w - 1) / 2 + 0.3), F((h - 1) / 2 - 0.2)]


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def extrinsic_of(kind):
    """None; the identity; a rigid motion turned far enough that normals come out on both sides of the flip; a general
    matrix (shear, unequal scales, a last row that is not 0 0 0 1)"""
    if kind is None:
        return None
    E = np.eye(4)
    if kind == "rigid":
        E[:3, :3] = _rot(0, 1.45) @ _rot(1, -0.4) @ _rot(2, 0.3)
        E[:3, 3] = (0.3, -0.2, 0.5)
    elif kind == "general":
        E[:3, :3] = (_rot(1, 0.7) @ _rot(0, -0.5)) @ np.array([[1.3, 0.2, 0.0], [0.0, 0.8, -0.3], [0.1, 0.0, 1.1]])
        E[:3, 3] = (-0.4, 0.1, 0.25)
        E[3] = (0.01, -0.02, 0.03, 1.1)
    else:
        assert kind == "identity"
    return E.astype(F)


def convention_images():
    """[(name, depth, intrinsic4, cutoff)]: images built for the neighbour rules -- the right neighbour of the last
    column is the next row's first pixel, the lower neighbour of the last row is zero, a rejected neighbour is zero"""
    a = np.full((6, 8), 2.0, F)
    a[2, 3] = 0.0
    b = (1.0 + 0.125 * np.arange(20, dtype=F).reshape(4, 5) % 0.75).astype(F)
    b[1, 4] = np.nan                                       # a last-column pixel that is itself no point
    b[2, 0] = 3.0                                          # beyond the cutoff: the wrap neighbour of (1, 4) and of no one else
    b[3, 2] = np.inf                                       # accepted, its point is not finite
    return [("hole", a, [4.0, 4.0, 3.5, 2.5], -1.0), ("edges", b, [3.0, 2.5, 2.0, 1.5], 2.5)]


def hand_images():
    """[(name, depth)] for fx = fy = 1, cx = cy = 0, no extrinsic, no cutoff: the point of pixel (row, col) with depth d
    is (col * d, row * d, d), so every step of the normal rule is integer arithmetic one can do by hand
    (test_depth_exact_cpu.py writes the results out)"""
    wrap = np.ones((3, 3), F)
    wrap[2, 0] = 2.0
    last = np.ones((3, 4), F)
    last[1, 1] = 2.0
    hole = np.ones((3, 3), F)
    hole[1, 0] = 0.0
    return [("wrap", wrap), ("last", last), ("hole", hole)]


HAND_K = [1.0, 1.0, 0.0, 0.0]


# ---- the cases (both test files run exactly these) -------------------------------------------------------------------
def _case(**kw):
    base = dict(extrinsic=None, integral=False, stride=1, color=None, cutoff=-1.0, normals=False, valid_only=True)
    base.update(kw)
    return base


def depth_cases():
    """rgbd = 0.  70 / 3 = 23 columns and 50 / 3 = 16 rows: the sampled grid is not the image."""
    out = []
    for (w, h) in ((1, 1), (7, 1), (1, 7), (37, 23), (257, 3)):
        out.append(_case(w=w, h=h, extrinsic="rigid"))
    for stride in (1, 2, 3, 7, 71):                        # 71 > 70: an empty cloud
        for ext in ((None, "general") if stride in (1, 3) else ("rigid",)):
            out.append(_case(w=70, h=50, stride=stride, extrinsic=ext))
    out.append(_case(w=70, h=50, stride=2, extrinsic="identity"))
    out.append(_case(w=37, h=23, stride=3, extrinsic="identity", integral=True))
    out.append(_case(w=70, h=50, extrinsic="rigid", integral=True))
    out.append(_case(w=640, h=480, extrinsic="rigid"))
    return out


def rgbd_cases():
    """rgbd = 1.  37x23: the full cross.  The other sizes: KinFu's setting (colour, cutoff, normals, valid only) and its
    valid_only = 0 twin.  2x3 beside 2x2: the smallest image in which a last-column pixel has a right neighbour at all
    (in 2x2 the only last-column pixel below row 0 is the last pixel)."""
    out = []
    for color in (None, "u8", "f32"):
        for cutoff in (-1.0, CUTOFF):
            for valid_only in (True, False):
                for normals in (False, True):
                    out.append(_case(w=37, h=23, extrinsic="rigid", color=color, cutoff=cutoff, normals=normals,
                                     valid_only=valid_only))
    sizes = (((2, 2), "identity", "u8"), ((2, 3), "identity", "u8"), ((8, 6), "rigid", "f32"), ((70, 50), "general", "u8"),
             ((35, 25), None, "f32"), ((17, 12), "rigid", "u8"), ((640, 480), "rigid", "u8"))
    for (w, h), ext, color in sizes:
        for valid_only in ((True,) if w == 640 else (True, False)):
            out.append(_case(w=w, h=h, extrinsic=ext, color=color, cutoff=CUTOFF, normals=True, valid_only=valid_only))
    out.append(_case(w=70, h=50, extrinsic="rigid", integral=True, color="u8", normals=True, valid_only=False))
    return out


def case_id(c):
    return "%dx%d-s%d-%s%s-%s-cut%s-n%d-v%d" % (c["w"], c["h"], c["stride"], c["extrinsic"], "-intcx" if c["integral"] else "",
                                              c["color"], c["cutoff"], int(c["normals"]), int(c["valid_only"]))


def case_inputs(c, rgbd):
    """-> (depth, intrinsic4, extrinsic, keyword arguments of cloud() / Engine.create_from_depth without `color`, color)"""
    w, h = c["w"], c["h"]
    seed = 7 * w + h
    d = scene(w, h, seed)
    K = intrinsic_of(w, h, c["integral"])
    if c["integral"]:
        d[h // 3, w // 2] = np.inf                          # col == cx under an infinite depth: 0 * inf
    kw = dict(stride=c["stride"])
    if rgbd:
        kw.update(rgbd=True, depth_cutoff=c["cutoff"], compute_normals=c["normals"], valid_only=c["valid_only"])
    return d, K, extrinsic_of(c["extrinsic"]), kw, colors_of(c["color"], w, h, seed)


U16_K = [F(59.8), F(57.6), F(34.8), F(24.3)]
U16_PARAMS = ((1000.0, 1000.0), (1000.0, 3.0), (999.7, 2.9), (500.0, 4.5))


def u16_image():
    """70x50, millimetres of scene() with values at and beside every threshold of U16_PARAMS, 0 and 65535"""
    d = scene(70, 50, 77)
    with np.errstate(all="ignore"):
        m = np.where(np.isfinite(d) & (d > 0), d * 1000.0, 0.0)
    u = np.clip(m, 0, 65535).astype(np.uint16)
    u[3, 5:17] = (1998, 1999, 2000, 2001, 2249, 2250, 2251, 2997, 2998, 2999, 3000, 65535)
    u[40, 60:64] = (65535, 1, 0, 65534)
    return u
