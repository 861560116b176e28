"""The VoxelGrid contract of include/mi_icp.h restated in numpy, fp32 in the order written there: from_points, dense,
merge (both modes), carve, query, bounds.  The yardstick of test_voxelgrid_cpu.py (which holds it to the reference's
unit tests and to brute-force definitions) and of the GPU tests (which hold the library to it, bit for bit).
Also the scenes those tests share."""
import numpy as np

F = np.float32
AVERAGE, KEEP_FIRST = 0, 1
INT_MAX = 2147483647


def floor_index(v):
    """floor(.) as int32, held inside +-1e9 first"""
    with np.errstate(all="ignore"):
        return np.clip(np.floor(v), F(-1.0e9), F(1.0e9)).astype(np.int32)


def point_keys(xyz, voxel_size, origin):
    """-> (keys [n, 3] int32, finite [n] bool): floor((p - origin) / voxel_size) per axis in fp32"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    fin = np.isfinite(xyz).all(axis=1)
    with np.errstate(all="ignore"):
        q = (xyz - np.asarray(origin, F).reshape(1, 3)) / F(voxel_size)
    return floor_index(q), fin


def _runs(keys):
    """stable lexicographic order (x most significant) -> (order, starts [r + 1])"""
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))   # (lexsort is stable)
    sk = keys[order]
    head = np.ones(len(sk), bool)
    head[1:] = (sk[1:] != sk[:-1]).any(axis=1)
    starts = np.concatenate([np.flatnonzero(head), [len(sk)]])
    return order, starts


def _run_sums(values, order, starts, dtype):
    """per run the sum of values[order[...]] left to right in `dtype` (no pairwise tricks)"""
    lens = np.diff(starts)
    acc = np.zeros((len(lens), values.shape[1]), dtype)
    v = values[order].astype(dtype)
    first = True
    for j in range(int(lens.max()) if len(lens) else 0):
        live = np.flatnonzero(lens > j)
        if first:
            acc[live] = v[starts[live]]
            first = False
        else:
            acc[live] = acc[live] + v[starts[live] + j]
    return acc, lens


def refused_from_points(voxel_size, min_bound, max_bound):
    vs = F(voxel_size)
    lo, hi = np.asarray(min_bound, F).reshape(3), np.asarray(max_bound, F).reshape(3)
    if not (vs > 0) or not np.isfinite(vs) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        return True
    return bool(F(vs * F(INT_MAX)) < (hi - lo).max())


def from_points(xyz, colors, voxel_size, min_bound, max_bound):
    """-> (keys [m, 3] int32 ascending, colors [m, 3] fp32): the fp64 mean in input order, rounded once"""
    assert not refused_from_points(voxel_size, min_bound, max_bound)
    keys, fin = point_keys(xyz, voxel_size, min_bound)
    keep = np.flatnonzero(fin)
    keys = keys[keep]
    if len(keys) == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    order, starts = _runs(keys)
    out_keys = keys[order[starts[:-1]]]
    if colors is None:
        return out_keys, np.ones((len(out_keys), 3), F)
    col = np.asarray(colors, F).reshape(-1, 3)[keep]
    s, lens = _run_sums(col, order, starts, np.float64)
    return out_keys, (s / lens[:, None].astype(np.float64)).astype(F)


def key_span_bits(keys):
    """the bits the packed key of these keys needs (x: one slot more)"""
    ext = keys.astype(np.int64).max(axis=0) - keys.astype(np.int64).min(axis=0) + 1
    return int(ext[0]).bit_length() + int(ext[1] - 1).bit_length() + int(ext[2] - 1).bit_length()


def dense(num_w, num_h, num_d):
    if num_w <= 0 or num_h <= 0 or num_d <= 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    assert num_w * num_h * num_d <= INT_MAX
    idx = np.arange(num_w * num_h * num_d, dtype=np.int64)
    hd = num_h * num_d
    keys = np.stack([idx // hd, (idx % hd) // num_d, idx % num_d], axis=1).astype(np.int32)
    return keys, np.ones((len(keys), 3), F)


def merge(keys_a, colors_a, keys_b, colors_b, mode):
    keys = np.concatenate([np.asarray(keys_a, np.int32).reshape(-1, 3), np.asarray(keys_b, np.int32).reshape(-1, 3)])
    cols = np.concatenate([np.asarray(colors_a, F).reshape(-1, 3), np.asarray(colors_b, F).reshape(-1, 3)])
    if len(keys) == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    order, starts = _runs(keys)
    out_keys = keys[order[starts[:-1]]]
    if mode == KEEP_FIRST:
        return out_keys, cols[order[starts[:-1]]]
    s, lens = _run_sums(cols, order, starts, F)
    return out_keys, (s / lens[:, None].astype(F)).astype(F)


CORNER_SIGNS = [(-1, -1, -1), (-1, -1, 1), (1, -1, -1), (1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, 1, -1), (1, 1, 1)]


def k3(intrinsic4):
    fx, fy, cx, cy = [F(v) for v in intrinsic4]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


def carve_stay(keys, voxel_size, origin, image, intrinsic4, extrinsic, keep_outside):
    """-> stay [m] bool.  image: [H, W] or [H, W, C] of any dtype; extrinsic: 4x4 row-major"""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    vs = F(voxel_size)
    o = np.asarray(origin, F).reshape(3)
    img = np.asarray(image)
    H, W = img.shape[0], img.shape[1]
    float_image = img.ndim == 2 and img.dtype == np.float32
    K, E = k3(intrinsic4), np.asarray(extrinsic, F).reshape(4, 4)
    R, t = E[:3, :3], E[:3, 3]
    r = F(vs / F(2.0))
    c = (keys.astype(F) + F(0.5)) * vs + o
    stay = np.zeros(len(keys), bool)
    with np.errstate(all="ignore"):
        for sg in CORNER_SIGNS:
            p = [c[:, d] + (r if sg[d] > 0 else -r) for d in range(3)]
            X = [((R[d, 0] * p[0] + R[d, 1] * p[1]) + R[d, 2] * p[2]) + t[d] for d in range(3)]
            uvz = [(K[d, 0] * X[0] + K[d, 1] * X[1]) + K[d, 2] * X[2] for d in range(3)]
            z = uvz[2]
            u, v = uvz[0] / z, uvz[1] / z
            within = (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))
            if not float_image:
                within[:] = False
            ok = np.zeros(len(keys), bool)
            if float_image and within.any():
                uu, vv = np.where(within, u, F(0)), np.where(within, v, F(0))
                ui = np.clip(uu.astype(np.int32), 0, W - 2)
                vi = np.clip(vv.astype(np.int32), 0, H - 2)
                pu, pv = uu - ui.astype(F), vv - vi.astype(F)
                one = F(1)
                v00, v01, v10, v11 = img[vi, ui], img[vi + 1, ui], img[vi, ui + 1], img[vi + 1, ui + 1]
                d = (v00 * (one - pv) + v01 * pv) * (one - pu) + (v10 * (one - pv) + v11 * pv) * pu
                ok = within & (d > 0) & (z >= d)
            stay |= np.where(within, ok, bool(keep_outside))
    return stay


def carve(keys, colors, voxel_size, origin, image, intrinsic4, extrinsic, keep_outside):
    stay = carve_stay(keys, voxel_size, origin, image, intrinsic4, extrinsic, keep_outside)
    return np.asarray(keys, np.int32).reshape(-1, 3)[stay], np.asarray(colors, F).reshape(-1, 3)[stay]


def query(keys, voxel_size, origin, queries):
    """-> (included [nq] bool, index [nq, 3] int32; a non-finite query: not included, index 0)"""
    idx, fin = point_keys(queries, voxel_size, origin)
    idx[~fin] = 0
    have = set(map(tuple, np.asarray(keys, np.int32).reshape(-1, 3).tolist()))
    inc = np.array([bool(f) and (tuple(k) in have) for k, f in zip(idx.tolist(), fin)], bool)
    return inc.reshape(-1), idx


def bounds(keys, voxel_size, origin):
    """-> (min_bound, max_bound fp32; centre as the fp64 mean of the fp32 voxel centres, rounded once)"""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    vs, o = F(voxel_size), np.asarray(origin, F).reshape(3)
    if len(keys) == 0:
        return o.copy(), o.copy(), np.zeros(3, F)
    lo, hi = keys.min(axis=0), keys.max(axis=0)
    centres = (keys.astype(F) * vs + o) + F(0.5) * vs
    s = np.zeros(3, np.float64)
    for chunk in np.array_split(centres.astype(np.float64), max(1, len(centres) // 4096)):
        s = s + chunk.sum(axis=0)
    return lo.astype(F) * vs + o, (hi.astype(F) + F(1)) * vs + o, (s / float(len(keys))).astype(F)


def ulp_distance(a, b):
    """fp32 values -> how many representable floats apart (same sign assumed or both near zero)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


# ---- the carving scenes: create_dense((0, 0, 0), 1/32, 1, 1, 1) = 32^3 voxels over [0, 1]^3, a 64 x 48 image --------
DENSE_ORIGIN, DENSE_VS, DENSE_SIDE = (0.0, 0.0, 0.0), 1.0 / 32.0, 1.0
IMG_W, IMG_H = 64, 48


def _look(cam_pos, yaw_deg=0.0):
    """world -> camera, the camera at cam_pos looking along +z turned about y"""
    a = np.deg2rad(yaw_deg)
    R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]], np.float64)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ np.asarray(cam_pos, np.float64)
    return E.astype(F)


def depth_plane(base):
    """a tilted plane with a zero-depth hole"""
    v, u = np.mgrid[0:IMG_H, 0:IMG_W]
    d = (base + 0.004 * (u - 31.5) + 0.003 * (v - 23.5)).astype(F)
    d[10:20, 20:30] = 0
    return d


def silhouette():
    v, u = np.mgrid[0:IMG_H, 0:IMG_W]
    return (((u - 30.0) ** 2 + (v - 22.0) ** 2) < 15.0 ** 2).astype(F)


# name -> (intrinsic4, extrinsic, image)
def carve_scenes():
    return {
        "front": ((60.0, 60.0, 31.5, 23.5), _look((0.5, 0.5, -1.5)), depth_plane(2.0)),
        "inside": ((20.0, 20.0, 31.5, 23.5), _look((0.5, 0.5, 0.5)), depth_plane(0.25)),
        "partial": ((60.0, 60.0, 31.5, 23.5), _look((1.2, 0.5, -1.0), 7.0), depth_plane(1.6)),
        "silhouette": ((60.0, 60.0, 31.5, 23.5), _look((0.5, 0.5, -1.5)), silhouette()),
    }


# ---- the voxelise -> merge -> carve -> query scene of the C++ and pybind11 tests ----------------------------------------
def scene_inputs():
    """a coloured cloud in the unit cube (dyadic colours: every sum exact), the front camera's depth map, queries"""
    rng = np.random.default_rng(31)
    pts = rng.random((6000, 3)).astype(F)
    col = (rng.integers(0, 1025, (6000, 3)) / 1024.0).astype(F)
    intr, E, img = carve_scenes()["front"]
    q = rng.random((2000, 3)).astype(F)
    q[5] = [np.nan, 0, 0]
    return pts, col, intr, E, img, q


def scene_expected(pts, col, intr, E, img, q, vs=DENSE_VS):
    half = len(pts) // 2
    ka, ca = from_points(pts[:half], col[:half], vs, (0, 0, 0), (1, 1, 1))
    kb, cb = from_points(pts[half:], col[half:], vs, (0, 0, 0), (1, 1, 1))
    mk, mc = merge(ka, ca, kb, cb, AVERAGE)
    ck, cc = carve(mk, mc, vs, (0, 0, 0), img, intr, E, False)
    inc, _ = query(ck, vs, (0, 0, 0), q)
    return (ka, kb), (mk, mc), (ck, cc), inc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
