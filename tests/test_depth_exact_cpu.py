"""The numpy restatement of mi_icp_create_from_depth (tests/depth_exact.py) pinned on the CPU, so that a failure of
test_gpu_depth.py can only mean the kernel: against the C oracle given the library's pose, word for word, in every case
the GPU file runs; against three images whose normals are worked out by hand; and every case is shown to contain what
it is there for."""
import numpy as np
import pytest

import depth_exact as dx
from oracle import oracle as orc

F = np.float32
DEPTH_CASES, RGBD_CASES = dx.depth_cases(), dx.rgbd_cases()


def oracle_cloud(d, K, E, color, **kw):
    kw = dict(kw)
    if "depth_cutoff" not in kw:
        kw["depth_cutoff"] = -1.0
    return orc.create_from_depth(d, K, None, color=color, pose=dx.pose_of(E), **kw)


def check(d, K, E, color, kw):
    gp, gn, gc, pix = dx.cloud(d, K, E, color=color, **kw)
    rp, rn, rc = oracle_cloud(d, K, E, color, **kw)
    w = d.shape[1]
    assert len(gp) == len(rp)
    for what, g, r in (("points", gp, rp), ("normals", gn, rn), ("colors", gc, rc)):
        assert (g is None) == (r is None)
        if g is not None:
            msg = dx.difference(what, r, g, pix, w)
            assert msg is None, msg
    return gp, gn, gc, pix


@pytest.mark.parametrize("c", DEPTH_CASES, ids=dx.case_id)
def test_depth_form_equals_the_oracle(c):
    d, K, E, kw, _ = dx.case_inputs(c, False)
    p, _, _, pix = check(d, K, E, None, kw)
    w, h, s = c["w"], c["h"], c["stride"]
    grid = (w // s) * (h // s)
    assert len(p) <= grid and (len(p) > 0) == (grid > 0)
    if grid >= 40 * 4:                                      # every defect kind is sampled, and each is left out
        smp = d[::s, ::s][:h // s, :w // s].reshape(-1)
        kinds = [(smp == 0).sum(), (smp < 0).sum(), np.isnan(smp).sum(), np.isposinf(smp).sum()]
        assert min(kinds) > 0, kinds
        assert len(p) == grid - sum(kinds)                 # NaN and +inf pass !(d <= 0) and are removed as points
    if c["integral"]:
        row, col = np.nonzero(np.isposinf(d))
        hit = (col == int(K[2])) & (row % s == 0) & (col % s == 0) & (row < (h // s) * s)
        assert hit.any()                                   # 0 * inf: a NaN coordinate under an accepted depth
        assert not np.isin(row[hit] * w + col[hit], pix).any()


def claims(c, d, K, E, color):
    """what a normals case is there for, counted from the restatement alone: kept pixels with a non-zero normal in the
    last column, in the last row, beside a neighbour that counted as zero, and with a flipped / an unflipped normal"""
    w, h = c["w"], c["h"]
    s = dx.structured(d, K, E, color=color, rgbd=True, depth_cutoff=c["cutoff"], compute_normals=True)
    kept = np.isfinite(s["points"]).all(1) if c["valid_only"] else np.ones(w * h, bool)
    nz = kept & (np.abs(s["normals"]) > 0).any(1)
    row, col = s["pix"] // w, s["pix"] % w
    return dict(points=int(kept.sum()), last_col=int((nz & (col == w - 1)).sum()), last_row=int((nz & (row == h - 1)).sum()),
                zeroed=int((nz & s["zeroed"]).sum()), flipped=int((nz & s["flipped"]).sum()),
                unflipped=int((nz & ~s["flipped"]).sum()))


@pytest.mark.parametrize("c", RGBD_CASES, ids=dx.case_id)
def test_rgbd_form_equals_the_oracle(c):
    d, K, E, kw, color = dx.case_inputs(c, True)
    p, n, col, pix = check(d, K, E, color, kw)
    w, h = c["w"], c["h"]
    assert (col is None) == (c["color"] is None) and (n is None) == (not c["normals"])
    if c["valid_only"]:
        assert np.isfinite(p).all() and 0 < len(p)
        assert len(p) < w * h or w * h < 40
    else:
        assert len(p) == w * h
        if col is not None and w * h >= 40:                # a rejected pixel's colour is +inf; a depth of +inf is accepted
            rej = ~np.isfinite(p).all(1)                   # where no cutoff rejects it: no finite point, but its own colour
            assert np.isposinf(col[rej]).all(1).any()
            assert np.isfinite(col[rej]).all(1).any() == (c["cutoff"] <= 0)    # (a cutoff rejects the depth +inf)
    if w * h >= 40:
        smp = d.reshape(-1)
        assert min((smp == 0).sum(), (smp < 0).sum(), np.isnan(smp).sum(), np.isposinf(smp).sum()) > 0
        if c["cutoff"] > 0:
            fin = smp[np.isfinite(smp)]
            assert (fin >= c["cutoff"]).sum() > w * h // 10 and ((fin > 0) & (fin < c["cutoff"])).sum() > w * h // 10
    if c["normals"]:
        k = claims(c, d, K, E, color)
        print("%s: %s" % (dx.case_id(c), k))
        assert k["points"] == len(p)
        assert k["last_row"] > 0 and k["last_col"] > 0
        if w * h >= 40:
            assert k["zeroed"] > 0
        if c["extrinsic"] == "rigid":
            assert k["flipped"] > 0 and k["unflipped"] > 0
    if c["integral"]:
        at = (h // 3) * w + w // 2
        assert np.isposinf(d.reshape(-1)[at]) and K[2] == w // 2
        assert np.isnan(p[pix == at]).any()                # valid_only = 0: the NaN is written


def test_u16_rule_equals_the_oracle():
    u = dx.u16_image()
    assert u.max() == 65535 and u.min() == 0
    counts = []
    for scale, trunc in dx.U16_PARAMS:
        f = dx.u16_to_float(u, scale, trunc)
        p, _, _, pix = dx.cloud(f, dx.U16_K, None)
        rp, _, _ = orc.create_from_depth(u, dx.U16_K, None, depth_scale=scale, depth_trunc=trunc, pose=np.eye(4))
        msg = dx.difference("points", rp, p, pix, 70)
        assert msg is None, msg
        counts.append(len(p))
    assert counts[0] > counts[1] > counts[3] > counts[2] > 0      # dropped from: never, 3000, 4 * 500 = 2000, 2 * 999 = 1998
    f29, f2 = dx.u16_to_float(u, 1000.0, 2.9), dx.u16_to_float(u, 1000.0, 2.0)
    assert dx.same_words(f29, f2)                                       # depth_trunc is held as an int
    assert f2[3, 6] > 0 and f2[3, 7] == 0                               # 1999 stays, 2000 goes


def test_same_words_is_strict():
    a = np.array([[0.0, np.inf, np.nan], [1.0, -0.0, -np.inf]], F)
    b = a.copy()
    assert dx.same_words(a, b) and dx.difference("x", a, b, [0, 1], 1) is None
    b.view(np.uint32)[0, 2] ^= 1 | (1 << 31)                            # another NaN: the same place is enough
    assert np.isnan(b[0, 2]) and dx.same_words(a, b)
    for at, v in (((1, 1), 0.0), ((0, 1), -np.inf), ((0, 2), 0.0), ((1, 0), np.nan), ((1, 0), np.nextafter(F(1), F(2)))):
        c = a.copy()
        c[at] = v
        assert not dx.same_words(a, c)
        assert "pixel %d " % (7 + at[0]) in dx.difference("x", c, a, [7, 8], 5)
    assert not dx.same_words(a, a[:1]) and "rows" in dx.difference("x", a[:1], a, [0, 1], 1)


# ---- three images worked by hand -------------------------------------------------------------------------------------
# fx = fy = 1, cx = cy = 0, the identity pose: the point of pixel (row, col) with depth d is (col*d, row*d, d).
# With l, r, u, d the points of pixels pix-1, pix+1, pix-width, pix+width (zero past the image, zero where rejected):
#   h = l - r, v = u - d, c = (h1*v2 - h2*v1, h2*v0 - h0*v2, h0*v1 - h1*v0), n = c / sqrtf(c.c), times -1 where n2 > 0.
# Below, per pixel with row >= 1 and col >= 1: l, r, u, d -> h, v -> c, and the literal written is (c after the flip,
# c.c); signed zeros as IEEE gives them (x - x = +0, 0 * -2 = -0, +0 * -1 = -0).
def unit(c, cc):
    return (np.array(c, F) / np.sqrt(F(cc))).astype(F)


Z = (0.0, 0.0, 0.0)
HAND = {
    # 3x3, depth 1 except (2,0) = 2: P(2,0) = (0,4,2), else P(row,col) = (col,row,1)
    "wrap": [Z, Z, Z,
             Z,
             # (1,1): l (0,1,1) r (2,1,1) u (1,0,1) d (1,2,1): h (-2,0,0) v (0,-2,0): c (0,0,4), n (0,0,1), flipped
             unit((-0.0, -0.0, -4.0), 16),
             # (1,2), last column: l (1,1,1) r = pixel 6 = (2,0): (0,4,2); u (2,0,1) d (2,2,1): h (1,-3,-1) v (0,-2,0):
             # c0 = -3*0 - -1*-2 = -0 - 2 = -2; c1 = -1*0 - 1*0 = -0 - 0 = -0; c2 = 1*-2 - -3*0 = -2 - -0 = -2
             unit((-2.0, -0.0, -2.0), 8),
             Z,
             # (2,1), last row: l (0,4,2) r (2,2,1) u (1,1,1) d zero: h (-2,2,1) v (1,1,1): c (2-1, 1+2, -2-2) = (1,3,-4)
             unit((1.0, 3.0, -4.0), 26),
             # (2,2), last pixel: l (1,2,1) r zero u (2,1,1) d zero: h (1,2,1) v (2,1,1): c (2-1, 2-1, 1-4) = (1,1,-3)
             unit((1.0, 1.0, -3.0), 11)],
    # 4x3 (width 4), depth 1 except (1,1) = 2: P(1,1) = (2,2,2)
    "last": [Z, Z, Z, Z,
             Z,
             # (1,1): l (0,1,1) r (2,1,1) u (1,0,1) d (1,2,1): h (-2,0,0) v (0,-2,0): c (0,0,4), flipped
             unit((-0.0, -0.0, -4.0), 16),
             # (1,2): l (2,2,2) r (3,1,1) u (2,0,1) d (2,2,1): h (-1,1,1) v (0,-2,0): c0 = 1*0 - 1*-2 = 2;
             # c1 = 1*0 - -1*0 = 0 - -0 = 0; c2 = -1*-2 - 1*0 = 2: n2 > 0, flipped
             unit((-2.0, -0.0, -2.0), 8),
             # (1,3), last column: l (2,1,1) r = pixel 8 = (2,0): (0,2,1); u (3,0,1) d (3,2,1): h (2,-1,0) v (0,-2,0):
             # c0 = -1*0 - 0*-2 = -0 - -0 = 0; c1 = 0*0 - 2*0 = 0; c2 = 2*-2 - -1*0 = -4
             unit((0.0, 0.0, -4.0), 16),
             Z,
             # (2,1), last row: l (0,2,1) r (2,2,1) u (2,2,2) d zero: h (-2,0,0) v (2,2,2): c (0-0, 0+4, -4-0) = (0,4,-4)
             unit((0.0, 4.0, -4.0), 32),
             # (2,2): l (1,2,1) r (3,2,1) u (2,1,1) d zero: h (-2,0,0) v (2,1,1): c (0-0, 0+2, -2-0) = (0,2,-2)
             unit((0.0, 2.0, -2.0), 8),
             # (2,3), last pixel: l (2,2,1) r zero u (3,1,1) d zero: h (2,2,1) v (3,1,1): c (2-1, 3-2, 2-6) = (1,1,-4)
             unit((1.0, 1.0, -4.0), 18)],
    # 3x3, depth 1 except (1,0) = 0: rejected, its point +inf, as a neighbour zero
    "hole": [Z, Z, Z,
             Z,
             # (1,1): l rejected = zero, r (2,1,1) u (1,0,1) d (1,2,1): h (-2,-1,-1) v (0,-2,0): c0 = -1*0 - -1*-2 = -2;
             # c1 = -1*0 - -2*0 = -0 - -0 = 0; c2 = -2*-2 - -1*0 = 4: n2 > 0, flipped
             unit((2.0, -0.0, -4.0), 20),
             # (1,2), last column: l (1,1,1) r = pixel 6 = (2,0): (0,2,1); u (2,0,1) d (2,2,1): h (1,-1,0) v (0,-2,0):
             # c0 = -1*0 - 0*-2 = -0 - -0 = 0; c1 = 0*0 - 1*0 = 0; c2 = 1*-2 - -1*0 = -2
             unit((0.0, 0.0, -2.0), 4),
             Z,
             # (2,1): l (0,2,1) r (2,2,1) u (1,1,1) d zero: h (-2,0,0) v (1,1,1): c (0-0, 0+2, -2-0) = (0,2,-2)
             unit((0.0, 2.0, -2.0), 8),
             # (2,2): l (1,2,1) r zero u (2,1,1) d zero: c (1,1,-3)
             unit((1.0, 1.0, -3.0), 11)],
}


@pytest.mark.parametrize("name,depth", dx.hand_images(), ids=[n for n, _ in dx.hand_images()])
def test_hand_worked_normals(name, depth):
    want = np.array(HAND[name], F)
    h, w = depth.shape
    p, n, _, pix = dx.cloud(depth, dx.HAND_K, None, rgbd=True, compute_normals=True, valid_only=False)
    assert (pix == np.arange(w * h)).all()
    msg = dx.difference("normals", n, want, pix, w)
    assert msg is None, msg
    rp, rn, _ = orc.create_from_depth(depth, dx.HAND_K, None, rgbd=True, compute_normals=True, valid_only=False, pose=np.eye(4))
    assert dx.same_words(rn, want) and dx.same_words(rp, p)
    y, x = np.mgrid[0:h, 0:w]
    pts = np.stack([x * depth, y * depth, depth], -1).reshape(-1, 3).astype(F)
    pts[depth.reshape(-1) <= 0] = np.inf
    assert dx.same_words(p, pts)


def test_convention_images_equal_the_oracle():
    for name, d, K, cutoff in dx.convention_images():
        for valid_only in (False, True):
            kw = dict(rgbd=True, depth_cutoff=cutoff, compute_normals=True, valid_only=valid_only)
            _, n, _, pix = check(d, K, None, None, kw)
            if not valid_only:
                n = n.reshape(d.shape + (3,))
                assert (n[0] == 0).all() and (n[:, 0] == 0).all()          # first row / column: zero normal
                assert np.abs(n[-1, 1:]).sum() > 0                          # last row: lower neighbour taken as zero
                assert np.abs(n[1:, -1]).sum() > 0                          # last column: the next row's first pixel


def test_pose_inverts_the_extrinsic():
    """invert4 of the general extrinsic (last row not 0 0 0 1) inverts it; of the identity, and of no extrinsic, it is
    the identity to the word"""
    E = dx.extrinsic_of("general")
    P = dx.invert4(E)
    assert np.abs(P.astype(np.float64) @ E.astype(np.float64) - np.eye(4)).max() < 1e-6
    assert dx.same_words(dx.invert4(np.eye(4, dtype=F)), np.eye(4, dtype=F))
    assert dx.same_words(dx.pose_of(None), np.eye(4, dtype=F))
