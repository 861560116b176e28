"""tests/sgm_exact.py is what the GPU's stereo results are held to bit for bit, so it is not trusted blind: the census
against words worked out by hand, the recurrence against a scalar loop, the whole against the truth of a synthetic
pair, and the comparison's sharpness against deliberately wrong variants.  No GPU."""
import numpy as np
import pytest

import sgm_exact as sx


def test_census_of_hand_written_ramps():
    ramp = np.arange(63, dtype=np.uint8).reshape(7, 9)          # raster order: every earlier pixel is darker
    live = np.zeros((7, 9), np.uint32)
    assert np.array_equal(sx.census(ramp), live)                # I(earlier) > I(later) never holds
    live[3, 4] = 0x7FFFFFFF
    assert np.array_equal(sx.census(62 - ramp), live)           # ... and always holds in the mirror; bit 31 stays clear
    # a ramp along x alone: the bit of (dy, dx) is set iff dx > 0 -- bits 5 .. 8 of each of the three 9-bit rows above
    # the centre's, none of the centre row's four
    across = np.tile(np.arange(9, dtype=np.uint8), (7, 1))
    assert sx.census(across)[3, 4] == 0x1E0 | 0x1E0 << 9 | 0x1E0 << 18 == 0x783C1E0
    # its mirror: dx < 0 -- bits 0 .. 3 of each row and the centre row's four, bits 27 .. 30
    assert sx.census(8 - across)[3, 4] == 0xF | 0xF << 9 | 0xF << 18 | 0xF << 27 == 0x783C1E0F
    assert not sx.census(np.full((6, 20), 7, np.uint8)).any() and not sx.census(np.full((20, 8), 7, np.uint8)).any()
    wide = sx.census(np.random.default_rng(0).integers(0, 256, (9, 12)).astype(np.uint8))
    assert not wide[:3].any() and not wide[-3:].any() and not wide[:, :4].any() and not wide[:, -4:].any()


def _row_by_hand(c, p1, p2):
    """L along one row from left to right, the recurrence written out term by term"""
    w, D = c.shape
    L = [[0] * D for _ in range(w)]
    for x in range(w):
        for d in range(D):
            if x == 0:
                L[x][d] = int(c[x][d])
                continue
            prev = L[x - 1]
            m = min(prev)
            terms = [prev[d], m + p2]
            if d - 1 >= 0:
                terms.append(prev[d - 1] + p1)
            if d + 1 <= D - 1:
                terms.append(prev[d + 1] + p1)
            L[x][d] = int(c[x][d]) + min(terms) - m
    return np.array(L)


@pytest.mark.parametrize("p1,p2", [(10, 120), (0, 0), (224, 224), (3, 7)])
def test_one_row_aggregation_is_the_recurrence(p1, p2):
    rng = np.random.default_rng(p1 + p2)
    c = rng.integers(0, 32, (1, 23, 64)).astype(np.uint8)
    hand = _row_by_hand(c[0], p1, p2)
    assert np.array_equal(sx.aggregate(c, 0, 1, p1, p2)[0], hand)
    assert np.array_equal(sx.aggregate(c[:, ::-1], 0, -1, p1, p2)[0, ::-1], hand)
    assert hand.max() <= 255                                    # p2 <= 224 keeps a path cost within a byte
    # a one-row image: every vertical and diagonal path starts anew at every pixel
    for dy, dx in sx.PATHS8[2:]:
        assert np.array_equal(sx.aggregate(c, dy, dx, p1, p2), c)
    # a column walked downwards is the same recurrence
    assert np.array_equal(sx.aggregate(c.transpose(1, 0, 2), 1, 0, p1, p2)[:, 0], hand)


def test_diagonal_paths_restart_at_the_side_border():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 32, (5, 4, 64)).astype(np.uint8)
    L = sx.aggregate(c, 1, 1)
    assert np.array_equal(L[:, 0], c[:, 0]) and np.array_equal(L[0], c[0])
    # the diagonal from (0, 0): (1, 1), (2, 2), (3, 3) -- the same values as a row holding those pixels
    diag = np.stack([c[i, i] for i in range(4)])[None]
    assert np.array_equal(np.stack([L[i, i] for i in range(4)]), sx.aggregate(diag, 0, 1)[0])
    L = sx.aggregate(c, -1, -1)
    assert np.array_equal(L[:, 3], c[:, 3]) and np.array_equal(L[4], c[4])


def test_the_contract_is_stereo_matching():
    left, right, truth = sx.pair(320, 120, 3)
    out = sx.sgm(left, right)
    valid = out != 255
    near = np.abs(out.astype(np.int32) - truth) <= 1
    print("valid %.4f, of those within 1 of the truth %.4f" % (valid.mean(), near[valid].mean()))
    assert valid.mean() >= 0.90
    assert near[valid].mean() >= 0.95


def test_wrong_variants_differ():
    left, right, _ = sx.pair(130, 40, 3)
    good = sx.sgm(left, right)
    for wrong in (dict(wrong_order=True), dict(wrong_reach=2), dict(wrong_last=True), dict(wrong_median_last=True)):
        assert (sx.sgm(left, right, **wrong) != good).any(), wrong


def test_small_maps_and_the_median_rules():
    m = np.array([[1, 9, 3], [0xFFFF, 5, 7], [2, 0xFFFF, 4]], np.uint16)
    out = sx.median3(m)
    assert out[1, 1] == 5 and np.array_equal(np.delete(out.reshape(-1), 4), np.delete(m.reshape(-1), 4))
    assert np.array_equal(sx.median3(m[:2]), m[:2])
    left, right, _ = sx.pair(2, 2, 1)
    assert sx.sgm(left, right, disp_size=64).shape == (2, 2)


def test_points_from_disparity_words():
    disp = np.array([[0, 4], [16, 255]], np.uint8)
    color = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    pts, col = sx.points_from_disparity(disp, color, 2.0, 2.0, 1.0, 1.0, 1.0, 0.5)
    # fx = fy = 2, tx = -0.5: q00 = q11 = -1, q03 = q13 = 1, q23 = -2, q32 = -2, q33 = 0
    assert not np.isfinite(pts[0]).all()                        # w = 0
    assert np.array_equal(pts[1], np.array([0.0, -0.125, 0.25], np.float32))      # u = 1, v = 0, w = -8
    assert np.array_equal(pts[2], np.array([-0.03125, 0.0, 0.0625], np.float32))  # u = 0, v = 1, w = -32
    assert col[3, 2] == np.float32(11) / np.float32(255)
