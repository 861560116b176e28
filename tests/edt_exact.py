"""The contract of geometry::DistanceTransform (include/mi_icp.h) restated in numpy: the cell rule of the VoxelGrid form
(fp32, in the stated order), the query rule, the distance formula, and the exact squared-distance field of a site set by
two engines -- brute force in int64 for small inputs, and scipy.ndimage.distance_transform_edt (an outside
implementation) with d2 recomputed in integers from the indices it returns.  valid_nearest is the checker every test
uses: a reported index must be a site and its squared distance the field's minimum; which of several equidistant sites
is reported is not part of the contract."""
import numpy as np

F = np.float32


def floor_int(v):
    """floor(.) of fp32 values as int64, held inside +-1e9 first"""
    v = np.asarray(v, F)
    return np.clip(np.nan_to_num(np.floor(v), nan=-1.0e9, posinf=1.0e9, neginf=-1.0e9), -1.0e9, 1.0e9).astype(np.int64)


def cells_of_keys(keys, vs, origin_grid, origin_dt, res):
    """form 2: floor((((float)key * vs + origin_grid) - origin_dt) / vs) + h per axis, every step rounded to fp32"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    vs = F(vs)
    p = (keys.astype(F) * vs).astype(F)
    p = (p + np.asarray(origin_grid, F).reshape(1, 3)).astype(F)
    p = (p - np.asarray(origin_dt, F).reshape(1, 3)).astype(F)
    return floor_int((p / vs).astype(F)) + res // 2


def cells_of_points(q, vs, origin, res):
    """the query rule: floor((q - origin) / vs) + h per axis"""
    q = np.asarray(q, F).reshape(-1, 3)
    d = (q - np.asarray(origin, F).reshape(1, 3)).astype(F)
    return floor_int((d / F(vs)).astype(F)) + res // 2


def inside(cells, res):
    cells = np.asarray(cells).reshape(-1, 3)
    return ((cells >= 0) & (cells < res)).all(axis=1)


def site_set(cells, res):
    """the distinct cells inside the grid, ascending in linear index, int64 [m, 3]; and the number dropped"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    keep = inside(cells, res)
    c = cells[keep]
    lin = np.unique((c[:, 0] * res + c[:, 1]) * res + c[:, 2])
    return np.stack([lin // (res * res), (lin // res) % res, lin % res], axis=1), int((~keep).sum())


def distance(d2, vs):
    """sqrtf((float)d2) * voxel_size in fp32; d2 < 0 means no site: +inf"""
    d2 = np.asarray(d2, np.int64)
    out = (np.sqrt(np.maximum(d2, 0).astype(F)) * F(vs)).astype(F)
    return np.where(d2 < 0, F(np.inf), out).astype(F)


def grid_cells(res):
    """every cell of the grid in linear order, int64 [res^3, 3]"""
    a = np.arange(res, dtype=np.int64)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def d2_brute(sites, cells):
    """min over the sites of the squared distance to each cell, int64; -1 everywhere without a site"""
    sites = np.asarray(sites, np.int64).reshape(-1, 3)
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    if len(sites) == 0:
        return np.full(len(cells), -1, np.int64)
    out = np.full(len(cells), np.iinfo(np.int64).max, np.int64)
    step = max(1, (1 << 22) // max(1, len(cells)))
    for s in range(0, len(sites), step):
        d = cells[:, None, :] - sites[None, s:s + step, :]
        out = np.minimum(out, (d * d).sum(axis=2).min(axis=1))
    return out


def field_brute(sites, res):
    return d2_brute(sites, grid_cells(res))


def field_scipy(sites, res):
    """the same field through scipy's exact EDT: d2 recomputed in integers from the indices of the nearest site"""
    from scipy import ndimage
    sites = np.asarray(sites, np.int64).reshape(-1, 3)
    if len(sites) == 0:
        return np.full(res ** 3, -1, np.int64)
    free = np.ones((res, res, res), bool)
    free[sites[:, 0], sites[:, 1], sites[:, 2]] = False
    idx = ndimage.distance_transform_edt(free, return_distances=False, return_indices=True).astype(np.int64)
    d = idx.reshape(3, -1).T - grid_cells(res)
    return (d * d).sum(axis=1)


def field(sites, res):
    """the exact field of a site set: brute force while it is cheap, scipy beyond"""
    return field_brute(sites, res) if len(sites) * res ** 3 <= (1 << 24) else field_scipy(sites, res)


def valid_nearest(nearest, sites, d2, cells=None, res=None):
    """every reported index is a site and lies at the field's minimum from its cell (cells: the cells asked about, the
    whole grid of `res` by default); where d2 < 0 (no site) the index must be (-1, -1, -1).  -> (ok, message)"""
    nearest = np.asarray(nearest, np.int64).reshape(-1, 3)
    d2 = np.asarray(d2, np.int64).reshape(-1)
    cells = grid_cells(res) if cells is None else np.asarray(cells, np.int64).reshape(-1, 3)
    if not (len(nearest) == len(d2) == len(cells)):
        return False, "sizes differ"
    none = d2 < 0
    if not (nearest[none] == -1).all():
        return False, "an index where there is no site"
    have = ~none
    if not have.any():
        return True, ""
    sites = np.asarray(sites, np.int64).reshape(-1, 3)
    big = int(max(sites.max(), nearest.max(), 0)) + 2
    key = lambda a: (a[:, 0] * big + a[:, 1]) * big + a[:, 2]
    n = nearest[have]
    if (n < 0).any() or not np.isin(key(n), key(sites)).all():
        return False, "%d reported indices are no sites" % int((~np.isin(key(n), key(sites))).sum())
    d = n - cells[have]
    got = (d * d).sum(axis=1)
    if not (got == d2[have]).all():
        bad = np.flatnonzero(got != d2[have])
        return False, "%d cells are not at the minimum, first %s: %d against %d" % (len(bad), cells[have][bad[0]], got[bad[0]], d2[have][bad[0]])
    return True, ""


# ---- the scene the C++ and pybind11 surfaces run: a cloud voxelised on a lattice that is no multiple of the voxel size, into
# a transform of 65^3 around another origin
SCENE_RES, SCENE_VS = 65, 0.1
SCENE_LO = np.array([-3.013, -2.987, -3.041], F)
SCENE_ORIGIN = np.array([0.31, -0.17, 0.052], F)


def scene_points():
    rng = np.random.default_rng(65)
    shell = rng.normal(size=(2500, 3))
    shell = shell / np.linalg.norm(shell, axis=1, keepdims=True) * 2.2
    return np.concatenate([shell, rng.uniform(-2.98, 2.98, (600, 3))]).astype(F)


def scene_check(keys, nearest, dist):
    """the plane (nearest [res^3, 3], dist [res^3]) is the exact field of the cells of `keys`; -> the number of sites"""
    cells = cells_of_keys(keys, SCENE_VS, SCENE_LO, SCENE_ORIGIN, SCENE_RES)
    sites, dropped = site_set(cells, SCENE_RES)
    assert len(sites) > 500 and dropped > 0          # the scene crosses the transform's border
    d2 = field(sites, SCENE_RES)
    want = distance(d2, SCENE_VS)
    dist = np.ascontiguousarray(dist, F)
    assert dist.shape == want.shape and (dist.view(np.uint32) == want.view(np.uint32)).all()
    ok, msg = valid_nearest(nearest, sites, d2, res=SCENE_RES)
    assert ok, msg
    return len(sites)
