"""Thin object wrapper over the C ABI (include/mi_icp.h).

Inputs may be numpy arrays (host memory, copied by the engine) or torch CUDA
tensors (read in place on the device).  4x4 transforms are row-major numpy at
this level (what a user writes); the C ABI takes Eigen's column-major layout,
so they are transposed on the way in and out.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MI_ICP_DEVICE, MI_ICP_HOST, MiIcpError, Params, Result

try:  # torch is plumbing (device memory, streams), not a hard requirement of the host path
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_tensor(a):
    return torch is not None and isinstance(a, torch.Tensor)


class _Buf:
    """A float32/int32 array argument: keeps the backing object alive and exposes
    (pointer, mem_kind) and, for a device array, its torch device."""

    def __init__(self, a, dtype, cols, device_index, copy=False):
        self.keep = None
        self.ptr = None
        self.kind = MI_ICP_HOST
        self.device = None
        self.n = 0
        if a is None:
            return
        if _is_tensor(a):
            tdt = {np.float32: torch.float32, np.int32: torch.int32}[dtype]
            t = a
            if t.dtype != tdt:
                t = t.to(tdt)
            t = t.reshape(-1, cols).contiguous()
            if t.is_cuda:
                if t.device.index != device_index:
                    raise MiIcpError("tensor on cuda:%s passed to an engine on cuda:%s"
                                     % (t.device.index, device_index))
                self.kind = MI_ICP_DEVICE
                self.device = t.device
                self.ptr = C.c_void_p(t.data_ptr())
            else:
                t = t.numpy()
                self.ptr = t.ctypes.data_as(C.c_void_p)
            self.keep = t
            self.n = int(t.shape[0])
        else:
            arr = np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1, cols))
            if copy and np.shares_memory(arr, a):
                arr = arr.copy()
            self.keep = arr
            self.ptr = arr.ctypes.data_as(C.c_void_p)
            self.n = int(arr.shape[0])


def _T_in(T):
    if T is None:
        return None, None
    if _is_tensor(T):
        T = T.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T)
    return a, a.ctypes.data_as(C.c_void_p)


def _T_out(buf16):
    return np.array(buf16, dtype=np.float32).reshape(4, 4).T.copy()


class Engine:
    """One mi_icp context = one GPU."""

    def __init__(self, device=0, use_torch_stream=True):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._L.mi_icp_create(int(device), C.byref(self._ctx))
        if rc != 0:
            self._ctx = None
            raise MiIcpError("mi_icp_create(device=%d) failed with status %d "
                             "(no MI355X visible?)" % (device, rc))
        self.device = int(device)
        self.n_source = 0
        self.n_target = 0
        if use_torch_stream and torch is not None and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                self.set_stream(torch.cuda.current_stream().cuda_stream)

    # -- plumbing --------------------------------------------------------------
    def _chk(self, rc):
        if rc < 0:
            msg = self._L.mi_icp_last_error(self._ctx)
            err = MiIcpError("mi_icp error %d: %s" % (rc, (msg or b"").decode()))
            err.code = int(rc)
            raise err
        return rc

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.mi_icp_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._chk(self._L.mi_icp_set_stream(self._ctx, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        self._chk(self._L.mi_icp_synchronize(self._ctx))

    def _same_kind(self, *bufs):
        kinds = {b.kind for b in bufs if b.ptr is not None}
        if len(kinds) > 1:
            raise MiIcpError("all arrays of one call must live on the same side (host or device)")
        return kinds.pop() if kinds else MI_ICP_HOST

    @staticmethod
    def _out(kind, device, shape, dtype=np.float32):
        """an empty output array: a torch tensor on `device` (MI_ICP_DEVICE) or a numpy array; (array, pointer)"""
        if kind == MI_ICP_DEVICE:
            tdt = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}[dtype]
            t = torch.empty(shape, dtype=tdt, device=device)
            return t, C.c_void_p(t.data_ptr())
        a = np.empty(shape, dtype)
        return a, a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _trim(t, k):
        return None if t is None else t[:k]

    # -- clouds ------------------------------------------------------------------
    def _set_cloud(self, fn, points, normals, covariances):
        """mi_icp_set_target / mi_icp_set_source; returns the cloud's size"""
        self.generation = getattr(self, "generation", 0) + 1   # the clouds changed (registration._generic_icp)
        p = _Buf(points, np.float32, 3, self.device)
        n = _Buf(normals, np.float32, 3, self.device)
        c = _Buf(_cov_in(covariances), np.float32, 9, self.device)
        kind = self._same_kind(p, n, c)
        self._chk(fn(self._ctx, p.ptr, n.ptr, c.ptr, p.n, kind))
        self.synchronize()  # the staging copies above may be freed by the caller now
        return p.n

    def set_target(self, points, normals=None, covariances=None):
        self.n_target = self._set_cloud(self._L.mi_icp_set_target, points, normals, covariances)

    def set_source(self, points, normals=None, covariances=None):
        self.n_source = self._set_cloud(self._L.mi_icp_set_source, points, normals, covariances)

    # -- KDTreeFlann-style search against the target ---------------------------------------
    def search_knn(self, queries, knn, radius=0.0):
        """(found, idx[nq, knn] int32, d2[nq, knn] float32): the knn nearest target points of
        every query (within `radius` when > 0), ascending; -1 / +inf padding.  Replaces the
        context's source cloud."""
        q = _Buf(queries, np.float32, 3, self.device)
        knn = int(knn)
        idx, ip = self._out(q.kind, q.device, (q.n, knn), np.int32)
        d2, dp = self._out(q.kind, q.device, (q.n, knn))
        found = C.c_int64(0)
        self._chk(self._L.mi_icp_search_knn(self._ctx, q.ptr, q.n, knn, float(radius), ip, dp,
                                            C.byref(found), q.kind))
        self.n_source = q.n
        self.generation = getattr(self, "generation", 0) + 1
        return int(found.value), idx, d2

    # -- colored ICP --------------------------------------------------------------------
    def set_target_colors(self, colors):
        b = _Buf(colors, np.float32, 3, self.device)
        if b.n and b.n != self.n_target:
            raise MiIcpError("set_target_colors: %d colours for %d target points" % (b.n, self.n_target))
        self._chk(self._L.mi_icp_set_target_colors(self._ctx, b.ptr, b.kind))
        self.synchronize()

    def set_source_colors(self, colors):
        b = _Buf(colors, np.float32, 3, self.device)
        if b.n and b.n != self.n_source:
            raise MiIcpError("set_source_colors: %d colours for %d source points" % (b.n, self.n_source))
        self._chk(self._L.mi_icp_set_source_colors(self._ctx, b.ptr, b.kind))
        self.synchronize()

    def set_lambda_geometric(self, lambda_geometric):
        self._chk(self._L.mi_icp_set_lambda_geometric(self._ctx, float(lambda_geometric)))

    def compute_color_gradients(self, radius, max_nn=30, want_output=True):
        """InitializePointCloudForColoredICP; returns the gradients (target's original
        order, numpy) when want_output."""
        out, optr = self._out(MI_ICP_HOST, None, (self.n_target, 3)) if want_output else (None, None)
        self._chk(self._L.mi_icp_compute_color_gradients(self._ctx, float(radius), int(max_nn), optr,
                                                         MI_ICP_HOST))
        return out

    def registration_colored_icp(self, max_distance, init=None, relative_fitness=1e-6,
                                 relative_rmse=1e-6, max_iteration=30, lambda_geometric=0.968,
                                 det_thresh=1e-6):
        res = Result()
        prm = Params(float(relative_fitness), float(relative_rmse), int(max_iteration),
                     float(det_thresh))
        _, tp = _T_in(init)
        self._chk(self._L.mi_icp_registration_colored_icp(self._ctx, float(max_distance), tp,
                                                          C.byref(prm), float(lambda_geometric),
                                                          C.byref(res)))
        return res

    def morton_order(self, points):
        """order[s] = original index of the s-th point of the engine's spatial (Morton) order;
        numpy int64.  points: numpy or a torch tensor on the engine's device (sorted there)."""
        p = _Buf(points, np.float32, 3, self.device)
        if p.n == 0:
            return np.zeros(0, np.int64)
        out, optr = self._out(p.kind, p.device, (p.n,), np.int32)
        self._chk(self._L.mi_icp_spatial_order(self._ctx, p.ptr, p.n, optr, p.kind))
        if p.kind == MI_ICP_DEVICE:
            out = out.cpu().numpy()
        return out.view(np.uint32).astype(np.int64)

    def set_global_source_count(self, n_total):
        self._chk(self._L.mi_icp_set_global_source_count(self._ctx, int(n_total)))

    # -- search ---------------------------------------------------------------------
    def search_radius_1nn(self, radius, T=None, want_d2=True):
        """(indices[int32 n], d2[float32 n], stats) in original source order;
        -1 / +inf where no target point lies within `radius` (strict)."""
        idx, ip = self._out(MI_ICP_HOST, None, (self.n_source,), np.int32)
        d2, dp = self._out(MI_ICP_HOST, None, (self.n_source,)) if want_d2 else (None, None)
        stats = np.zeros(3, np.float64)
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_search_radius_1nn(self._ctx, tp, float(radius), ip, dp, MI_ICP_HOST,
                                                   stats.ctypes.data_as(C.c_void_p)))
        return idx, d2, stats

    def drop_seeds(self):
        """test hook (mi_icp_debug.h): the next search starts top-down, not from the previous matches"""
        self._chk(self._L.mi_icp_debug_drop_seeds(self._ctx))

    def loop_counters(self):
        """test hook (mi_icp_debug.h): {iterations, passes, re-locations, re-location launches armed} of the present loop"""
        out = np.zeros(4, np.int32)
        self._chk(self._L.mi_icp_debug_loop_counters(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def search_skip_state(self):
        """test hook (mi_icp_debug.h): the search skip's state of the present loop -- the odometer `travel`, the queries'
        rounding bound `fuzz`, the per-packet `limits`, `armed` (will the next search be gated at all?) and `will_skip`, the
        packets that search is going to skip: travel + fuzz < limit"""
        n, armed = C.c_int64(0), C.c_int(0)
        st = np.zeros(2, np.float64)
        self._chk(self._L.mi_icp_debug_search_skip(self._ctx, st.ctypes.data_as(C.c_void_p), None, 0, C.byref(n), C.byref(armed)))
        lim = np.zeros(n.value, np.float64)
        self._chk(self._L.mi_icp_debug_search_skip(self._ctx, st.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p),
                                                   n.value, C.byref(n), C.byref(armed)))
        with np.errstate(invalid="ignore"):
            will = (st[0] + st[1] < lim) if armed.value else np.zeros(n.value, bool)
        return {"travel": float(st[0]), "fuzz": float(st[1]), "limits": lim, "armed": bool(armed.value), "will_skip": will}

    def pair_state(self):
        """test hook (mi_icp_debug.h): the pair stream's per-packet `state` (uint8: 0, 1, 2 = record valid) and `mask`
        (uint64: the lanes with a match; meaningful in state 2) as the last launch left them"""
        n = C.c_int64(0)
        self._chk(self._L.mi_icp_debug_pair_state(self._ctx, None, None, 0, C.byref(n)))
        st, mk = np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint64)
        self._chk(self._L.mi_icp_debug_pair_state(self._ctx, st.ctypes.data_as(C.c_void_p), mk.ctypes.data_as(C.c_void_p),
                                                  n.value, C.byref(n)))
        return {"state": st, "mask": mk}

    def drop_pairs(self):
        """test hook (mi_icp_debug.h): every packet's pair state back to 0, nothing else"""
        self._chk(self._L.mi_icp_debug_drop_pairs(self._ctx))

    def last_search_kind(self):
        """test hook: 0 = the last search started at the root, 1 = from the previous matches, 2 = from its own seeds"""
        return int(self._L.mi_icp_debug_last_search_kind(self._ctx))

    def get_correspondences(self):
        cnt = C.c_int64(0)
        self._chk(self._L.mi_icp_get_correspondences(self._ctx, None, 0, C.byref(cnt), MI_ICP_HOST))
        out, optr = self._out(MI_ICP_HOST, None, (max(cnt.value, 0), 2), np.int32)
        if cnt.value > 0:
            self._chk(self._L.mi_icp_get_correspondences(self._ctx, optr, cnt.value, C.byref(cnt), MI_ICP_HOST))
        return out

    def set_correspondences(self, pairs):
        b = _Buf(pairs, np.int32, 2, self.device)
        self._chk(self._L.mi_icp_set_correspondences(self._ctx, b.ptr, b.n, b.kind))

    # -- estimation -------------------------------------------------------------------
    def compute_system(self, est, T=None):
        out = np.zeros(32, np.float64)
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_compute_system(self._ctx, int(est), tp,
                                                out.ctypes.data_as(C.c_void_p)))
        return out

    def compute_transformation(self, est, T=None, det_thresh=1e-6):
        out = (C.c_float * 16)()
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_compute_transformation(self._ctx, int(est), tp,
                                                        float(det_thresh), out))
        return _T_out(out)

    def compute_rmse(self, est, T=None):
        out = C.c_float(0)
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_compute_rmse(self._ctx, int(est), tp, C.byref(out)))
        return float(out.value)

    # -- registration --------------------------------------------------------------------
    def evaluate_registration(self, max_distance, T=None):
        res = Result()
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_evaluate_registration(self._ctx, float(max_distance), tp,
                                                       C.byref(res)))
        return res

    def registration_icp(self, est, max_distance, init=None, relative_fitness=1e-6,
                         relative_rmse=1e-6, max_iteration=30, det_thresh=1e-6):
        res = Result()
        prm = Params(float(relative_fitness), float(relative_rmse), int(max_iteration),
                     float(det_thresh))
        _, tp = _T_in(init)
        self._chk(self._L.mi_icp_registration_icp(self._ctx, int(est), float(max_distance), tp,
                                                  C.byref(prm), C.byref(res)))
        return res

    def icp_begin(self, est, max_distance, init=None, det_thresh=1e-6):
        res = Result()
        _, tp = _T_in(init)
        self._chk(self._L.mi_icp_icp_begin(self._ctx, int(est), float(max_distance), tp,
                                           float(det_thresh), C.byref(res)))
        return res

    def icp_iterate(self, n_iterations=1):
        res = Result()
        self._chk(self._L.mi_icp_icp_iterate(self._ctx, int(n_iterations), C.byref(res)))
        return res

    # -- geometry ---------------------------------------------------------------------------
    def transform(self, T, points=None, normals=None, covariances=None):
        """In place on torch CUDA tensors (as PointCloud::Transform); numpy inputs are
        left untouched and transformed copies are returned."""
        p = _Buf(points, np.float32, 3, self.device, copy=True)
        n = _Buf(normals, np.float32, 3, self.device, copy=True)
        c = _Buf(_cov_in(covariances), np.float32, 9, self.device, copy=True)
        kind = self._same_kind(p, n, c)
        cnt = max(p.n, n.n, c.n)
        _, tp = _T_in(T)
        self._chk(self._L.mi_icp_transform(self._ctx, tp, p.ptr, n.ptr, c.ptr, cnt, kind))
        return p.keep, n.keep, _cov_out(c.keep)

    def compute_bounds(self, points):
        """(min_bound, max_bound, center) of a cloud as float32 numpy vectors
        (GeometryBase3D::GetMinBound / GetMaxBound / GetCenter); zeros for an empty cloud."""
        p = _Buf(points, np.float32, 3, self.device)
        out = np.zeros((3, 3), np.float32)
        ptr = lambda r: out[r].ctypes.data_as(C.c_void_p)
        self._chk(self._L.mi_icp_compute_bounds(self._ctx, p.ptr, p.n, p.kind, ptr(0), ptr(1), ptr(2)))
        return out[0].copy(), out[1].copy(), out[2].copy()

    def affine(self, points=None, normals=None, covariances=None, R=None, scale=None, center=None, translate=None):
        """GeometryBase3D::Translate / Scale / Rotate: p <- (R (p - center)) * scale + center + translate,
        normals <- R n, covariances <- R C R^T.  In place on torch CUDA tensors; numpy inputs are left
        untouched and moved copies are returned, as Engine.transform."""
        p = _Buf(points, np.float32, 3, self.device, copy=True)
        n = _Buf(normals, np.float32, 3, self.device, copy=True)
        c = _Buf(_cov_in(covariances), np.float32, 9, self.device, copy=True)
        kind = self._same_kind(p, n, c)
        cnt = max(p.n, n.n, c.n)
        vec = lambda v: None if v is None else np.ascontiguousarray(np.asarray(v, np.float32).reshape(3))
        Rc = None if R is None else np.ascontiguousarray(np.asarray(R, np.float32).reshape(3, 3).T)   # column-major
        cv, tv = vec(center), vec(translate)
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._chk(self._L.mi_icp_affine(self._ctx, ptr(Rc), float(scale if scale is not None else 1.0),
                                        0 if scale is None else 1, ptr(cv), ptr(tv), p.ptr, n.ptr, c.ptr, cnt, kind))
        self.synchronize()
        return p.keep, n.keep, _cov_out(c.keep)

    # -- PointCloud::VoxelDownSample / SelectByIndex / UniformDownSample / Remove*Outliers (down_sample.cu), ------
    # -- ClusterDBSCAN, SegmentPlane, ComputeISSKeypoints / SelectByMask
    def _cloud_args(self, points, normals, colors):
        p = _Buf(points, np.float32, 3, self.device)
        n = _Buf(normals, np.float32, 3, self.device)
        c = _Buf(colors, np.float32, 3, self.device)
        return p, n, c, self._same_kind(p, n, c)

    def _cloud_outputs(self, kind, p, n, c, rows):
        op = self._out(kind, p.device, (rows, 3))
        on = self._out(kind, p.device, (rows, 3)) if n.ptr is not None else (None, None)
        oc = self._out(kind, p.device, (rows, 3)) if c.ptr is not None else (None, None)
        return op, on, oc

    def voxel_downsample(self, points, voxel_size, normals=None, colors=None):
        p, n, c, kind = self._cloud_args(points, normals, colors)
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, p.n)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_voxel_downsample(self._ctx, p.ptr, n.ptr, c.ptr, p.n, float(voxel_size), pp, pn, pc,
                                                  C.byref(m), kind))
        k = int(m.value)
        return (self._trim(op, k) if p.ptr is not None else np.empty((0, 3), np.float32)), self._trim(on, k), \
            self._trim(oc, k)

    def _outlier_filter(self, fn, points, k, param, normals, colors, stat_dtype):
        p, n, c, kind = self._cloud_args(points, normals, colors)
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, p.n)
        idx, pidx = self._out(kind, p.device, (p.n,), np.int64)
        stat, pstat = self._out(kind, p.device, (p.n,), stat_dtype)
        m = C.c_int64(0)
        self._chk(fn(self._ctx, p.ptr, n.ptr, c.ptr, p.n, int(k), float(param), pp, pn, pc, pidx, pstat, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k), idx[:k], stat

    def remove_statistical_outliers(self, points, nb_neighbors, std_ratio, normals=None, colors=None):
        """PointCloud::RemoveStatisticalOutliers (down_sample.cu:354-438).  Returns (points, normals or None,
        colors or None, indices int64 ascending, avg_d2 per input point), on the side of `points`."""
        return self._outlier_filter(self._L.mi_icp_remove_statistical_outliers, points, nb_neighbors, std_ratio,
                                    normals, colors, np.float32)

    def remove_radius_outliers(self, points, nb_points, radius, normals=None, colors=None):
        """PointCloud::RemoveRadiusOutliers (down_sample.cu:317-352).  Returns (points, normals or None,
        colors or None, indices int64 ascending, counts int32 per input point, capped at nb_points + 1)."""
        return self._outlier_filter(self._L.mi_icp_remove_radius_outliers, points, nb_points, radius,
                                    normals, colors, np.int32)

    def cluster_dbscan(self, points, eps, min_points, max_edges=100):
        """PointCloud::ClusterDBSCAN (pointcloud_cluster.cu:109-179; the contract is in include/mi_icp.h).
        Returns (labels int32[n], degrees int32[n], n_clusters), on the side of `points`."""
        p = _Buf(points, np.float32, 3, self.device)
        kind = self._same_kind(p)
        labels, plab = self._out(kind, p.device, (p.n,), np.int32)
        degrees, pdeg = self._out(kind, p.device, (p.n,), np.int32)
        nc = C.c_int64(0)
        self._chk(self._L.mi_icp_cluster_dbscan(self._ctx, p.ptr, p.n, float(eps), int(min_points), int(max_edges),
                                                plab, pdeg, C.byref(nc), kind))
        return labels, degrees, int(nc.value)

    def segment_plane(self, points, distance_threshold, ransac_n=3, num_iterations=100, seed=0):
        """PointCloud::SegmentPlane (segmentation.cu:187-268; the contract is in include/mi_icp.h).  Returns
        (plane float32[4] refit to the inliers, inlier indices int64 ascending on the side of `points`, the winning
        RANSAC plane float32[4], the winner's iteration or -1, its inlier count)."""
        p = _Buf(points, np.float32, 3, self.device)
        kind = self._same_kind(p)
        idx, pidx = self._out(kind, p.device, (p.n,), np.int64)
        plane, ransac = np.zeros(4, np.float32), np.zeros(4, np.float32)
        m, best, count = C.c_int64(0), C.c_int64(-1), C.c_int64(0)
        self._chk(self._L.mi_icp_segment_plane(self._ctx, p.ptr, p.n, float(distance_threshold), int(ransac_n),
                                               int(num_iterations), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                               plane.ctypes.data_as(C.c_void_p), ransac.ctypes.data_as(C.c_void_p), pidx,
                                               C.byref(m), C.byref(best), C.byref(count), kind))
        return plane, idx[:int(m.value)], ransac, int(best.value), int(count.value)

    def select_by_index(self, points, indices, invert=False, normals=None, colors=None):
        """PointCloud::SelectByIndex (down_sample.cu:40-62,110-129).  indices: anything 1-D integer (a tensor on
        the points' device, a numpy array, a list); returns (points, normals or None, colors or None)."""
        p, n, c, kind = self._cloud_args(points, normals, colors)
        if kind == MI_ICP_DEVICE:
            ix = torch.as_tensor(indices).to(device=p.device, dtype=torch.int64).reshape(-1).contiguous() \
                if _is_tensor(indices) else torch.from_numpy(np.ascontiguousarray(np.asarray(indices, np.int64).reshape(-1))).to(p.device)
            pix, nix = C.c_void_p(ix.data_ptr()), int(ix.shape[0])
        else:
            ix = indices.detach().cpu().numpy() if _is_tensor(indices) else indices
            ix = np.ascontiguousarray(np.asarray(ix, np.int64).reshape(-1))
            pix, nix = ix.ctypes.data_as(C.c_void_p), int(ix.shape[0])
        rows = p.n if invert else nix
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, rows)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_select_by_index(self._ctx, p.ptr, n.ptr, c.ptr, p.n, pix, nix, int(bool(invert)),
                                                 pp, pn, pc, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k)

    def iss_keypoints(self, points, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975,
                      min_neighbors=5, max_neighbors=100, want_response=False):
        """geometry::keypoint::ComputeISSKeypoints (iss_keypoints.cu:108-172; the contract is in include/mi_icp.h).
        Returns (mask uint8[n] on the side of `points`, the number of keypoints, (salient_radius, non_max_radius) as
        used); with want_response also saliency float32[n], eigenvalues float32[n, 3] and salient-row counts int32[n]."""
        p = _Buf(points, np.float32, 3, self.device)
        kind = self._same_kind(p)
        mask, pmask = self._out(kind, p.device, (p.n,), np.uint8)
        sal = eig = cnt = psal = peig = pcnt = None
        if want_response:
            sal, psal = self._out(kind, p.device, (p.n,), np.float32)
            eig, peig = self._out(kind, p.device, (p.n, 3), np.float32)
            cnt, pcnt = self._out(kind, p.device, (p.n,), np.int32)
        radii = np.zeros(2, np.float32)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_iss_keypoints(self._ctx, p.ptr, p.n, float(salient_radius), float(non_max_radius),
                                               float(gamma_21), float(gamma_32), int(min_neighbors), int(max_neighbors),
                                               pmask, psal, peig, pcnt, radii.ctypes.data_as(C.c_void_p), C.byref(m), kind))
        out = (mask, int(m.value), (float(radii[0]), float(radii[1])))
        return out + (sal, eig, cnt) if want_response else out

    def select_by_mask(self, points, mask, invert=False, normals=None, colors=None):
        """PointCloud::SelectByMask (down_sample.cu:131-168).  mask: anything 1-D of one truth value per point (a bool
        or uint8 tensor on the points' device, a numpy array, a list); returns (points, normals or None, colors or None)."""
        p, n, c, kind = self._cloud_args(points, normals, colors)
        if kind == MI_ICP_DEVICE:
            mk = mask if _is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0))
            mk = (mk.reshape(-1) != 0).to(device=p.device, dtype=torch.uint8).contiguous()
            pmk, nmk = C.c_void_p(mk.data_ptr()), int(mk.shape[0])
        else:
            mk = mask.detach().cpu().numpy() if _is_tensor(mask) else mask
            mk = np.ascontiguousarray((np.asarray(mk).reshape(-1) != 0).astype(np.uint8))
            pmk, nmk = mk.ctypes.data_as(C.c_void_p), int(mk.shape[0])
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, p.n)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_select_by_mask(self._ctx, p.ptr, n.ptr, c.ptr, p.n, pmk, nmk, int(bool(invert)),
                                                pp, pn, pc, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k)

    # -- FarthestPointDownSample / GaussianFilter / PassThroughFilter / Crop / RemoveNoneFinitePoints (pointcloud.cu)
    def farthest_point_downsample(self, points, num_samples, normals=None, colors=None):
        """PointCloud::FarthestPointDownSample (pointcloud.cu:122-139, 301-338; the contract is in include/mi_icp.h:
        sel[0] = 0, ties to the lowest index).  Returns (points, normals or None, colors or None, indices int64
        [num_samples] in selection order), on the side of `points`."""
        p, n, c, kind = self._cloud_args(points, normals, colors)
        rows = max(0, min(int(num_samples), p.n))
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, rows)
        idx, pidx = self._out(kind, p.device, (rows,), np.int64)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_farthest_point_downsample(self._ctx, p.ptr, n.ptr, c.ptr, p.n, int(num_samples),
                                                           pp, pn, pc, pidx, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k), idx[:k]

    def gaussian_filter(self, points, search_radius, sigma2, num_max_search_points=50, normals=None, colors=None):
        """PointCloud::GaussianFilter (pointcloud.cu:56-106, 387-434; the contract is in include/mi_icp.h).  Returns
        (points, normals or None, colors or None), one entry per input point."""
        p, n, c, kind = self._cloud_args(points, normals, colors)
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, p.n)
        self._chk(self._L.mi_icp_gaussian_filter(self._ctx, p.ptr, n.ptr, c.ptr, p.n, float(search_radius), float(sigma2),
                                                 int(num_max_search_points), pp, pn, pc, kind))
        return op, on, oc

    def _predicate_filter(self, points, normals, colors, call):
        p, n, c, kind = self._cloud_args(points, normals, colors)
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, p.n)
        idx, pidx = self._out(kind, p.device, (p.n,), np.int64)
        m = C.c_int64(0)
        self._chk(call(p, n, c, pp, pn, pc, pidx, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k), idx[:k]

    def pass_through_filter(self, points, axis_no, min_bound, max_bound, normals=None, colors=None):
        """PointCloud::PassThroughFilter (pointcloud.cu:108-120, 436-466): kept iff !(v < min_bound || max_bound < v),
        v = p[axis_no].  Returns (points, normals or None, colors or None, kept indices int64 ascending)."""
        return self._predicate_filter(points, normals, colors, lambda p, n, c, *out: self._L.mi_icp_pass_through_filter(
            self._ctx, p.ptr, n.ptr, c.ptr, p.n, int(axis_no), float(min_bound), float(max_bound), *out))

    def crop_aabb(self, points, min_bound, max_bound, normals=None, colors=None):
        """PointCloud::Crop(AxisAlignedBoundingBox) (pointcloud.cu:340-348): kept iff inside the closed box; an empty
        box is an error.  Returns as pass_through_filter."""
        lo = np.ascontiguousarray(np.asarray(min_bound, np.float32).reshape(3))
        hi = np.ascontiguousarray(np.asarray(max_bound, np.float32).reshape(3))
        return self._predicate_filter(points, normals, colors, lambda p, n, c, *out: self._L.mi_icp_crop_aabb(
            self._ctx, p.ptr, n.ptr, c.ptr, p.n, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), *out))

    def remove_none_finite(self, points, remove_nan=True, remove_infinite=True, normals=None, colors=None):
        """PointCloud::RemoveNoneFinitePoints (pointcloud.cu:40-54, 360-385) into new arrays.  Returns as
        pass_through_filter."""
        return self._predicate_filter(points, normals, colors, lambda p, n, c, *out: self._L.mi_icp_remove_none_finite(
            self._ctx, p.ptr, n.ptr, c.ptr, p.n, int(bool(remove_nan)), int(bool(remove_infinite)), *out))

    def uniform_downsample(self, points, every_k_points, normals=None, colors=None):
        """PointCloud::UniformDownSample (down_sample.cu:275-316): points 0, k, 2k, ... (n // k of them)."""
        p, n, c, kind = self._cloud_args(points, normals, colors)
        k = int(every_k_points)
        rows = p.n // k if k > 0 else 0
        (op, pp), (on, pn), (oc, pc) = self._cloud_outputs(kind, p, n, c, rows)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_uniform_downsample(self._ctx, p.ptr, n.ptr, c.ptr, p.n, k, pp, pn, pc,
                                                    C.byref(m), kind))
        return op[:int(m.value)], on, oc

    def create_from_depth(self, depth, intrinsic4, extrinsic=None, color=None, depth_scale=1000.0,
                          depth_trunc=1000.0, depth_cutoff=-1.0, stride=1, rgbd=False,
                          compute_normals=False, valid_only=True):
        """PointCloud::CreateFromDepthImage (rgbd=False) / CreateFromRGBDImage (rgbd=True),
        geometry/pointcloud_factory.cu:286-376.  depth: [H, W] float32 or uint16; color: None,
        [H, W, 3] uint8 or [H, W] float32; numpy or torch (all on the same side).
        Returns (points, normals or None, colors or None)."""
        on_dev = _is_tensor(depth) and depth.is_cuda
        def prep(x, kinds):
            if x is None:
                return None, None
            if _is_tensor(x):
                if x.dtype not in kinds:
                    raise TypeError("unsupported image dtype %s" % x.dtype)
                if x.is_cuda != on_dev:
                    raise ValueError("depth and color must live on the same side")
                x = x.contiguous() if on_dev else np.ascontiguousarray(x.numpy())
            else:
                if on_dev:
                    raise ValueError("depth and color must live on the same side")
                x = np.ascontiguousarray(x)
            return x, (C.c_void_p(x.data_ptr()) if on_dev else x.ctypes.data_as(C.c_void_p))
        if _is_tensor(depth):
            dkinds, ckinds = (torch.float32, torch.uint16), (torch.uint8, torch.float32)
        else:
            dkinds = ckinds = None
        d, dptr = prep(depth, dkinds)
        col, cptr = prep(color, ckinds)
        if d.ndim != 2:
            raise ValueError("depth must be [H, W]")
        dname = str(d.dtype).replace("torch.", "")
        if dname not in ("float32", "uint16"):
            raise TypeError("depth must be float32 or uint16")
        h, w = int(d.shape[0]), int(d.shape[1])
        ctype = 0
        if col is not None:
            cname = str(col.dtype).replace("torch.", "")
            if cname == "uint8" and tuple(col.shape) == (h, w, 3):
                ctype = 1
            elif cname == "float32" and tuple(col.shape)[:2] == (h, w) and \
                    (col.numel() if on_dev else col.size) == h * w:
                ctype = 2
            else:
                raise TypeError("[PointCloud::CreateFromRGBDImage] Unsupported image format.")
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        E = None
        if extrinsic is not None:
            E = np.ascontiguousarray(np.asarray(extrinsic, np.float32).reshape(4, 4).T)
            Eptr = E.ctypes.data_as(C.c_void_p)
        else:
            Eptr = None
        count = (w // int(stride)) * (h // int(stride)) if stride >= 1 else 0
        kind = MI_ICP_DEVICE if on_dev else MI_ICP_HOST
        out = lambda want: self._out(kind, d.device if on_dev else None, (count, 3)) if want else (None, None)
        (op, pp), (on, pn), (oc, pc) = out(True), out(compute_normals), out(col is not None)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_create_from_depth(
            self._ctx, dptr, 1 if dname == "uint16" else 0, cptr, ctype, w, h, K, Eptr,
            float(depth_scale), float(depth_trunc), float(depth_cutoff), int(stride), int(bool(rgbd)),
            int(bool(compute_normals)), int(bool(valid_only)), pp, pn, pc, C.byref(m), kind))
        k = int(m.value)
        return self._trim(op, k), self._trim(on, k), self._trim(oc, k)

    # -- integration::UniformTSDFVolume (include/mi_icp.h) ----------------------------------------------
    def tsdf_create(self, length, resolution, sdf_trunc, color_type, origin=None):
        """-> an opaque volume handle of this engine (mi_icp_tsdf_create)"""
        o = np.ascontiguousarray(np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3))
        h = C.c_void_p()
        self._chk(self._L.mi_icp_tsdf_create(self._ctx, float(length), int(resolution), float(sdf_trunc), int(color_type),
                                             o.ctypes.data_as(C.c_void_p), C.byref(h)))
        return h

    def tsdf_destroy(self, vol):
        if getattr(self, "_ctx", None) and vol:
            self._chk(self._L.mi_icp_tsdf_destroy(self._ctx, vol))

    def tsdf_reset(self, vol):
        self._chk(self._L.mi_icp_tsdf_reset(self._ctx, vol))

    @staticmethod
    def _image_desc(x, bad=None):
        """(array kept alive, pointer, width, height, channels, bytes per channel, on the device?) of an image:
        [H, W] or [H, W, C], numpy or torch; anything else raises MiIcpError(bad)"""
        if x is None:
            return None, None, 0, 0, 0, 0, None
        on_dev = _is_tensor(x) and x.is_cuda
        if _is_tensor(x):
            x = x.contiguous() if on_dev else np.ascontiguousarray(x.numpy())
        else:
            x = np.ascontiguousarray(x)
        if x.ndim not in (2, 3):
            raise MiIcpError(bad)
        bpc = int(x.element_size()) if on_dev else int(x.dtype.itemsize)
        ptr = C.c_void_p(x.data_ptr()) if on_dev else x.ctypes.data_as(C.c_void_p)
        return x, ptr, int(x.shape[1]), int(x.shape[0]), (int(x.shape[2]) if x.ndim == 3 else 1), bpc, on_dev

    def _tsdf_frame(self, label, depth, color):
        """-> (depth, color) of an Integrate call as _image_desc describes them.  A pair the reference's `label` class
        turns away raises MiIcpError("[label::Integrate] Unsupported image format.")."""
        bad = "[%s::Integrate] Unsupported image format." % label
        d, col = self._image_desc(depth, bad), self._image_desc(color, bad)
        if d[0] is None:
            raise MiIcpError(bad)
        if col[0] is not None and col[6] != d[6]:
            raise MiIcpError("depth and color must live on the same side")
        f32, u8 = (torch.float32, torch.uint8) if d[6] else (np.float32, np.uint8)
        # a float image must be float: the C ABI sees bytes per channel only
        if d[0].dtype != f32 or not (col[0] is None or col[0].dtype in (f32, u8)):
            raise MiIcpError(bad)
        return d, col

    def tsdf_integrate(self, vol, depth, color, width, height, intrinsic4, extrinsic=None):
        """UniformTSDFVolume::Integrate; depth / color numpy or torch, both on the same side.  A format the
        reference turns away raises MiIcpError."""
        d, col = self._tsdf_frame("UniformTSDFVolume", depth, color)     # (they keep the arrays alive through the call)
        (_, dptr, dw, dh, dc, db, d_dev), (_, cptr, cw, ch, cc, cb, _) = d, col
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        _, Eptr = _T_in(extrinsic)
        self._chk(self._L.mi_icp_tsdf_integrate(self._ctx, vol, dptr, dw, dh, dc, db, cptr, cw, ch, cc, cb, int(width),
                                                int(height), K, Eptr, MI_ICP_DEVICE if d_dev else MI_ICP_HOST))

    TSDF_FIRST_CAPACITY = 1 << 18   # points an extraction makes room for before it knows the count (9 MB for three arrays)

    def _tsdf_cloud(self, call, want, capacity, device):
        """the capacity rule of include/mi_icp.h: one call with room for `capacity` points, a second with the room
        the first asked for only when that was not enough"""
        kind = MI_ICP_DEVICE if device is not None else MI_ICP_HOST
        m = C.c_int64(0)
        outs = [self._out(kind, device, (capacity, 3)) if w else (None, None) for w in want]
        self._chk(call([p for _, p in outs], capacity, C.byref(m), kind))
        if int(m.value) > capacity:                     # did not fit: nothing was written, m is the room needed
            capacity = int(m.value)
            outs = [self._out(kind, device, (capacity, 3)) if w else (None, None) for w in want]
            self._chk(call([p for _, p in outs], capacity, C.byref(m), kind))
        k = int(m.value)
        return [self._trim(a, k) for a, _ in outs]

    def _tsdf_device(self, on_device):
        return torch.device("cuda", self.device) if on_device else None

    def tsdf_extract_point_cloud(self, vol, colored, on_device=True):
        """-> (points, normals, colors or None)"""
        return self._tsdf_cloud(lambda p, cap, m, kind: self._L.mi_icp_tsdf_extract_point_cloud(
            self._ctx, vol, p[0], p[1], p[2], cap, m, kind), [True, True, bool(colored)], self.TSDF_FIRST_CAPACITY, self._tsdf_device(on_device))

    def tsdf_extract_voxel_point_cloud(self, vol, on_device=True):
        """-> (points, colors)"""
        return self._tsdf_cloud(lambda p, cap, m, kind: self._L.mi_icp_tsdf_extract_voxel_point_cloud(
            self._ctx, vol, p[0], p[1], cap, m, kind), [True, True], self.TSDF_FIRST_CAPACITY, self._tsdf_device(on_device))

    def tsdf_raycast(self, vol, width, height, intrinsic4, extrinsic, sdf_trunc, valid_only=True, on_device=True):
        """-> (points, normals, colors) in pixel order; one call, with room for every pixel"""
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        keep, Eptr = _T_in(extrinsic)
        return self._tsdf_cloud(lambda p, cap, m, kind: self._L.mi_icp_tsdf_raycast(
            self._ctx, vol, int(width), int(height), K, Eptr, float(sdf_trunc), int(bool(valid_only)), p[0], p[1], p[2],
            cap, m, kind), [True, True, True], int(width) * int(height), self._tsdf_device(on_device))

    TSDF_MAX_LEVELS = 16            # MI_ICP_TSDF_MAX_LEVELS

    def tsdf_raycast_levels(self, vol, levels, width, height, intrinsic4, extrinsic, sdf_trunc, valid_only=True,
                            on_device=True):
        """-> [(points, normals, colors) of level i, in pixel order] for the `levels` levels of the camera's pyramid
        (mi_icp_tsdf_raycast_levels): one call, with room for every pixel of every level.  The levels are slices of
        three device arrays."""
        levels, width, height = int(levels), int(width), int(height)
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        keep, Eptr = _T_in(extrinsic)
        capacity = sum(max(width >> i, 0) * max(height >> i, 0) for i in range(max(0, min(levels, self.TSDF_MAX_LEVELS))))
        m = (C.c_int64 * self.TSDF_MAX_LEVELS)()
        outs = [self._out(MI_ICP_DEVICE, self._tsdf_device(True), (capacity, 3)) for _ in range(3)]
        self._chk(self._L.mi_icp_tsdf_raycast_levels(self._ctx, vol, levels, width, height, K, Eptr, float(sdf_trunc),
                                                     int(bool(valid_only)), outs[0][1], outs[1][1], outs[2][1], capacity, m))
        clouds, first = [], 0
        for i in range(levels):
            k = int(m[i])
            level = [a[first:first + k] for a, _ in outs]
            clouds.append(tuple(level if on_device else [a.cpu().numpy() for a in level]))
            first += k
        return clouds

    def tsdf_get_voxels(self, vol, n, colored, on_device=False):
        """-> (tsdf[n], weight[n], color[n, 3] or None)"""
        dev = self._tsdf_device(on_device)
        kind = MI_ICP_DEVICE if on_device else MI_ICP_HOST
        (t, tp), (w, wp) = self._out(kind, dev, (n,)), self._out(kind, dev, (n,))
        c, cp = self._out(kind, dev, (3, n)) if colored else (None, None)
        self._chk(self._L.mi_icp_tsdf_get_voxels(self._ctx, vol, tp, wp, cp, kind))
        return t, w, (None if c is None else (c.T.contiguous() if on_device else np.ascontiguousarray(c.T)))

    # -- integration::ScalableTSDFVolume (include/mi_icp.h) ---------------------------------------------
    def stsdf_create(self, voxel_length, sdf_trunc, color_type, depth_sampling_stride=4, map_size=1000):
        """-> an opaque volume handle of this engine (mi_icp_stsdf_create)"""
        h = C.c_void_p()
        self._chk(self._L.mi_icp_stsdf_create(self._ctx, float(voxel_length), float(sdf_trunc), int(color_type),
                                              int(depth_sampling_stride), int(map_size), C.byref(h)))
        return h

    def stsdf_destroy(self, vol):
        if getattr(self, "_ctx", None) and vol:
            self._chk(self._L.mi_icp_stsdf_destroy(self._ctx, vol))

    def stsdf_reset(self, vol):
        self._chk(self._L.mi_icp_stsdf_reset(self._ctx, vol))

    def stsdf_num_units(self, vol):
        """-> (open units, unit slots)"""
        n, cap = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.mi_icp_stsdf_num_units(self._ctx, vol, C.byref(n), C.byref(cap)))
        return int(n.value), int(cap.value)

    def stsdf_integrate(self, vol, depth, color, width, height, intrinsic4, extrinsic=None):
        """ScalableTSDFVolume::Integrate; depth / color numpy or torch, both on the same side.  The C ABI of this family
        reads device memory only: host images are uploaded here, and the call waits before they are let go.  A format
        the reference turns away raises MiIcpError."""
        d, col = self._tsdf_frame("ScalableTSDFVolume", depth, color)
        d_dev = d[6]
        if not d_dev:
            dev = torch.device("cuda", self.device)
            d, col = [self._image_desc(None if x[0] is None else torch.from_numpy(x[0]).to(dev)) for x in (d, col)]
            torch.cuda.synchronize(dev)
        (_, dptr, dw, dh, dc, db, _), (_, cptr, cw, ch, cc, cb, _) = d, col
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        _, Eptr = _T_in(extrinsic)
        self._chk(self._L.mi_icp_stsdf_integrate(self._ctx, vol, dptr, dw, dh, dc, db, cptr, cw, ch, cc, cb, int(width),
                                                 int(height), K, Eptr))
        if not d_dev:
            self.synchronize()

    def _stsdf_cloud(self, call, want, on_device):
        """the capacity rule on device arrays; on_device False: the result as numpy arrays"""
        out = self._tsdf_cloud(lambda p, cap, m, kind: call(p, cap, m), want, self.TSDF_FIRST_CAPACITY, self._tsdf_device(True))
        return out if on_device else [None if a is None else a.cpu().numpy() for a in out]

    def stsdf_extract_point_cloud(self, vol, colored, on_device=True):
        """-> (points, normals, colors or None)"""
        return self._stsdf_cloud(lambda p, cap, m: self._L.mi_icp_stsdf_extract_point_cloud(
            self._ctx, vol, p[0], p[1], p[2], cap, m), [True, True, bool(colored)], on_device)

    def stsdf_extract_voxel_point_cloud(self, vol, on_device=True):
        """-> (points, colors)"""
        return self._stsdf_cloud(lambda p, cap, m: self._L.mi_icp_stsdf_extract_voxel_point_cloud(
            self._ctx, vol, p[0], p[1], cap, m), [True, True], on_device)

    def stsdf_get_units(self, vol, colored, on_device=False):
        """-> (keys[m, 3] int32 ascending, tsdf[m, 4096], weight[m, 4096], color[m, 4096, 3] or None)"""
        dev = self._tsdf_device(True)
        n = self.stsdf_num_units(vol)[0]
        (k, kp) = self._out(MI_ICP_DEVICE, dev, (n, 3), np.int32)
        (t, tp), (w, wp) = self._out(MI_ICP_DEVICE, dev, (n, 4096)), self._out(MI_ICP_DEVICE, dev, (n, 4096))
        c, cp = self._out(MI_ICP_DEVICE, dev, (3, n, 4096)) if colored else (None, None)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_stsdf_get_units(self._ctx, vol, kp, tp, wp, cp, n, C.byref(m)))
        assert int(m.value) == n
        if c is not None:
            c = c.permute(1, 2, 0).contiguous()
        out = (k, t, w, c)
        return out if on_device else tuple(None if a is None else a.cpu().numpy() for a in out)

    # -- geometry::OccupancyGrid (include/mi_icp.h; arrays are device tensors, numpy inputs are uploaded) ----------
    @staticmethod
    def occgrid_params(voxel_size, origin, clamping_thres_min, clamping_thres_max, prob_hit_log, prob_miss_log,
                       occ_prob_thres_log):
        p = _lib.OccGridParams()
        p.voxel_size = float(voxel_size)
        p.origin[:] = [float(v) for v in np.asarray(origin, np.float32).reshape(3)]
        p.clamping_thres_min, p.clamping_thres_max = float(clamping_thres_min), float(clamping_thres_max)
        p.prob_hit_log, p.prob_miss_log = float(prob_hit_log), float(prob_miss_log)
        p.occ_prob_thres_log = float(occ_prob_thres_log)
        return p

    def _occ_dev(self, a, dtype):
        """[n, 3] of dtype on this engine's GPU: a tensor there is read in place, anything else is uploaded"""
        tdt = {np.float32: torch.float32, np.int32: torch.int32}[dtype]
        dev = torch.device("cuda", self.device)
        if _is_tensor(a):
            t = a.to(device=dev, dtype=tdt)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)
        return t.reshape(-1, 3).contiguous()

    def occgrid_create(self, resolution):
        """-> an opaque grid handle of this engine (mi_icp_occgrid_create)"""
        h = C.c_void_p()
        self._chk(self._L.mi_icp_occgrid_create(self._ctx, int(resolution), C.byref(h)))
        return h

    def occgrid_destroy(self, grid):
        if getattr(self, "_ctx", None) and grid:
            self._chk(self._L.mi_icp_occgrid_destroy(self._ctx, grid))

    def occgrid_reset(self, grid):
        self._chk(self._L.mi_icp_occgrid_reset(self._ctx, grid))

    def occgrid_reconstruct(self, grid, resolution):
        self._chk(self._L.mi_icp_occgrid_reconstruct(self._ctx, grid, int(resolution)))

    def occgrid_insert(self, grid, params, points, viewpoint, max_range=-1.0):
        t = self._occ_dev(points, np.float32)
        vp = (C.c_float * 3)(*[float(v) for v in np.asarray(viewpoint, np.float32).reshape(3)])
        self._chk(self._L.mi_icp_occgrid_insert(self._ctx, grid, C.byref(params), C.c_void_p(t.data_ptr()), int(t.shape[0]),
                                                vp, float(max_range)))

    def occgrid_add_voxels(self, grid, params, indices, occupied=False):
        t = self._occ_dev(indices, np.int32)
        self._chk(self._L.mi_icp_occgrid_add_voxels(self._ctx, grid, C.byref(params), C.c_void_p(t.data_ptr()),
                                                    int(t.shape[0]), int(bool(occupied))))

    def occgrid_set_free_area(self, grid, params, min_bound, max_bound):
        lo = (C.c_float * 3)(*[float(v) for v in np.asarray(min_bound, np.float32).reshape(3)])
        hi = (C.c_float * 3)(*[float(v) for v in np.asarray(max_bound, np.float32).reshape(3)])
        self._chk(self._L.mi_icp_occgrid_set_free_area(self._ctx, grid, C.byref(params), lo, hi))

    def occgrid_query(self, grid, params, points):
        """-> (log-odds [n], NaN for unknown or outside; voxel index [n, 3] int32), device tensors"""
        t = self._occ_dev(points, np.float32)
        n = int(t.shape[0])
        dev = torch.device("cuda", self.device)
        (prob, pp), (idx, ip) = self._out(MI_ICP_DEVICE, dev, (n,)), self._out(MI_ICP_DEVICE, dev, (n, 3), np.int32)
        self._chk(self._L.mi_icp_occgrid_query(self._ctx, grid, C.byref(params), C.c_void_p(t.data_ptr()), n, pp, ip))
        self.synchronize()   # (t may go)
        return prob, idx

    OCCGRID_FIRST_CAPACITY = 1 << 18   # voxels an extraction makes room for before it knows the count

    def occgrid_extract(self, grid, params, which, want_points=False):
        """-> (grid_index [m, 3] int32, prob_log [m], points [m, 3] or None), device tensors, ascending linear index;
        the capacity rule of include/mi_icp.h"""
        dev = torch.device("cuda", self.device)
        m = C.c_int64(0)
        capacity = self.OCCGRID_FIRST_CAPACITY
        for _ in range(2):
            (idx, ip), (prob, pp) = self._out(MI_ICP_DEVICE, dev, (capacity, 3), np.int32), self._out(MI_ICP_DEVICE, dev, (capacity,))
            xyz, xp = self._out(MI_ICP_DEVICE, dev, (capacity, 3)) if want_points else (None, None)
            self._chk(self._L.mi_icp_occgrid_extract(self._ctx, grid, C.byref(params), int(which), ip, pp, xp, capacity,
                                                     C.byref(m)))
            if int(m.value) <= capacity:
                break
            capacity = int(m.value)
        k = int(m.value)
        return self._trim(idx, k), self._trim(prob, k), self._trim(xyz, k)

    def occgrid_count(self, grid, params, which):
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_occgrid_extract(self._ctx, grid, C.byref(params), int(which), None, None, None, 0, C.byref(m)))
        return int(m.value)

    def occgrid_get_bounds(self, grid):
        """-> (min_bound [3], max_bound [3]) int32 numpy, inclusive voxel indices"""
        lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
        self._chk(self._L.mi_icp_occgrid_get_bounds(self._ctx, grid, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
        return lo, hi

    def occgrid_get_voxels(self, grid, n):
        """-> the whole log-odds plane, [n] on the device"""
        t, tp = self._out(MI_ICP_DEVICE, torch.device("cuda", self.device), (n,))
        self._chk(self._L.mi_icp_occgrid_get_voxels(self._ctx, grid, tp))
        return t

    # -- geometry::DistanceTransform (include/mi_icp.h; arrays are device tensors, numpy inputs are uploaded) -------
    @staticmethod
    def _f3(v):
        return (C.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])

    def dt_create(self, resolution):
        """-> an opaque transform handle of this engine (mi_icp_dt_create)"""
        h = C.c_void_p()
        self._chk(self._L.mi_icp_dt_create(self._ctx, int(resolution), C.byref(h)))
        return h

    def dt_destroy(self, dt):
        if getattr(self, "_ctx", None) and dt:
            self._chk(self._L.mi_icp_dt_destroy(self._ctx, dt))

    def dt_reconstruct(self, dt, resolution):
        self._chk(self._L.mi_icp_dt_reconstruct(self._ctx, dt, int(resolution)))

    def dt_compute_cells(self, dt, cells, want_dropped=False):
        """the sites are the cells [n, 3] int32 inside the grid; -> the number dropped (None unless asked for)"""
        t = self._occ_dev(cells, np.int32)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_dt_compute_cells(self._ctx, dt, C.c_void_p(t.data_ptr()), int(t.shape[0]),
                                                  C.byref(m) if want_dropped else None))
        if not want_dropped:
            self.synchronize()   # (t may go)
        return int(m.value) if want_dropped else None

    def dt_compute_voxelgrid(self, dt, voxel_size, origin, keys, grid_voxel_size, grid_origin, want_dropped=False):
        t = self._occ_dev(keys, np.int32)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_dt_compute_voxelgrid(self._ctx, dt, float(voxel_size), self._f3(origin),
                                                      C.c_void_p(t.data_ptr()), int(t.shape[0]), float(grid_voxel_size),
                                                      self._f3(grid_origin), C.byref(m) if want_dropped else None))
        if not want_dropped:
            self.synchronize()   # (t may go)
        return int(m.value) if want_dropped else None

    def dt_compute_occgrid(self, dt, grid, occ_prob_thres_log):
        self._chk(self._L.mi_icp_dt_compute_occgrid(self._ctx, dt, grid, float(occ_prob_thres_log)))

    def dt_query(self, dt, voxel_size, origin, points):
        """-> (distance [n], NaN outside the grid; nearest site [n, 3] int32, -1 without one), device tensors"""
        t = self._occ_dev(points, np.float32)
        n = int(t.shape[0])
        dev = torch.device("cuda", self.device)
        (dist, dp), (idx, ip) = self._out(MI_ICP_DEVICE, dev, (n,)), self._out(MI_ICP_DEVICE, dev, (n, 3), np.int32)
        self._chk(self._L.mi_icp_dt_query(self._ctx, dt, float(voxel_size), self._f3(origin), C.c_void_p(t.data_ptr()), n, dp, ip))
        self.synchronize()   # (t may go)
        return dist, idx

    def dt_get_voxels(self, dt, voxel_size, n, want_nearest=True, want_distance=True):
        """-> the whole plane: (nearest site [n, 3] int32 or None, distance [n] or None) on the device"""
        dev = torch.device("cuda", self.device)
        idx, ip = self._out(MI_ICP_DEVICE, dev, (n, 3), np.int32) if want_nearest else (None, None)
        dist, dp = self._out(MI_ICP_DEVICE, dev, (n,)) if want_distance else (None, None)
        self._chk(self._L.mi_icp_dt_get_voxels(self._ctx, dt, float(voxel_size), ip, dp))
        return idx, dist

    # -- geometry::VoxelGrid (include/mi_icp.h; keys int32 [m, 3] and colours [m, 3] are device tensors) -----------
    VOXELGRID_AVERAGE, VOXELGRID_KEEP_FIRST = 0, 1

    def _vg_dev(self, a, dtype, cols=3):
        """[n, cols] of dtype on this engine's GPU (None stays None): a tensor there is read in place"""
        if a is None:
            return None
        tdt = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        dev = torch.device("cuda", self.device)
        if _is_tensor(a):
            t = a.to(device=dev, dtype=tdt)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(dev)
        return (t.reshape(-1, cols) if cols > 1 else t.reshape(-1)).contiguous()

    @staticmethod
    def _ptr(t):
        return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())

    @staticmethod
    def _f3(v):
        return (C.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])

    def _vg_counted(self, first_capacity, call):
        """the capacity rule: call(keys_ptr, colors_ptr, capacity, byref(m)) once for the count, again with room"""
        dev = torch.device("cuda", self.device)
        m = C.c_int64(0)
        capacity = max(int(first_capacity), 1)
        for _ in range(2):
            (keys, kp), (cols, cp) = self._out(MI_ICP_DEVICE, dev, (capacity, 3), np.int32), self._out(MI_ICP_DEVICE, dev, (capacity, 3))
            self._chk(call(kp, cp, capacity, C.byref(m)))
            if int(m.value) <= capacity:
                break
            capacity = int(m.value)
        self.synchronize()   # (uploaded inputs may go)
        k = int(m.value)
        return keys[:k], cols[:k]

    def voxelgrid_from_points(self, points, voxel_size, min_bound, max_bound, colors=None):
        """-> (keys [m, 3] int32 ascending, colors [m, 3]) (mi_icp_voxelgrid_from_points)"""
        p, c = self._vg_dev(points, np.float32), self._vg_dev(colors, np.float32)
        n = int(p.shape[0])
        if c is not None and int(c.shape[0]) != n:
            raise MiIcpError("voxelgrid_from_points: %d colours for %d points" % (int(c.shape[0]), n))
        lo, hi = self._f3(min_bound), self._f3(max_bound)
        return self._vg_counted(n, lambda kp, cp, cap, m: self._L.mi_icp_voxelgrid_from_points(
            self._ctx, self._ptr(p), self._ptr(c), n, float(voxel_size), lo, hi, kp, cp, cap, m))

    def voxelgrid_dense(self, num_w, num_h, num_d):
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_voxelgrid_dense(self._ctx, int(num_w), int(num_h), int(num_d), None, None, 0, C.byref(m)))
        return self._vg_counted(int(m.value), lambda kp, cp, cap, mm: self._L.mi_icp_voxelgrid_dense(
            self._ctx, int(num_w), int(num_h), int(num_d), kp, cp, cap, mm))

    def voxelgrid_merge(self, keys_a, colors_a, keys_b, colors_b, mode):
        ka, ca = self._vg_dev(keys_a, np.int32), self._vg_dev(colors_a, np.float32)
        kb, cb = self._vg_dev(keys_b, np.int32), self._vg_dev(colors_b, np.float32)
        ma, mb = int(ka.shape[0]), int(kb.shape[0])
        if int(ca.shape[0]) != ma or int(cb.shape[0]) != mb:
            raise MiIcpError("voxelgrid_merge: keys and colours differ in length")
        return self._vg_counted(ma + mb, lambda kp, cp, cap, m: self._L.mi_icp_voxelgrid_merge(
            self._ctx, self._ptr(ka), self._ptr(ca), ma, self._ptr(kb), self._ptr(cb), mb, int(mode), kp, cp, cap, m))

    def voxelgrid_carve(self, keys, colors, voxel_size, origin, image, intrinsic4, extrinsic=None,
                        keep_voxels_outside_image=False):
        """-> the (keys, colors) that stay, order kept (mi_icp_voxelgrid_carve); image: [H, W] or [H, W, C], any dtype"""
        k, c = self._vg_dev(keys, np.int32), self._vg_dev(colors, np.float32)
        m = int(k.shape[0])
        dev = torch.device("cuda", self.device)
        if _is_tensor(image):
            img = image.to(dev).contiguous()
        else:
            a = np.ascontiguousarray(image)
            if a.dtype == np.uint16:    # (torch has no arithmetic on uint16; the bytes are all that travel)
                a = a.view(np.int16)
            img = torch.from_numpy(a).to(dev)
        height, width = int(img.shape[0]), int(img.shape[1])
        channels = int(img.shape[2]) if img.dim() == 3 else 1
        intr = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        E, Ep = _T_in(extrinsic)
        (ok, okp), (oc, ocp) = self._out(MI_ICP_DEVICE, dev, (max(m, 1), 3), np.int32), self._out(MI_ICP_DEVICE, dev, (max(m, 1), 3))
        mo = C.c_int64(0)
        self._chk(self._L.mi_icp_voxelgrid_carve(self._ctx, self._ptr(k), self._ptr(c), m, float(voxel_size), self._f3(origin),
                                                 self._ptr(img), width, height, channels, int(img.element_size()), intr, Ep,
                                                 int(bool(keep_voxels_outside_image)), okp, ocp, C.byref(mo)))
        return ok[:int(mo.value)], oc[:int(mo.value)]

    def voxelgrid_query(self, keys, voxel_size, origin, queries, keys_sorted=False):
        """-> (included [nq] uint8, index [nq, 3] int32), device tensors (mi_icp_voxelgrid_query)"""
        k, q = self._vg_dev(keys, np.int32), self._vg_dev(queries, np.float32)
        m, nq = int(k.shape[0]), int(q.shape[0])
        dev = torch.device("cuda", self.device)
        (inc, ip), (idx, xp) = self._out(MI_ICP_DEVICE, dev, (nq,), np.uint8), self._out(MI_ICP_DEVICE, dev, (nq, 3), np.int32)
        self._chk(self._L.mi_icp_voxelgrid_query(self._ctx, self._ptr(k), m, int(bool(keys_sorted)), float(voxel_size),
                                                 self._f3(origin), self._ptr(q), nq, ip, xp))
        self.synchronize()   # (q may go)
        return inc, idx

    def voxelgrid_bounds(self, keys, voxel_size, origin):
        """-> (min_index [3] int32, max_index [3] int32, centre_sum [3] float64), numpy; the grid must not be empty"""
        k = self._vg_dev(keys, np.int32)
        lo, hi, s = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.float64)
        self._chk(self._L.mi_icp_voxelgrid_bounds(self._ctx, self._ptr(k), int(k.shape[0]), float(voxel_size), self._f3(origin),
                                                  lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p),
                                                  s.ctypes.data_as(C.c_void_p)))
        return lo, hi, s

    def voxelgrid_select_by_index(self, keys, colors, indices, invert=False):
        k, c = self._vg_dev(keys, np.int32), self._vg_dev(colors, np.float32)
        idx = self._vg_dev(indices, np.int64, 1)
        m, ni = int(k.shape[0]), int(idx.shape[0])
        rows = max(m if invert else ni, 1)
        dev = torch.device("cuda", self.device)
        (ok, okp), (oc, ocp) = self._out(MI_ICP_DEVICE, dev, (rows, 3), np.int32), self._out(MI_ICP_DEVICE, dev, (rows, 3))
        mo = C.c_int64(0)
        self._chk(self._L.mi_icp_voxelgrid_select_by_index(self._ctx, self._ptr(k), self._ptr(c), m, self._ptr(idx), ni,
                                                           int(bool(invert)), okp, ocp, C.byref(mo)))
        return ok[:int(mo.value)], oc[:int(mo.value)]

    def voxelgrid_paint(self, colors, color, indices=None):
        """paints the device tensor `colors` [m, 3] in place: every row, or the rows listed"""
        idx = None if indices is None else self._vg_dev(indices, np.int64, 1)
        ni = 0 if idx is None else int(idx.shape[0])
        if idx is not None and ni == 0:
            return
        self._chk(self._L.mi_icp_voxelgrid_paint(self._ctx, self._ptr(colors), int(colors.shape[0]), self._ptr(idx), ni,
                                                 self._f3(color)))
        self.synchronize()   # (idx may go)

    # -- collision (include/mi_icp.h; a side is built by one of the four makers below and keeps its tensors alive) ----
    def collision_voxel_side(self, keys, voxel_size, origin, keys_sorted=False):
        s = _lib.CollisionSide()
        k = self._vg_dev(keys, np.int32)
        s.kind, s.keys_sorted, s.m = _lib.COLLISION_VOXELGRID, int(bool(keys_sorted)), int(k.shape[0])
        s.keys = k.data_ptr() if s.m else None
        s.voxel_size = float(voxel_size)
        s.origin[:] = [float(v) for v in np.asarray(origin, np.float32).reshape(3)]
        return s, (k,)

    @staticmethod
    def collision_occgrid_side(grid, params):
        s = _lib.CollisionSide()
        s.kind, s.grid_params = _lib.COLLISION_OCCGRID, params
        s.grid = grid.value if isinstance(grid, C.c_void_p) else grid
        return s, (grid, params)

    def collision_lineset_side(self, points, lines):
        s = _lib.CollisionSide()
        p, l = self._vg_dev(points, np.float32), self._vg_dev(lines, np.int32, 2)
        s.kind, s.n_points, s.n_lines = _lib.COLLISION_LINESET, int(p.shape[0]), int(l.shape[0])
        s.points = p.data_ptr() if s.n_points else None
        s.lines = l.data_ptr() if s.n_lines else None
        return s, (p, l)

    def collision_primitives_side(self, records):
        """records: numpy structured array / bytes of 80-byte mi_icp_primitive records"""
        s = _lib.CollisionSide()
        raw = np.ascontiguousarray(np.frombuffer(np.ascontiguousarray(records).tobytes(), np.uint8))
        n = raw.size // C.sizeof(_lib.Primitive)
        t = torch.from_numpy(raw.copy()).to(torch.device("cuda", self.device))
        s.kind, s.n_primitives = _lib.COLLISION_PRIMITIVES, n
        s.primitives = t.data_ptr() if n else None
        return s, (t,)

    def collision_compute(self, side_a, side_b, margin=0.0, first_capacity=None):
        """-> pairs [m, 2] int32 on the device (mi_icp_collision_compute); the capacity rule of include/mi_icp.h"""
        (a, keep_a), (b, keep_b) = side_a, side_b
        dev = torch.device("cuda", self.device)
        m = C.c_int64(0)
        capacity = max(int(first_capacity if first_capacity is not None else 1 << 16), 1)
        for _ in range(2):
            pairs, pp = self._out(MI_ICP_DEVICE, dev, (capacity, 2), np.int32)
            self._chk(self._L.mi_icp_collision_compute(self._ctx, C.byref(a), C.byref(b), float(margin), pp, capacity, C.byref(m)))
            if int(m.value) <= capacity:
                break
            capacity = int(m.value)
        self.synchronize()   # (uploaded inputs may go)
        del keep_a, keep_b
        return pairs[:int(m.value)]

    def collision_voxelize_primitive(self, record, voxel_size):
        """-> (keys [m, 3] int32 ascending, colors [m, 3], origin [3] numpy) (mi_icp_collision_voxelize_primitive)"""
        P = _lib.Primitive.from_buffer_copy(np.ascontiguousarray(record).tobytes())
        origin = (C.c_float * 3)()
        keys, cols = self._vg_counted(1 << 16, lambda kp, cp, cap, m: self._L.mi_icp_collision_voxelize_primitive(
            self._ctx, C.byref(P), float(voxel_size), kp, cp, cap, m, origin))
        return keys, cols, np.array(list(origin), np.float32)

    @staticmethod
    def primitive_aabb(record):
        P = _lib.Primitive.from_buffer_copy(np.ascontiguousarray(record).tobytes())
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        _lib.load().mi_icp_primitive_aabb(C.byref(P), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p))
        return lo, hi

    # -- graph (include/mi_icp.h "graph"; every array a device tensor of this engine's GPU) ----------------------------
    def graph_construct(self, lines, n_points, weights=None, colors=None):
        """sorts lines [m, 2] (and weights [m], colors [m, 3] with them) IN PLACE, stably -> offsets [n_points + 1]"""
        dev = torch.device("cuda", self.device)
        off, op = self._out(MI_ICP_DEVICE, dev, (int(n_points) + 1,), np.int32)
        self._chk(self._L.mi_icp_graph_construct(self._ctx, self._ptr(lines), self._ptr(weights), self._ptr(colors),
                                                 int(lines.shape[0]), int(n_points), op))
        return off

    def graph_weights_from_distance(self, points, lines):
        dev = torch.device("cuda", self.device)
        m = int(lines.shape[0])
        w, wp = self._out(MI_ICP_DEVICE, dev, (m,), np.float32)
        self._chk(self._L.mi_icp_graph_weights_from_distance(self._ctx, self._ptr(points), int(points.shape[0]),
                                                             self._ptr(lines), m, wp))
        return w

    def graph_node_distances(self, points, point):
        dev = torch.device("cuda", self.device)
        d, dp = self._out(MI_ICP_DEVICE, dev, (int(points.shape[0]),), np.float32)
        self._chk(self._L.mi_icp_graph_node_distances(self._ctx, self._ptr(points), int(points.shape[0]), self._f3(point), dp))
        return d

    def graph_lattice(self, min_bound, max_bound, resolutions):
        """-> (points [n, 3], lines [m, 2], weights [m], offsets [n + 1]) (mi_icp_graph_lattice)"""
        dev = torch.device("cuda", self.device)
        lo, hi = self._f3(min_bound), self._f3(max_bound)
        res = (C.c_int32 * 3)(*[int(v) for v in np.asarray(resolutions).reshape(3)])
        n, m = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.mi_icp_graph_lattice(self._ctx, lo, hi, res, None, 0, None, None, 0, None, C.byref(n), C.byref(m)))
        nn, mm = int(n.value), int(m.value)
        (p, pp), (l, lp) = self._out(MI_ICP_DEVICE, dev, (nn, 3)), self._out(MI_ICP_DEVICE, dev, (max(mm, 1), 2), np.int32)
        (w, wp), (o, op) = self._out(MI_ICP_DEVICE, dev, (max(mm, 1),)), self._out(MI_ICP_DEVICE, dev, (nn + 1,), np.int32)
        self._chk(self._L.mi_icp_graph_lattice(self._ctx, lo, hi, res, pp, nn, lp, wp, mm, op, C.byref(n), C.byref(m)))
        return p, l[:mm], w[:mm], o

    def graph_set_edge_weights(self, lines, weights, edges, weight, is_directed):
        """weights [m] changed in place; lines sorted (graph_construct)"""
        self._chk(self._L.mi_icp_graph_set_edge_weights(self._ctx, self._ptr(lines), self._ptr(weights), int(lines.shape[0]),
                                                        self._ptr(edges), int(edges.shape[0]), int(bool(is_directed)),
                                                        float(weight)))

    def graph_remove_edges(self, lines, n_points, edges, is_directed, weights=None, colors=None):
        """compacts lines / weights / colors in place -> (the number of lines that stay, offsets)"""
        dev = torch.device("cuda", self.device)
        off, op = self._out(MI_ICP_DEVICE, dev, (int(n_points) + 1,), np.int32)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_graph_remove_edges(self._ctx, self._ptr(lines), self._ptr(weights), self._ptr(colors),
                                                    int(lines.shape[0]), int(n_points), self._ptr(edges), int(edges.shape[0]),
                                                    int(bool(is_directed)), op, C.byref(m)))
        return int(m.value), off

    def graph_sssp(self, offsets, lines, weights, n, start, end=-1, want_info=False):
        """-> (dist [n] float32, prev [n] int32) on the device (mi_icp_graph_sssp); with want_info also the five words
        (regime, launches, host waits, rounds, tier-2 rounds)"""
        dev = torch.device("cuda", self.device)
        (d, dp), (p, pp) = self._out(MI_ICP_DEVICE, dev, (int(n),)), self._out(MI_ICP_DEVICE, dev, (int(n),), np.int32)
        info = (C.c_int32 * 5)()
        self._chk(self._L.mi_icp_graph_sssp(self._ctx, self._ptr(offsets), self._ptr(lines), self._ptr(weights), int(n),
                                            int(lines.shape[0]), int(start), int(end), dp, pp, info))
        return (d, p, [int(v) for v in info]) if want_info else (d, p)

    @staticmethod
    def graph_sssp_limits():
        """-> (the small regime's largest n, its largest m, the rounds of a batch in the large regime)"""
        n, m, b = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _lib.load().mi_icp_graph_sssp_limits(C.byref(n), C.byref(m), C.byref(b))
        return int(n.value), int(m.value), int(b.value)

    # -- laserscan (include/mi_icp.h "laserscan"; ranges / intensities / points device tensors, origins host) --------
    def laserscan_to_points(self, ranges, intensities, origins, num_steps, num_max_scans, first_slot, num_scans,
                            min_angle, max_angle, min_range, max_range, capacity=None):
        """-> (points [m, 3], colours [m, 3] or None, m) on the device.  origins: [num_max_scans, 4, 4] row-major numpy.
        capacity=None asks for the count first and then makes room; a given capacity is passed as it is (too little
        room: empty arrays and the count)."""
        dev = torch.device("cuda", self.device)
        O = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        m = C.c_int64(0)

        def call(cap):
            (p, pp) = self._out(MI_ICP_DEVICE, dev, (max(cap, 1), 3))
            (c, cp) = self._out(MI_ICP_DEVICE, dev, (max(cap, 1), 3)) if intensities is not None else (None, None)
            self._chk(self._L.mi_icp_laserscan_to_points(
                self._ctx, self._ptr(ranges), self._ptr(intensities), O.ctypes.data_as(C.c_void_p), int(num_steps),
                int(num_max_scans), int(first_slot), int(num_scans), float(min_angle), float(max_angle), float(min_range),
                float(max_range), pp if cap > 0 else None, cp if cap > 0 else None, int(cap), C.byref(m)))
            return p, c
        if capacity is None:
            p, c = call(int(num_scans) * int(num_steps))
        else:
            p, c = call(int(capacity))
            if int(m.value) > int(capacity):
                return p[:0], (None if c is None else c[:0]), int(m.value)
        k = int(m.value)
        return p[:k], (None if c is None else c[:k]), k

    def _laserscan_bins(self, angle_increment, min_angle, max_angle):
        q = np.ceil((np.float32(max_angle) - np.float32(min_angle)) / np.float32(angle_increment))
        return int(q) if np.isfinite(q) and 0 < q < 2 ** 31 else 0

    def laserscan_from_points(self, points, angle_increment, min_height, max_height, num_vertical_divisions=1,
                              min_range=0.0, max_range=float("inf"), min_angle=-np.pi, max_angle=np.pi):
        """-> (ranges [num_vertical_divisions, num_steps] on the device, the path: 0 LDS, 1 global)"""
        dev = torch.device("cuda", self.device)
        with np.errstate(all="ignore"):
            steps = self._laserscan_bins(angle_increment, min_angle, max_angle)
        div = int(num_vertical_divisions)
        room = steps * div if 0 < steps * max(div, 0) <= self.laserscan_limits()[1] else 1
        out, op = self._out(MI_ICP_DEVICE, dev, (room,))
        info = C.c_int32(-1)
        self._chk(self._L.mi_icp_laserscan_from_points(
            self._ctx, self._ptr(points), int(points.shape[0]), float(angle_increment), float(min_height), float(max_height),
            div, float(min_range), float(max_range), float(min_angle), float(max_angle), steps, op, C.byref(info)))
        return out.reshape(div, steps), int(info.value)

    def laserscan_from_depth(self, depth, intrinsic4, angle_increment, min_y, max_y, num_vertical_divisions=1, min_range=0.0,
                             max_range=float("inf"), min_angle=-np.pi, max_angle=np.pi, depth_scale=1000.0,
                             depth_trunc=1000.0, stride=1):
        """depth: [H, W] float32 or uint16 device tensor -> (ranges [num_vertical_divisions, num_steps], the path)"""
        dev = torch.device("cuda", self.device)
        name = str(depth.dtype).replace("torch.", "")
        if depth.ndim != 2 or name not in ("float32", "uint16"):
            raise TypeError("depth must be [H, W] float32 or uint16")
        d = depth.contiguous()
        with np.errstate(all="ignore"):
            steps = self._laserscan_bins(angle_increment, min_angle, max_angle)
        div = int(num_vertical_divisions)
        room = steps * div if 0 < steps * max(div, 0) <= self.laserscan_limits()[1] else 1
        out, op = self._out(MI_ICP_DEVICE, dev, (room,))
        info = C.c_int32(-1)
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        self._chk(self._L.mi_icp_laserscan_from_depth(
            self._ctx, C.c_void_p(d.data_ptr()), 1 if name == "uint16" else 0, int(d.shape[1]), int(d.shape[0]), K,
            float(depth_scale), float(depth_trunc), int(stride), float(angle_increment), float(min_y), float(max_y), div,
            float(min_range), float(max_range), float(min_angle), float(max_angle), steps, op, C.byref(info)))
        return out.reshape(div, steps), int(info.value)

    def laserscan_range_filter(self, ranges, min_range, max_range):
        out = torch.empty_like(ranges)
        self._chk(self._L.mi_icp_laserscan_range_filter(self._ctx, self._ptr(ranges), int(ranges.numel()), float(min_range),
                                                        float(max_range), self._ptr(out)))
        return out

    def laserscan_shadow_filter(self, ranges, num_steps, scan_min_angle, scan_max_angle, min_angle, max_angle, window,
                                neighbors=0, remove_shadow_start_point=False):
        """ranges: [rows, num_steps] -> the filtered copy"""
        out = torch.empty_like(ranges)
        self._chk(self._L.mi_icp_laserscan_shadow_filter(
            self._ctx, self._ptr(ranges), int(num_steps), int(ranges.numel() // max(int(num_steps), 1)), float(scan_min_angle),
            float(scan_max_angle), float(min_angle), float(max_angle), int(window), int(neighbors),
            int(bool(remove_shadow_start_point)), self._ptr(out)))
        return out

    def laserscan_scale(self, ranges, scale):
        self._chk(self._L.mi_icp_laserscan_scale(self._ctx, self._ptr(ranges), int(ranges.numel()), float(scale)))

    @staticmethod
    def laserscan_limits():
        """-> (the LDS path's largest bin count, the largest bin count taken at all)"""
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.load().mi_icp_laserscan_limits(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # -- image (include/mi_icp.h "image"; pixels are contiguous device tensors [H, W] or [H, W, C], taps and the table host) --
    @staticmethod
    def _image_dims(t):
        """-> (height, width, channels, bytes per channel) of a device tensor [H, W] or [H, W, C]"""
        if t.dim() not in (2, 3) or not t.is_cuda or not t.is_contiguous():
            raise TypeError("an image is a contiguous device tensor [H, W] or [H, W, C]")
        return int(t.shape[0]), int(t.shape[1]), (int(t.shape[2]) if t.dim() == 3 else 1), int(t.element_size())

    @staticmethod
    def _taps(k):
        k = np.ascontiguousarray(np.asarray(k, np.float32).reshape(-1))
        return k, k.ctypes.data_as(C.c_void_p), int(k.size)

    def image_filter(self, src, dx, dy=None):
        """Image::Filter(dx, dy), or Image::FilterHorizontal(dx) with dy None; src [H, W] float32 -> the filtered copy"""
        h, w, ch, b = self._image_dims(src)
        if (ch, b) != (1, 4) or src.dim() != 2:
            raise TypeError("image_filter takes a 1 x float32 image")
        out = torch.empty_like(src)
        kx, px, nx = self._taps(dx)
        ky, py, ny = self._taps(dy) if dy is not None else (None, None, 0)
        self._chk(self._L.mi_icp_image_filter(self._ctx, self._ptr(src), w, h, px, nx, py, ny, self._ptr(out)))
        return out

    def image_downsample(self, src):
        """Image::Downsample: [H, W] float32 or [H, W, 3] uint8 -> [H // 2, W // 2(, 3)]"""
        h, w, ch, b = self._image_dims(src)
        out = torch.empty((h // 2, w // 2) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
        self._chk(self._L.mi_icp_image_downsample(self._ctx, self._ptr(src), w, h, ch, b, self._ptr(out)))
        return out

    def image_pyramid_level(self, src):
        """Downsample(Filter(Gaussian3)) of [H, W] float32 in one kernel"""
        h, w, ch, b = self._image_dims(src)
        if (ch, b) != (1, 4) or src.dim() != 2:
            raise TypeError("image_pyramid_level takes a 1 x float32 image")
        out = torch.empty((h // 2, w // 2), dtype=src.dtype, device=src.device)
        self._chk(self._L.mi_icp_image_pyramid_level(self._ctx, self._ptr(src), w, h, self._ptr(out)))
        return out

    @staticmethod
    def image_bilateral_table(diameter, sigma_space):
        """the spatial table of Image::BilateralFilter, 2 * diameter + 1 floats (host arithmetic)"""
        t = np.zeros(2 * max(int(diameter), 0) + 1, np.float32)
        if _lib.load().mi_icp_image_bilateral_table(int(diameter), float(sigma_space), t.ctypes.data_as(C.c_void_p)) < 0:
            raise MiIcpError("image_bilateral_table: diameter must be in [0, %d]" % Engine.image_limits()[1])
        return t

    def image_bilateral(self, src, diameter, sigma_color, sigma_space, exp_kind=None):
        """Image::BilateralFilter of [H, W] float32.  exp_kind (measurements and tests only): 1 the hardware
        exponential, which is what runs by default, 0 expf."""
        h, w, ch, b = self._image_dims(src)
        if (ch, b) != (1, 4) or src.dim() != 2:
            raise TypeError("image_bilateral takes a 1 x float32 image")
        t = self.image_bilateral_table(diameter, sigma_space)
        out = torch.empty_like(src)
        args = (self._ctx, self._ptr(src), w, h, int(diameter), float(sigma_color), t.ctypes.data_as(C.c_void_p), self._ptr(out))
        if exp_kind is None:
            self._chk(self._L.mi_icp_image_bilateral(*args))
        else:
            self._chk(self._L.mi_icp_debug_image_bilateral(*(args + (int(exp_kind),))))
        return out

    def image_create_float(self, src, type=1):
        """Image::CreateFloatImage -> [H, W] float32"""
        h, w, ch, b = self._image_dims(src)
        out = torch.empty((h, w), dtype=torch.float32, device=src.device)
        self._chk(self._L.mi_icp_image_create_float(self._ctx, self._ptr(src), w, h, ch, b, int(type), self._ptr(out)))
        return out

    def image_depth_to_float(self, src, depth_scale=1000.0, depth_trunc=3.0):
        """Image::ConvertDepthToFloatImage -> [H, W] float32"""
        h, w, ch, b = self._image_dims(src)
        out = torch.empty((h, w), dtype=torch.float32, device=src.device)
        self._chk(self._L.mi_icp_image_depth_to_float(self._ctx, self._ptr(src), w, h, ch, b, float(depth_scale),
                                                      float(depth_trunc), self._ptr(out)))
        return out

    def image_create_gray(self, src, type=1):
        """Image::CreateGrayImage -> [H, W] uint8"""
        h, w, ch, b = self._image_dims(src)
        out = torch.empty((h, w), dtype=torch.uint8, device=src.device)
        self._chk(self._L.mi_icp_image_create_gray(self._ctx, self._ptr(src), w, h, ch, b, int(type), self._ptr(out)))
        return out

    def image_from_float(self, src, bytes_per_channel):
        """Image::CreateImageFromFloatImage<uint8_t | uint16_t>: [H, W] float32 -> [H, W] uint8 (1) or uint16 (2)"""
        h, w, ch, b = self._image_dims(src)
        if (ch, b) != (1, 4) or src.dim() != 2:
            raise TypeError("image_from_float takes a 1 x float32 image")
        if int(bytes_per_channel) not in (1, 2):
            raise ValueError("bytes_per_channel must be 1 or 2")
        out = torch.empty((h, w), dtype=torch.uint8 if int(bytes_per_channel) == 1 else torch.uint16, device=src.device)
        self._chk(self._L.mi_icp_image_from_float(self._ctx, self._ptr(src), w, h, int(bytes_per_channel), self._ptr(out)))
        return out

    def image_linear_transform(self, data, scale=1.0, offset=0.0):
        """Image::LinearTransform in place ([H, W] float32 or uint8 of any channel count)"""
        h, w, ch, b = self._image_dims(data)
        self._chk(self._L.mi_icp_image_linear_transform(self._ctx, self._ptr(data), w, h, ch, b, float(scale), float(offset)))

    def image_clip(self, data, min=0.0, max=1.0):
        """Image::ClipIntensity in place ([H, W] float32)"""
        h, w, ch, b = self._image_dims(data)
        if (ch, b) != (1, 4):
            raise TypeError("image_clip takes a 1 x float32 image")
        self._chk(self._L.mi_icp_image_clip(self._ctx, self._ptr(data), w, h, float(min), float(max)))

    def image_move(self, src, op):
        """op 0 Image::Transpose, 1 FlipVertical, 2 FlipHorizontal -> the moved copy"""
        h, w, ch, b = self._image_dims(src)
        shape = ((w, h) if int(op) == 0 else (h, w)) + tuple(src.shape[2:])
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
        self._chk(self._L.mi_icp_image_move(self._ctx, self._ptr(src), w, h, ch * b, int(op), self._ptr(out)))
        return out

    def image_depth_format(self, src, format):
        """format 0 SUN, 1 NYU: [H, W] uint16 -> the decoded copy"""
        h, w, ch, b = self._image_dims(src)
        if (ch, b) != (1, 2):
            raise TypeError("image_depth_format takes a 1 x uint16 image")
        out = torch.empty_like(src)
        self._chk(self._L.mi_icp_image_depth_format(self._ctx, self._ptr(src), w, h, int(format), self._ptr(out)))
        return out

    @staticmethod
    def image_limits():
        """-> (the longest filter, the largest bilateral radius)"""
        a, b = C.c_int32(0), C.c_int32(0)
        _lib.load().mi_icp_image_limits(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # -- stereo (include/mi_icp.h "stereo"; images are contiguous device tensors) ---------------------------
    def sgm_create(self, width, height, p1=10, p2=120, uniqueness=0.95, disp_size=128, path_type=1, min_disp=0,
                   lr_max_diff=1):
        """-> an opaque matcher handle of this engine (mi_icp_sgm_create); invalid options raise MiIcpError (code -1)"""
        h = C.c_void_p()
        self._chk(self._L.mi_icp_sgm_create(self._ctx, int(width), int(height), int(p1), int(p2), float(uniqueness),
                                            int(disp_size), int(path_type), int(min_disp), int(lr_max_diff), C.byref(h)))
        return h

    def sgm_destroy(self, matcher):
        if getattr(self, "_ctx", None) and matcher:
            self._chk(self._L.mi_icp_sgm_destroy(self._ctx, matcher))

    def _gray8(self, t, what):
        h, w, ch, b = self._image_dims(t)
        if (ch, b) != (1, 1) or t.dim() != 2:
            raise TypeError("%s takes a 1 x uint8 image" % what)
        return h, w

    def sgm_process(self, matcher, left, right):
        """SemiGlobalMatching::ProcessFrame: two [H, W] uint8 images of the matcher's size -> the disparity image"""
        self._gray8(left, "sgm_process")
        self._gray8(right, "sgm_process")
        out = torch.empty_like(left)
        self._chk(self._L.mi_icp_sgm_process(self._ctx, matcher, self._ptr(left), self._ptr(right), self._ptr(out)))
        return out

    def sgm_census(self, src):
        """[H, W] uint8 -> the census words, [H, W] int32 holding the unsigned words' bits"""
        h, w = self._gray8(src, "sgm_census")
        out = torch.empty((h, w), dtype=torch.int32, device=src.device)
        self._chk(self._L.mi_icp_sgm_census(self._ctx, self._ptr(src), w, h, self._ptr(out)))
        return out

    def sgm_get_sums(self, matcher, width, height, disp_size):
        """S of the matcher's last frame -> [H, W, D] uint16"""
        out = torch.empty((int(height), int(width), int(disp_size)), dtype=torch.uint16, device=torch.device("cuda", self.device))
        self._chk(self._L.mi_icp_sgm_get_sums(self._ctx, matcher, self._ptr(out)))
        return out

    @staticmethod
    def sgm_limits():
        """-> (the largest image side, the largest p2)"""
        a, b = C.c_int32(0), C.c_int32(0)
        _lib.load().mi_icp_sgm_limits(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def create_from_disparity(self, disp, color, q):
        """PointCloud::CreateFromDisparity: disp [H, W] uint8, color [H, W, 3] uint8 or uint16 (device tensors), q the
        seven float32 of include/mi_icp.h -> (points [H * W, 3], colors [H * W, 3]) device tensors"""
        h, w = self._gray8(disp, "create_from_disparity")
        ch, cw, cc, cb = self._image_dims(color)
        if (ch, cw, cc) != (h, w, 3) or cb not in (1, 2):
            raise TypeError("create_from_disparity takes a colour image of the disparity's size, 3 x uint8 or 3 x uint16")
        q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(7))
        pts = torch.empty((h * w, 3), dtype=torch.float32, device=disp.device)
        col = torch.empty((h * w, 3), dtype=torch.float32, device=disp.device)
        self._chk(self._L.mi_icp_create_from_disparity(self._ctx, self._ptr(disp), self._ptr(color), w, h, cb,
                                                       q.ctypes.data_as(C.c_void_p), self._ptr(pts), self._ptr(col)))
        return pts, col

    # -- feature matching and FastGlobalRegistration (include/mi_icp.h; every array becomes a device tensor) ----------
    @staticmethod
    def fgr_option(division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                   iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        return _lib.FgrOption(float(division_factor), int(bool(use_absolute_scale)), int(bool(decrease_mu)),
                              float(maximum_correspondence_distance), int(iteration_number), float(tuple_scale),
                              int(maximum_tuple_count))

    def _features(self, a, what):
        if not _is_tensor(a):
            a = np.asarray(a, np.float32)
        if a.ndim != 2:
            raise TypeError("%s takes features as [n, dim]" % what)
        dim = int(a.shape[1])
        return self._vg_dev(a, np.float32, max(dim, 1)), int(a.shape[0]), dim

    def feature_match(self, query, ref):
        """mi_icp_feature_match -> (q_idx int32 [nq], q_d [nq], r_idx int32 [nr], r_d [nr]) device tensors"""
        q, nq, dim = self._features(query, "feature_match")
        r, nr, rdim = self._features(ref, "feature_match")
        if dim != rdim:
            raise MiIcpError("feature_match: dimensions %d and %d differ" % (dim, rdim))
        dev = torch.device("cuda", self.device)
        (qi, qip), (qd, qdp) = self._out(MI_ICP_DEVICE, dev, (nq,), np.int32), self._out(MI_ICP_DEVICE, dev, (nq,))
        (ri, rip), (rd, rdp) = self._out(MI_ICP_DEVICE, dev, (nr,), np.int32), self._out(MI_ICP_DEVICE, dev, (nr,))
        self._chk(self._L.mi_icp_feature_match(self._ctx, self._ptr(q), nq, self._ptr(r), nr, dim, qip, qdp, rip, rdp))
        self.synchronize()   # (uploaded inputs may go)
        return qi, qd, ri, rd

    def fgr_correspondences(self, s_idx, t_idx, source, target, tuple_scale=0.95, maximum_tuple_count=1000, seed=0):
        """mi_icp_fgr_correspondences -> (pairs int32 [ncorr, 2], corr int32 [m, 2]) device tensors"""
        si, ti = self._vg_dev(s_idx, np.int32, 1), self._vg_dev(t_idx, np.int32, 1)
        p, q = self._vg_dev(source, np.float32), self._vg_dev(target, np.float32)
        ns, nt = int(p.shape[0]), int(q.shape[0])
        if int(si.shape[0]) != ns or int(ti.shape[0]) != nt:
            raise MiIcpError("fgr_correspondences: one neighbour per point is needed")
        dev = torch.device("cuda", self.device)
        room = max(0, min(int(maximum_tuple_count), 300 * min(ns, nt)))
        pairs, pp = self._out(MI_ICP_DEVICE, dev, (max(min(ns, nt), 1), 2), np.int32)
        corr, cp = self._out(MI_ICP_DEVICE, dev, (max(room, 1), 2), np.int32)
        n_pairs, n_corr = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.mi_icp_fgr_correspondences(self._ctx, self._ptr(si), ns, self._ptr(ti), nt, self._ptr(p), self._ptr(q),
                                                     float(tuple_scale), int(maximum_tuple_count), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                     pp, C.byref(n_pairs), cp, C.byref(n_corr)))
        return pairs[:int(n_pairs.value)], corr[:int(n_corr.value)]

    def fgr_optimize(self, source, target, corr, par_start, option=None):
        """mi_icp_fgr_optimize -> (T [4, 4] row-major numpy, the last iteration's 27 sums (float64), par after it)"""
        p, q = self._vg_dev(source, np.float32), self._vg_dev(target, np.float32)
        cr = self._vg_dev(corr, np.int32, 2)
        opt = self.fgr_option() if option is None else option
        dev = torch.device("cuda", self.device)
        T = torch.empty(16, dtype=torch.float32, device=dev)
        sums = torch.empty(27, dtype=torch.float64, device=dev)
        par = torch.empty(1, dtype=torch.float32, device=dev)
        self._chk(self._L.mi_icp_fgr_optimize(self._ctx, self._ptr(p), int(p.shape[0]), self._ptr(q), int(q.shape[0]), self._ptr(cr),
                                              int(cr.shape[0]), float(par_start), C.byref(opt), self._ptr(T), self._ptr(sums),
                                              self._ptr(par)))
        self.synchronize()
        return _T_out(T.cpu().numpy()), sums.cpu().numpy(), float(par.cpu()[0])

    def correspondences_from_features(self, source_features, target_features, mutual_filter=False, mutual_consistency_ratio=0.1):
        """mi_icp_correspondences_from_features -> int32 [m, 2] device tensor"""
        s, ns, dim = self._features(source_features, "correspondences_from_features")
        t, nt, tdim = self._features(target_features, "correspondences_from_features")
        if dim != tdim:
            raise MiIcpError("correspondences_from_features: dimensions %d and %d differ" % (dim, tdim))
        corr, cp = self._out(MI_ICP_DEVICE, torch.device("cuda", self.device), (max(ns, 1), 2), np.int32)
        m = C.c_int64(0)
        self._chk(self._L.mi_icp_correspondences_from_features(self._ctx, self._ptr(s), ns, self._ptr(t), nt, dim, int(bool(mutual_filter)),
                                                               float(mutual_consistency_ratio), cp, C.byref(m)))
        return corr[:int(m.value)]

    def fast_global_registration(self, source, target, source_features, target_features, option=None, seed=0):
        """mi_icp_fast_global_registration -> Result; the clouds stay loaded, get_correspondences() gives the set"""
        p, q = self._vg_dev(source, np.float32), self._vg_dev(target, np.float32)
        s, ns, dim = self._features(source_features, "fast_global_registration")
        t, nt, tdim = self._features(target_features, "fast_global_registration")
        if dim != tdim or ns != int(p.shape[0]) or nt != int(q.shape[0]):
            raise MiIcpError("fast_global_registration: one descriptor of one dimension per point is needed")
        opt = self.fgr_option() if option is None else option
        self.generation = getattr(self, "generation", 0) + 1   # (the call loads both clouds)
        res = Result()
        self._chk(self._L.mi_icp_fast_global_registration(self._ctx, self._ptr(p), self._ptr(s), ns, self._ptr(q), self._ptr(t), nt, dim,
                                                          C.byref(opt), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(res)))
        self.synchronize()
        self.n_source, self.n_target = ns, nt
        return res

    def compute_rgbd_odometry(self, source_color, source_depth, target_color, target_depth, intrinsic4,
                              odo_init=None, jacobian=1, iterations=(20, 10, 5), max_depth_diff=0.03,
                              min_depth=0.0, max_depth=4.0, weighted=False, prev_twist=None, nu=5.0,
                              sigma2_init=1.0, inv_sigma_mat_diag=None):
        """odometry::ComputeRGBDOdometry / ComputeWeightedRGBDOdometry (odometry/odometry.cu:833-943).
        Images: [H, W] float32, numpy or torch (all on the same side).  Returns (success, 4x4
        transformation, 6x6 information), with weighted=True (success, transformation, twist, information)."""
        imgs = [source_color, source_depth, target_color, target_depth]
        on_dev = _is_tensor(imgs[0]) and imgs[0].is_cuda
        keep, ptrs = [], []
        for x in imgs:
            if _is_tensor(x):
                if x.is_cuda != on_dev or x.dtype != torch.float32:
                    raise TypeError("odometry images must be float32 and live on the same side")
                x = x.contiguous() if on_dev else np.ascontiguousarray(x.numpy())
            else:
                if on_dev:
                    raise TypeError("odometry images must live on the same side")
                x = np.ascontiguousarray(x)
                if x.dtype != np.float32:
                    raise TypeError("odometry images must be float32")
            keep.append(x)
            ptrs.append(C.c_void_p(x.data_ptr()) if on_dev else x.ctypes.data_as(C.c_void_p))
        shape = tuple(keep[0].shape)
        if len(shape) != 2 or any(tuple(k.shape) != shape for k in keep):
            raise ValueError("[RGBDOdometry] Two RGBD pairs should be same in size.")
        from ._lib import OdometryOption
        opt = OdometryOption()
        opt.num_levels = len(iterations)
        for i, v in enumerate(list(iterations)[:8]):   # (more than 8 levels: the library reports it)
            opt.iterations[i] = int(v)
        opt.max_depth_diff, opt.min_depth, opt.max_depth = float(max_depth_diff), float(min_depth), float(max_depth)
        opt.nu, opt.sigma2_init = float(nu), float(sigma2_init)
        for i in range(6):
            opt.inv_sigma_mat_diag[i] = 0.0 if inv_sigma_mat_diag is None else float(inv_sigma_mat_diag[i])
        K = (C.c_float * 4)(*[float(v) for v in intrinsic4])
        init = None
        if odo_init is not None:
            init = np.ascontiguousarray(np.asarray(odo_init, np.float32).reshape(4, 4).T)
        ok = C.c_int(0)
        T = np.empty(16, np.float32)
        info = np.empty(36, np.float64)
        if weighted:
            pt = (C.c_float * 6)(*([0.0] * 6 if prev_twist is None else [float(v) for v in prev_twist]))
            tw = np.empty(6, np.float32)
            self._chk(self._L.mi_icp_compute_weighted_rgbd_odometry(
                self._ctx, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(shape[1]), int(shape[0]), K,
                None if init is None else init.ctypes.data_as(C.c_void_p), pt, C.byref(opt), C.byref(ok),
                T.ctypes.data_as(C.c_void_p), tw.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p),
                MI_ICP_DEVICE if on_dev else MI_ICP_HOST))
            return bool(ok.value), T.reshape(4, 4).T.copy(), tw, info.reshape(6, 6).copy()
        self._chk(self._L.mi_icp_compute_rgbd_odometry(
            self._ctx, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(shape[1]), int(shape[0]), K,
            None if init is None else init.ctypes.data_as(C.c_void_p), int(jacobian), C.byref(opt), C.byref(ok),
            T.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p), MI_ICP_DEVICE if on_dev else MI_ICP_HOST))
        return bool(ok.value), T.reshape(4, 4).T.copy(), info.reshape(6, 6).copy()

    def debug_odometry_image(self, level, which):
        """One image of the last odometry call (include/mi_icp_debug.h: level 0 = full size; which = 0 source colour,
        1 source depth, 2 target colour, 3 target depth, 4 dx colour, 5 dy colour, 6 dx depth, 7 dy depth) as a
        float32 [h, w] array.  Test-only, and valid only directly after compute_rgbd_odometry on this engine: the
        images live in scratch memory that other calls reuse."""
        w, h = C.c_int(0), C.c_int(0)
        self._chk(self._L.mi_icp_debug_odometry_image(self._ctx, int(level), int(which), None, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value), np.float32)
        self._chk(self._L.mi_icp_debug_odometry_image(self._ctx, int(level), int(which), out.ctypes.data_as(C.c_void_p),
                                                      C.byref(w), C.byref(h)))
        return out

    def covariances_from_normals(self, normals, epsilon=1e-3):
        n = _Buf(normals, np.float32, 3, self.device)
        out, optr = self._out(n.kind, n.device, (n.n, 9))
        self._chk(self._L.mi_icp_covariances_from_normals(self._ctx, n.ptr, n.n, float(epsilon),
                                                          optr, n.kind))
        return _cov_out(out)

    def estimate_normals_knn(self, points, knn=30):
        p = _Buf(points, np.float32, 3, self.device)
        out, optr = self._out(p.kind, p.device, (p.n, 3))
        self._chk(self._L.mi_icp_estimate_normals_knn(self._ctx, p.ptr, p.n, int(knn), optr, p.kind))
        return out

    def estimate_normals_radius(self, points, radius, max_nn=30):
        p = _Buf(points, np.float32, 3, self.device)
        out, optr = self._out(p.kind, p.device, (p.n, 3))
        self._chk(self._L.mi_icp_estimate_normals_radius(self._ctx, p.ptr, p.n, float(radius),
                                                         int(max_nn), optr, p.kind))
        return out

    # -- multi-GPU / instrumentation -------------------------------------------------------------
    def comm_init(self, unique_id, nranks, rank):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.mi_icp_comm_init(self._ctx, buf, int(nranks), int(rank)))

    def comm_init_local(self, job_name, nranks, rank):
        """node-local communicator: the shared-memory mailbox alone (csrc/mailbox.h), no RCCL"""
        self._chk(self._L.mi_icp_comm_init_local(self._ctx, str(job_name).encode(), int(nranks), int(rank)))

    def comm_kind(self):
        """0: none, 1: RCCL all-reduce, 2: shared-memory mailbox"""
        return int(self._L.mi_icp_comm_kind(self._ctx))

    def comm_autotune(self, exchanges=200):
        """Collective: self-test (known-answer) and time every available exchange path, keep the fastest that passed on
        every rank (mi_icp_comm_autotune).  Returns a dict: chosen ("host mailbox" / "device inboxes" / "rccl" / "none"),
        latency_us per path (None: not available, "failed": did not pass), rccl_comm_count, exchanges, verified."""
        lat = (C.c_double * 3)()
        info = (C.c_int * 4)()
        self._chk(self._L.mi_icp_comm_autotune(self._ctx, int(exchanges), lat, info))
        names = ("host mailbox", "device inboxes", "rccl")
        show = lambda v: None if v == -1.0 else ("failed" if v < 0 else round(float(v), 3))
        return {"chosen": names[info[0] - 1] if 1 <= info[0] <= 3 else "none",
                "latency_us": {n: show(lat[i]) for i, n in enumerate(names)},
                "rccl_comm_count": int(info[1]), "exchanges": int(info[2]), "verified": bool(info[3])}

    def comm_destroy(self):
        self._chk(self._L.mi_icp_comm_destroy(self._ctx))

    def set_iteration_callback(self, fn):
        """fn(iteration, fitness, inlier_rmse) once per iteration of the following loops, in order (what the
        reference logs at debug verbosity, registration.cu:155-156); None removes it."""
        from ._lib import ITERATION_FN
        self._iter_cb = None if fn is None else ITERATION_FN(lambda _user, i, f, r: fn(int(i), float(f), float(r)))
        self._chk(self._L.mi_icp_set_iteration_callback(self._ctx, C.cast(self._iter_cb, C.c_void_p) if self._iter_cb else None, None))

    def set_step_stamps(self, enable=True):
        """include/mi_icp_debug.h: the next loop runs the stamping instantiations of its kernels."""
        self._chk(self._L.mi_icp_debug_set_step_stamps(self._ctx, 1 if enable else 0))

    def get_step_stamps(self):
        """-> (32 stamp words as uint64, ticks per microsecond)"""
        out = np.zeros(32, np.uint64)
        tpu = C.c_double(0.0)
        self._chk(self._L.mi_icp_debug_get_step_stamps(self._ctx, out.ctypes.data_as(C.c_void_p), C.byref(tpu)))
        return out, float(tpu.value)

    def set_profiling(self, enable=True):
        self._chk(self._L.mi_icp_set_profiling(self._ctx, 1 if enable else 0))

    def get_profile(self):
        out = np.zeros(8, np.float64)
        self._chk(self._L.mi_icp_get_profile(self._ctx, out.ctypes.data_as(C.c_void_p)))
        return dict(nn_ms=out[0], nn_launches=int(out[1]), reduce_ms=out[2],
                    reduce_launches=int(out[3]), build_target_ms=out[4], build_source_ms=out[5],
                    halo_builds_by_loops=int(out[6]))


def comm_unique_id():
    L = _lib.load()
    buf = C.create_string_buffer(128)
    rc = L.mi_icp_comm_unique_id(buf)
    if rc != 0:
        raise MiIcpError("mi_icp_comm_unique_id failed (%d): RCCL not loadable" % rc)
    return bytes(buf.raw)


def _cov_in(covs):
    """(n,3,3) row-major user layout -> (n,9) column-major (Eigen::Matrix3f)."""
    if covs is None:
        return None
    if _is_tensor(covs):
        c = covs.reshape(-1, 3, 3)
        return c.transpose(1, 2).contiguous().reshape(-1, 9)
    c = np.asarray(covs, np.float32).reshape(-1, 3, 3)
    return np.ascontiguousarray(c.transpose(0, 2, 1)).reshape(-1, 9)


def _cov_out(c9):
    if c9 is None:
        return None
    if _is_tensor(c9):
        return c9.reshape(-1, 3, 3).transpose(1, 2).contiguous()
    return np.ascontiguousarray(np.asarray(c9).reshape(-1, 3, 3).transpose(0, 2, 1))


def solve_system(sys32, det_thresh=1e-6):
    L = _lib.load()
    sys32 = np.ascontiguousarray(sys32, np.float64)
    out = (C.c_float * 16)()
    ok = L.mi_icp_solve_system(sys32.ctypes.data_as(C.c_void_p), float(det_thresh), out)
    return bool(ok > 0), _T_out(out)


def kabsch_from_sums(sys32, n_model):
    L = _lib.load()
    sys32 = np.ascontiguousarray(sys32, np.float64)
    out = (C.c_float * 16)()
    L.mi_icp_kabsch_from_sums(sys32.ctypes.data_as(C.c_void_p), int(n_model), out)
    return _T_out(out)


def vector6_to_matrix4(x):
    L = _lib.load()
    x = np.ascontiguousarray(x, np.float32)
    out = (C.c_float * 16)()
    L.mi_icp_vector6_to_matrix4(x.ctypes.data_as(C.c_void_p), out)
    return _T_out(out)
