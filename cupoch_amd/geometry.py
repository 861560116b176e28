"""cupoch.geometry.PointCloud mirror (src/cupoch/geometry/pointcloud.h:43-263,
python surface src/python/cupoch_pybind/geometry/pointcloud.cpp:33-200) --
only the members the ICP path touches.  Arrays live on the GPU as torch
tensors; every operation below runs a HIP kernel through the C ABI.
OccupancyGrid / OccupancyVoxel mirror geometry/occupancygrid.h:31-142 (python surface
src/python/cupoch_pybind/geometry/occupancygrid.cpp); not built: OccupancyGrid.create_from_voxel_grid.
Voxel / VoxelGrid mirror geometry/voxelgrid.h:48-214 (python surface src/python/cupoch_pybind/geometry/voxelgrid.cpp);
not built: create_from_triangle_mesh[_within_bounds] (no TriangleMesh here), get_oriented_bounding_box, VoxelGrid file
I/O and visualisation.  The collision queries on both grid types are cupoch_amd.collision.
DistanceVoxel / DistanceTransform mirror geometry/distancetransform.h:30-78 (python surface
src/python/cupoch_pybind/geometry/distancetransform.cpp); not built: the planning and visualisation consumers of a
transform, and a transform as a collision target.
LineSet mirrors geometry/lineset.h (LineSet<3>; python surface src/python/cupoch_pybind/geometry/lineset.cpp); not
built: the factories from meshes, clouds with correspondences and oriented boxes, and file I/O.
Graph mirrors geometry/graph.h (Graph<3>; python surface src/python/cupoch_pybind/geometry/graph.cpp): the roadmap
cupoch_amd.planning searches; not built: Graph2D, create_from_triangle_mesh, file I/O and visualisation.
LaserScanBuffer mirrors geometry/laserscanbuffer.h (python surface src/python/cupoch_pybind/geometry/laserscanbuffer.cpp)
with PointCloud.create_from_laserscanbuffer; not built: file I/O and visualisation.
Image / RGBDImage mirror geometry/image.h and geometry/rgbdimage.h (python surface
src/python/cupoch_pybind/geometry/image.cpp): filters, bilateral filter, pyramids, format conversions and the RGB-D
factories, and PointCloud.create_from_disparity for the disparity image of cupoch_amd.imageproc; not built:
Image.FloatValueAt, image file I/O."""
import enum
import sys

import numpy as np

from . import _lib, utility
from .engine import Engine

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_engines = {}


def get_engine(device=None):
    """Process-wide engine per GPU (the reference's per-process allocator/streams)."""
    d = utility.default_device() if device is None else int(device)
    if d not in _engines:
        _engines[d] = Engine(d)
    return _engines[d]


class KDTreeSearchParamKNN:
    """knn::KDTreeSearchParamKNN (knn/kdtree_search_param.h:49-56)"""

    def __init__(self, knn=30):
        self.knn = int(knn)


class KDTreeSearchParamRadius:
    """knn::KDTreeSearchParamRadius (knn/kdtree_search_param.h:58-66)"""

    def __init__(self, radius, max_nn):   # no default in the reference either
        self.radius = float(radius)
        self.max_nn = int(max_nn)


class KDTreeFlann:
    """knn::KDTreeFlann (knn/kdtree_flann.h:43-124; python surface
    cupoch_pybind/geometry/kdtree_flann.cpp:88-141).  Owns its own engine context, i.e. its
    own tree; at most knn::NUM_MAX_NN = 100 neighbours per query."""

    def __init__(self, geometry=None):
        self._eng = None
        self._n = 0
        if geometry is not None:
            self.set_geometry(geometry)

    def set_geometry(self, geometry):
        pts = geometry.points.tensor if isinstance(geometry, PointCloud) else _v3(geometry).tensor
        if self._eng is None:
            self._eng = Engine(pts.device.index if pts.is_cuda else utility.default_device())
        self._eng.set_target(pts)
        self._n = int(pts.shape[0])
        return True

    # batch forms: (found, idx[nq, k], d2[nq, k]) on the device
    def search_knn(self, queries, knn):
        if self._n == 0:
            return -1, None, None
        return self._eng.search_knn(_v3(queries).tensor if not isinstance(queries, utility.Vector3fVector)
                                    else queries.tensor, knn)

    def search_radius(self, queries, radius, max_nn):
        if self._n == 0 or not radius > 0.0:   # (a non-positive radius holds no neighbours; the engine reads 0 as "unbounded")
            return -1, None, None
        return self._eng.search_knn(_v3(queries).tensor if not isinstance(queries, utility.Vector3fVector)
                                    else queries.tensor, max_nn, radius)

    # single-query forms of the pybind module: (k, indices, distance2) as host lists of length k
    def search_knn_vector_3f(self, query, knn):
        if self._n == 0:
            raise RuntimeError("search_knn_vector_3f() error!")
        k, idx, d2 = self._eng.search_knn(np.asarray(query, np.float32).reshape(1, 3), knn)
        return k, list(idx[0, :k]), list(d2[0, :k])

    def search_radius_vector_3f(self, query, radius, max_nn):
        if self._n == 0:
            raise RuntimeError("search_radius_vector_3f() error!")
        if not radius > 0.0:
            return 0, [], []
        k, idx, d2 = self._eng.search_knn(np.asarray(query, np.float32).reshape(1, 3), max_nn, radius)
        return k, list(idx[0, :k]), list(d2[0, :k])

    def search_vector_3f(self, query, search_param):
        if isinstance(search_param, KDTreeSearchParamRadius):
            return self.search_radius_vector_3f(query, search_param.radius, search_param.max_nn)
        return self.search_knn_vector_3f(query, search_param.knn)


class AxisAlignedBoundingBox:
    """geometry::AxisAlignedBoundingBox<3> (geometry/boundingvolume.h:121-230) as far as the
    ICP path's PointCloud hands it out: bounds, extent, centre, volume."""

    def __init__(self, min_bound=(0, 0, 0), max_bound=(0, 0, 0)):
        self.min_bound = np.asarray(min_bound, np.float32).reshape(3).copy()
        self.max_bound = np.asarray(max_bound, np.float32).reshape(3).copy()
        self.color = np.zeros(3, np.float32)

    def get_min_bound(self):
        return self.min_bound

    def get_max_bound(self):
        return self.max_bound

    def get_center(self):
        return ((self.min_bound + self.max_bound) * np.float32(0.5)).astype(np.float32)

    def get_extent(self):
        return self.max_bound - self.min_bound

    def get_half_extent(self):
        return self.get_extent() * np.float32(0.5)

    def get_max_extent(self):
        return float(self.get_extent().max())

    def volume(self):
        return float(np.prod(self.get_extent()))

    def is_empty(self):
        return self.volume() <= 0

    def __repr__(self):
        return "geometry::AxisAlignedBoundingBox with min_bound %s and max_bound %s" % (self.min_bound, self.max_bound)


class PointCloud:
    def __init__(self, points=None):
        self._points = utility.Vector3fVector() if points is None else _v3(points)
        self._normals = None
        self._colors = None
        self._covariances = None

    # device-vector style properties ------------------------------------------------
    @property
    def points(self):
        return self._points

    @points.setter
    def points(self, v):
        self._points = _v3(v)

    @property
    def normals(self):
        return self._normals if self._normals is not None else utility.Vector3fVector()

    @normals.setter
    def normals(self, v):
        self._normals = _v3(v)

    @property
    def colors(self):
        return self._colors if self._colors is not None else utility.Vector3fVector()

    @colors.setter
    def colors(self, v):
        self._colors = _v3(v)

    @property
    def covariances(self):
        return self._covariances if self._covariances is not None else utility.Matrix3fVector()

    @covariances.setter
    def covariances(self, v):
        self._covariances = v if isinstance(v, utility.Matrix3fVector) else utility.Matrix3fVector(v)

    # pointcloud.h:82-96 ------------------------------------------------------------------
    def has_points(self):
        return len(self._points) > 0

    def has_normals(self):
        return self.has_points() and self._normals is not None and len(self._normals) == len(self._points)

    def has_colors(self):
        return self.has_points() and self._colors is not None and len(self._colors) == len(self._points)

    def has_covariances(self):
        return (self.has_points() and self._covariances is not None
                and len(self._covariances) == len(self._points))

    def is_empty(self):
        return not self.has_points()

    def clear(self):
        """PointCloud::Clear"""
        self._points, self._normals, self._colors, self._covariances = utility.Vector3fVector(), None, None, None
        return self

    def clone(self):
        out = PointCloud()
        out._points = utility.Vector3fVector(self._points.tensor.clone())
        for name in ("_normals", "_colors"):
            v = getattr(self, name)
            if v is not None:
                setattr(out, name, utility.Vector3fVector(v.tensor.clone()))
        if self._covariances is not None:
            out._covariances = utility.Matrix3fVector(self._covariances.tensor.clone())
        return out

    # PointCloud::Transform (pointcloud.cu:293-299) ------------------------------------------
    # GeometryBase3D (geometry/geometry_base.h:44-90, geometry/pointcloud.cu:205-242) ---------------
    def _bounds(self):
        return get_engine(self._points.tensor.device.index if self._points.tensor.is_cuda else None) \
            .compute_bounds(self._points.tensor)

    def get_min_bound(self):
        return self._bounds()[0]

    def get_max_bound(self):
        return self._bounds()[1]

    def get_center(self):
        return self._bounds()[2]

    def get_axis_aligned_bounding_box(self):
        mn, mx, _ = self._bounds()
        return AxisAlignedBoundingBox(mn, mx)

    def _affine(self, with_attributes, **kw):
        eng = get_engine(self._points.tensor.device.index if self._points.tensor.is_cuda else None)
        n = self._normals.tensor if with_attributes and self._normals is not None and len(self._normals) else None
        c = self._covariances.tensor if with_attributes and self._covariances is not None and len(self._covariances) else None
        _, _, c_new = eng.affine(self._points.tensor, n, c, **kw)
        if c_new is not None:
            self._covariances.tensor = c_new
        return self

    def translate(self, translation, relative=True):
        t = np.asarray(translation, np.float32).reshape(3)
        if not relative:
            t = (t - self.get_center()).astype(np.float32)
        return self._affine(False, translate=t)

    def scale(self, scale, center=True):
        c = self.get_center() if center and len(self._points) else None
        return self._affine(False, scale=float(scale), center=c)

    def rotate(self, R, center=True):
        c = self.get_center() if center and len(self._points) else None
        return self._affine(True, R=np.asarray(R, np.float32).reshape(3, 3), center=c)

    def transform(self, transformation):
        eng = get_engine(self._points.tensor.device.index)
        n = self._normals.tensor if self._normals is not None and len(self._normals) else None
        c = self._covariances.tensor if self._covariances is not None and len(self._covariances) else None
        _, _, c_new = eng.transform(np.asarray(transformation, np.float32), self._points.tensor, n, c)
        if c_new is not None:
            self._covariances.tensor = c_new
        return self

    # PointCloud::VoxelDownSample (down_sample.cu:170-273) --------------------------------------
    def voxel_down_sample(self, voxel_size):
        out = PointCloud()
        if not self.has_points():
            return out
        eng = get_engine(self._points.tensor.device.index)
        n = self._normals.tensor if self.has_normals() else None
        c = self._colors.tensor if self.has_colors() else None
        p2, n2, c2 = eng.voxel_downsample(self._points.tensor, float(voxel_size), n, c)
        out._points = utility.Vector3fVector(p2.clone())
        if n2 is not None:
            out._normals = utility.Vector3fVector(n2.clone())
        if c2 is not None:
            out._colors = utility.Vector3fVector(c2.clone())
        return out

    # PointCloud::SelectByIndex / UniformDownSample / Remove*Outliers (down_sample.cu:40-438) ---------------------
    def _engine_args(self):
        eng = get_engine(self._points.tensor.device.index)
        n = self._normals.tensor if self.has_normals() else None
        c = self._colors.tensor if self.has_colors() else None
        return eng, n, c

    @staticmethod
    def _made(p, n, c):
        out = PointCloud()
        out._points = utility.Vector3fVector(p.clone())
        if n is not None:
            out._normals = utility.Vector3fVector(n.clone())
        if c is not None:
            out._colors = utility.Vector3fVector(c.clone())
        return out

    def select_by_index(self, indices, invert=False):
        """points, normals and colours at `indices` (a ULongVector, list, numpy array or tensor), in that order;
        invert=True: the points not named, ascending"""
        if isinstance(indices, utility.DeviceVector):
            indices = indices.tensor
        eng, n, c = self._engine_args()
        return self._made(*eng.select_by_index(self._points.tensor, indices, bool(invert), n, c))

    def select_by_mask(self, mask, invert=False):
        """points, normals and colours of the entries whose mask entry is set (a BoolVector, list, numpy array or
        tensor of one entry per point; invert=True: not set), ascending"""
        if isinstance(mask, utility.DeviceVector):
            mask = mask.tensor
        if len(mask) != len(self._points):
            print("[cupoch_amd] Error: [SelectByMask] The point size should be equal to the mask size.")
            return PointCloud()         # (down_sample.cu:134-137 logs and returns an empty cloud)
        if not self.has_points():
            return PointCloud()
        eng, n, c = self._engine_args()
        return self._made(*eng.select_by_mask(self._points.tensor, mask, bool(invert), n, c))

    def uniform_down_sample(self, every_k_points):
        eng, n, c = self._engine_args()
        return self._made(*eng.uniform_downsample(self._points.tensor, int(every_k_points), n, c))

    def remove_statistical_outlier(self, nb_neighbors, std_ratio):
        """(PointCloud of the kept points, ULongVector of their indices)"""
        eng, n, c = self._engine_args()
        p2, n2, c2, idx, _ = eng.remove_statistical_outliers(self._points.tensor, int(nb_neighbors), float(std_ratio), n, c)
        return self._made(p2, n2, c2), utility.ULongVector(idx.clone())

    def remove_radius_outlier(self, nb_points, radius):
        """(PointCloud of the kept points, ULongVector of their indices)"""
        eng, n, c = self._engine_args()
        p2, n2, c2, idx, _ = eng.remove_radius_outliers(self._points.tensor, int(nb_points), float(radius), n, c)
        return self._made(p2, n2, c2), utility.ULongVector(idx.clone())

    # PointCloud::FarthestPointDownSample / GaussianFilter / PassThroughFilter / Crop / RemoveNoneFinitePoints ------
    # (pointcloud.cu:40-139, 301-466; include/mi_icp.h states the contracts)
    def farthest_point_down_sample(self, num_samples):
        """num_samples points, each the farthest from those chosen before it; point 0 first, ties to the lowest index"""
        num_samples = int(num_samples)
        if num_samples == 0:
            return PointCloud()
        if num_samples < 0 or num_samples > len(self._points):
            print("[cupoch_amd] Error: Illegal number of samples: %d, must <= point size: %d" % (num_samples, len(self._points)))
            return PointCloud()
        eng, n, c = self._engine_args()
        return self._made(*eng.farthest_point_downsample(self._points.tensor, num_samples, n, c)[:3])

    def gaussian_filter(self, search_radius, sigma2, num_max_search_points=50):
        """every point, normal and colour replaced by the mean of its radius neighbours weighted with
        exp(-0.5 d2 / sigma2); normals are not re-normalised"""
        if not (search_radius > 0 and sigma2 > 0 and 1 <= int(num_max_search_points) <= 100):
            print("[cupoch_amd] Error: [GaussianFilter] Illegal input parameters, radius and sigma2 must be positive.")
            return PointCloud()         # (pointcloud.cu:390-395 logs and returns an empty cloud)
        if not self.has_points():
            return PointCloud()
        eng, n, c = self._engine_args()
        return self._made(*eng.gaussian_filter(self._points.tensor, float(search_radius), float(sigma2),
                                               int(num_max_search_points), n, c))

    def pass_through_filter(self, axis_no, min_bound, max_bound):
        """the points whose coordinate axis_no lies in [min_bound, max_bound]"""
        if int(axis_no) not in (0, 1, 2):
            print("[cupoch_amd] Error: [PassThroughFilter] Illegal input parameters, axis_no must be 0, 1 or 2.")
            return PointCloud()         # (pointcloud.cu:440-445)
        if not self.has_points():
            return PointCloud()
        eng, n, c = self._engine_args()
        return self._made(*eng.pass_through_filter(self._points.tensor, int(axis_no), float(min_bound), float(max_bound), n, c)[:3])

    def crop(self, bounding_box):
        """the points inside the closed AxisAlignedBoundingBox"""
        if not isinstance(bounding_box, AxisAlignedBoundingBox):
            raise TypeError("crop() takes an AxisAlignedBoundingBox (an OrientedBoundingBox is not supported)")
        if not bounding_box.volume() > 0:
            print("[cupoch_amd] Error: [CropPointCloud] AxisAlignedBoundingBox either has zeros size, or has wrong bounds.")
            return PointCloud()
        if not self.has_points():
            return PointCloud()
        eng, n, c = self._engine_args()
        return self._made(*eng.crop_aabb(self._points.tensor, bounding_box.min_bound, bounding_box.max_bound, n, c)[:3])

    def remove_none_finite_points(self, remove_nan=True, remove_infinite=True):
        """drops, in place, the points with a NaN (remove_nan) or infinite (remove_infinite) coordinate, with their
        normals and colours; returns self"""
        if not self.has_points():
            return self
        eng, n, c = self._engine_args()
        p2, n2, c2, _ = eng.remove_none_finite(self._points.tensor, bool(remove_nan), bool(remove_infinite), n, c)
        self._points = utility.Vector3fVector(p2.clone())
        if n2 is not None:
            self._normals = utility.Vector3fVector(n2.clone())
        if c2 is not None:
            self._colors = utility.Vector3fVector(c2.clone())
        if self._covariances is not None and len(self._covariances) != len(self._points):
            self._covariances = None      # (the reference does not carry them either)
        return self

    # PointCloud::ClusterDBSCAN (pointcloud_cluster.cu:109-179) ----------------------------------------------------
    def cluster_dbscan(self, eps, min_points, print_progress=False, max_edges=100):
        """an IntVector of one label per point: its cluster's number, or -1 for noise (include/mi_icp.h states the
        contract).  print_progress is accepted and prints nothing."""
        eng = get_engine(self._points.tensor.device.index)
        labels, _, _ = eng.cluster_dbscan(self._points.tensor, float(eps), int(min_points), int(max_edges))
        return utility.IntVector(labels)

    # PointCloud::SegmentPlane (segmentation.cu:187-268) -------------------------------------------------------------
    def segment_plane(self, distance_threshold=0.01, ransac_n=3, num_iterations=100, seed=None):
        """(plane_model float32[4], ULongVector of the inliers' indices): RANSAC over planes through three points, the
        winner refit to its inliers (include/mi_icp.h states the contract).  seed=None draws one from Python's
        `random` module, as the reference draws from rand(); the same seed gives the same result."""
        if seed is None:
            import random
            seed = random.getrandbits(64)
        eng = get_engine(self._points.tensor.device.index)
        plane, idx, _, _, _ = eng.segment_plane(self._points.tensor, float(distance_threshold), int(ransac_n),
                                                int(num_iterations), int(seed))
        return plane, utility.ULongVector(idx.clone())

    # PointCloud::EstimateNormals (estimate_normals.cu:82-127): KNN or Radius search parameter ----------
    def estimate_normals(self, search_param=None):
        eng = get_engine(self._points.tensor.device.index)
        if isinstance(search_param, KDTreeSearchParamRadius):
            nrm = eng.estimate_normals_radius(self._points.tensor, search_param.radius, search_param.max_nn)
        else:
            k = 30 if search_param is None else int(getattr(search_param, "knn", 30))
            nrm = eng.estimate_normals_knn(self._points.tensor, k)
        self._normals = utility.Vector3fVector(nrm)
        return True


class keypoint:
    """geometry::keypoint (geometry/keypoint.h; python surface cupoch_pybind/geometry/keypoint.cpp)"""

    @staticmethod
    def compute_iss_keypoints(input, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975,
                              min_neighbors=5, max_neighbors=100):
        """(PointCloud of the ISS keypoints, BoolVector of one entry per input point); include/mi_icp.h states the
        contract.  A radius of 0 has both radii computed from the cloud's resolution."""
        if not input.has_points():
            print("[cupoch_amd] Warning: [ComputeISSKeypoints] Input PointCloud is empty!")
            return PointCloud(), utility.BoolVector()
        eng = get_engine(input.points.tensor.device.index)
        mask, _, _ = eng.iss_keypoints(input.points.tensor, float(salient_radius), float(non_max_radius), float(gamma_21),
                                       float(gamma_32), int(min_neighbors), int(max_neighbors))
        return input.select_by_mask(mask), utility.BoolVector(mask)


class ImageFilterType(enum.IntEnum):
    """Image::FilterType with the names of the reference's Python module"""
    Gaussian3 = 0
    Gaussian5 = 1
    Gaussian7 = 2
    Sobel3dx = 3
    Sobel3dy = 4


class ImageColorToIntensityConversionType(enum.IntEnum):
    """Image::ColorToIntensityConversionType.  The reference's Python module misnames the two values Gaussian3 and
    Gaussian5; those names stay as aliases."""
    Equal = 0
    Weighted = 1
    Gaussian3 = 0
    Gaussian5 = 1


_FILTER_TAPS = {
    ImageFilterType.Gaussian3: ((.25, .5, .25),) * 2,
    ImageFilterType.Gaussian5: ((.0625, .25, .375, .25, .0625),) * 2,
    ImageFilterType.Gaussian7: ((.03125, .109375, .21875, .28125, .21875, .109375, .03125),) * 2,
    ImageFilterType.Sobel3dx: ((-1.0, 0.0, 1.0), (1.0, 2.0, 1.0)),
    ImageFilterType.Sobel3dy: ((1.0, 2.0, 1.0), (-1.0, 0.0, 1.0)),
}
IMAGE_MAX_TAPS = 31           # MI_ICP_IMAGE_MAX_TAPS
IMAGE_MAX_DIAMETER = 31       # MI_ICP_IMAGE_MAX_DIAMETER


def _image_error(name, what="Unsupported image format."):
    print("[cupoch_amd] Error: [%s] %s" % (name, what))


class Image:
    """geometry::Image (geometry/image.h; python surface cupoch_pybind/geometry/image.cpp): a [H, W] or [H, W, C] array
    of uint8, uint16 or float32 -- numpy, or a torch tensor on either side -- in `data`.  include/mi_icp.h ("image")
    states what every operation computes.  Results are new Images whose pixels stay on the device (a torch tensor);
    np.asarray(img) brings them to the host.  As in the reference, a format an operation does not take is printed
    ("[cupoch_amd] Error: [<Name>] Unsupported image format.") and the call returns an empty Image (self for the two
    in-place calls); nothing is raised.  filter, bilateral_filter and create_pyramid first make a float image of
    anything that is not 1 x float32, as the reference's Python module does; filter_taps / filter_horizontal, the C++
    Filter(dx, dy) / FilterHorizontal, turn such input away.  Not built: FloatValueAt, file I/O."""

    def __init__(self, data=None):
        self.data = _img(data)

    # ---- the container
    @property
    def height(self):
        return 0 if self.data is None else int(self.data.shape[0])

    @property
    def width(self):
        return 0 if self.data is None or len(self.data.shape) < 2 else int(self.data.shape[1])

    @property
    def num_of_channels(self):
        return 0 if self.data is None else (int(self.data.shape[2]) if len(self.data.shape) == 3 else 1)

    @property
    def bytes_per_channel(self):
        if self.data is None:
            return 0
        return int(self.data.element_size()) if _is_torch(self.data) else int(self.data.dtype.itemsize)

    def is_empty(self):
        return self.width <= 0 or self.height <= 0 or self.num_of_channels <= 0

    def __repr__(self):
        return "Image of size %dx%d, with %d channels." % (self.width, self.height, self.num_of_channels)

    def __array__(self, dtype=None, copy=None):
        d = self.data
        a = np.zeros((0, 0), np.uint8) if d is None else (d.detach().cpu().numpy() if _is_torch(d) else np.asarray(d))
        return a if dtype is None else a.astype(dtype)

    def clear(self):
        """Image::Clear"""
        self.data = None
        return self

    def get_min_bound(self):
        return np.zeros(2, np.float32)

    def get_max_bound(self):
        return np.array([self.width, self.height], np.float32)

    def bytes_per_line(self):
        """Image::BytesPerLine"""
        return self.width * self.num_of_channels * self.bytes_per_channel

    def test_image_boundary(self, u, v, inner_margin=0.0):
        """Image::TestImageBoundary"""
        return bool(u >= inner_margin and u < self.width - inner_margin and v >= inner_margin and v < self.height - inner_margin)

    # ---- staging
    def _is(self, channels, bytes_per_channel):
        return (not self.is_empty()) and self.num_of_channels == channels and self.bytes_per_channel == bytes_per_channel

    def _kind_ok(self):
        name = str(self.data.dtype).replace("torch.", "")
        return name in ("uint8", "uint16", "float32") and len(self.data.shape) in (2, 3)

    def _staged(self):
        """(engine, the pixels as a contiguous device tensor)"""
        d = self.data
        if _is_torch(d) and d.is_cuda:
            return get_engine(d.device.index), d.contiguous()
        eng = get_engine()
        a = d.detach().numpy() if _is_torch(d) else np.asarray(d)
        return eng, torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", eng.device))

    @staticmethod
    def _empty():
        return Image()

    # ---- in place
    def clip_intensity(self, min=0.0, max=1.0):
        if not self._is(1, 4):
            _image_error("ClipIntensity")
            return self
        eng, t = self._staged()
        eng.image_clip(t, min, max)
        self.data = t
        return self

    def linear_transform(self, scale=1.0, offset=0.0):
        if self.is_empty() or not (self.bytes_per_channel == 1 or self._is(1, 4)) or self.num_of_channels > 4:
            _image_error("LinearTransform")
            return self
        eng, t = self._staged()
        eng.image_linear_transform(t, scale, offset)
        self.data = t
        return self

    # ---- new images
    def downsample(self):
        if not (self._is(1, 4) or self._is(3, 1)):
            _image_error("Downsample")
            return self._empty()
        if self.width // 2 == 0 or self.height // 2 == 0:
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_downsample(t))

    def filter_horizontal(self, kernel):
        """Image::FilterHorizontal (C++ only in the reference)"""
        k = np.asarray(kernel, np.float32).reshape(-1)
        if not self._is(1, 4) or k.size % 2 != 1 or k.size > IMAGE_MAX_TAPS:
            _image_error("FilterHorizontal", "Unsupported image format or kernel size.")
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_filter(t.reshape(self.height, self.width), k))

    def filter_taps(self, dx, dy):
        """Image::Filter(dx, dy) (C++ only in the reference): odd tap counts up to IMAGE_MAX_TAPS"""
        kx, ky = np.asarray(dx, np.float32).reshape(-1), np.asarray(dy, np.float32).reshape(-1)
        if not self._is(1, 4):
            _image_error("Filter")
            return self._empty()
        if kx.size % 2 != 1 or ky.size % 2 != 1 or kx.size > IMAGE_MAX_TAPS or ky.size > IMAGE_MAX_TAPS:
            _image_error("FilterHorizontal", "Unsupported image format or kernel size.")
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_filter(t.reshape(self.height, self.width), kx, ky))

    def _as_float(self):
        return self if self._is(1, 4) else self.create_float_image()

    def filter(self, filter_type):
        try:
            taps = _FILTER_TAPS[ImageFilterType(int(filter_type))]
        except ValueError:
            _image_error("Filter", "Unsupported filter type.")
            return self._empty()
        f = self._as_float()
        return self._empty() if f.is_empty() else f.filter_taps(*taps)

    def flip_vertical(self):
        return self._move(1, "FlipVertical")

    def flip_horizontal(self):
        return self._move(2, "FlipHorizontal")

    def transpose(self):
        """Image::Transpose (C++ only in the reference)"""
        return self._move(0, "Transpose")

    def _move(self, op, name):
        if self.is_empty():
            return self._empty()
        if not self._kind_ok() or self.num_of_channels * self.bytes_per_channel > 16:
            _image_error(name)
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_move(t, op))

    def bilateral_filter(self, diameter, sigma_color, sigma_space):
        """`diameter` is a radius: the window is (2 diameter + 1)^2, diameter in [0, IMAGE_MAX_DIAMETER]"""
        if int(diameter) < 0 or int(diameter) > IMAGE_MAX_DIAMETER:
            _image_error("BilateralFilter", "Diameter should be in [0, %d]." % IMAGE_MAX_DIAMETER)
            return self._empty()
        f = self._as_float()
        if f.is_empty():
            return self._empty()
        eng, t = f._staged()
        return Image(eng.image_bilateral(t.reshape(f.height, f.width), int(diameter), sigma_color, sigma_space))

    def _convertible(self, name):
        if self.is_empty():
            return False
        if not self._kind_ok() or self.num_of_channels > 4:
            _image_error(name)
            return False
        return True

    def create_gray_image(self, type=ImageColorToIntensityConversionType.Weighted):
        if not self._convertible("CreateGrayImage"):
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_create_gray(t, int(type)))

    def create_float_image(self, type=ImageColorToIntensityConversionType.Weighted):
        if not self._convertible("CreateFloatImage"):
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_create_float(t, int(type)))

    def convert_depth_to_float_image(self, depth_scale=1000.0, depth_trunc=3.0):
        """Image::ConvertDepthToFloatImage (C++ only in the reference)"""
        if not self._convertible("ConvertDepthToFloatImage"):
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_depth_to_float(t, depth_scale, depth_trunc))

    def create_image_from_float_image(self, bytes_per_channel):
        """Image::CreateImageFromFloatImage<uint8_t> (1) / <uint16_t> (2) (C++ only in the reference)"""
        if not self._is(1, 4) or int(bytes_per_channel) not in (1, 2):
            _image_error("CreateImageFromFloatImage")
            return self._empty()
        eng, t = self._staged()
        return Image(eng.image_from_float(t.reshape(self.height, self.width), int(bytes_per_channel)))

    def _pyramid(self, num_of_levels, with_gaussian_filter):
        """Image::CreatePyramid on 1 x float32 or 3 x uint8 (the C++ rule)"""
        if not (self._is(1, 4) or self._is(3, 1)):
            _image_error("CreateImagePyramid")
            return []
        eng, t = self._staged()
        if self.num_of_channels == 1:
            t = t.reshape(self.height, self.width)
        levels = []
        for i in range(int(num_of_levels)):
            if i == 0:
                levels.append(Image(t.clone()))
                continue
            prev = levels[-1]
            if prev.is_empty() or prev.width // 2 == 0 or prev.height // 2 == 0:
                levels.append(Image())
            elif with_gaussian_filter and self.num_of_channels == 1:
                levels.append(Image(eng.image_pyramid_level(prev.data)))
            else:
                levels.append(Image(eng.image_downsample(prev.data)))
        return levels

    def create_pyramid(self, num_of_levels, with_gaussian_filter):
        f = self._as_float()
        return [] if f.is_empty() else f._pyramid(num_of_levels, with_gaussian_filter)

    @staticmethod
    def filter_pyramid(image_pyramid, filter_type):
        taps = _FILTER_TAPS[ImageFilterType(int(filter_type))]
        return [Image(level).filter_taps(*taps) for level in image_pyramid]

    @staticmethod
    def bilateral_filter_pyramid(image_pyramid, diameter, sigma_color, sigma_space):
        out = []
        for level in image_pyramid:
            level = Image(level)
            if not level._is(1, 4):
                _image_error("BilateralFilter")
                out.append(Image())
            else:
                out.append(level.bilateral_filter(diameter, sigma_color, sigma_space))
        return out


def _img(x):
    return x.data if isinstance(x, Image) else x


class RGBDImage:
    """geometry::RGBDImage (geometry/rgbdimage.h; python surface cupoch_pybind/geometry/image.cpp): colour + depth.
    `color` and `depth` hold the pixel arrays themselves (what Image.data holds), as every consumer here reads them;
    the factories below leave device tensors there.  Errors are printed, as for Image."""

    def __init__(self, color=None, depth=None):
        self.color = _img(color)
        self.depth = _img(depth)

    def is_empty(self):
        return Image(self.color).is_empty() or Image(self.depth).is_empty()

    def __repr__(self):
        c, d = Image(self.color), Image(self.depth)
        return ("RGBDImage of size \nColor image : %dx%d, with %d channels.\nDepth image : %dx%d, with %d channels.\n"
                "Use numpy.asarray to access buffer data." % (c.width, c.height, c.num_of_channels, d.width, d.height,
                                                               d.num_of_channels))

    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True,
                                    _name="CreateFromColorAndDepth"):
        color, depth = Image(color), Image(depth)
        if color.height != depth.height or color.width != depth.width:
            _image_error(_name)
            return RGBDImage()
        d = depth.convert_depth_to_float_image(depth_scale, depth_trunc)
        if convert_rgb_to_intensity:
            c = color.create_float_image()
        else:
            c = Image() if color.is_empty() else Image(color._staged()[1].clone())
        return RGBDImage(c, d)

    @staticmethod
    def create_from_redwood_format(color, depth, convert_rgb_to_intensity=True):
        return RGBDImage.create_from_color_and_depth(color, depth, 1000.0, 4.0, convert_rgb_to_intensity)

    @staticmethod
    def create_from_tum_format(color, depth, convert_rgb_to_intensity=True):
        return RGBDImage.create_from_color_and_depth(color, depth, 5000.0, 4.0, convert_rgb_to_intensity)

    @staticmethod
    def _decoded(color, depth, fmt, name, convert_rgb_to_intensity):
        color, depth = Image(color), Image(depth)
        if color.height != depth.height or color.width != depth.width or not depth._is(1, 2):
            _image_error(name)
            return RGBDImage()
        eng, t = depth._staged()
        decoded = Image(eng.image_depth_format(t.reshape(depth.height, depth.width), fmt))
        return RGBDImage.create_from_color_and_depth(color, decoded, 1000.0, 7.0, convert_rgb_to_intensity, _name=name)

    @staticmethod
    def create_from_sun_format(color, depth, convert_rgb_to_intensity=True):
        return RGBDImage._decoded(color, depth, 0, "CreateRGBDImageFromSUNFormat", convert_rgb_to_intensity)

    @staticmethod
    def create_from_nyu_format(color, depth, convert_rgb_to_intensity=True):
        return RGBDImage._decoded(color, depth, 1, "CreateRGBDImageFromNYUFormat", convert_rgb_to_intensity)

    def create_pyramid(self, num_of_levels, with_gaussian_filter_for_color=True, with_gaussian_filter_for_depth=False):
        """RGBDImage::CreatePyramid: the C++ rule for both images (1 x float32 or 3 x uint8)"""
        c = Image(self.color)._pyramid(num_of_levels, with_gaussian_filter_for_color)
        d = Image(self.depth)._pyramid(num_of_levels, with_gaussian_filter_for_depth)
        if len(c) != int(num_of_levels) or len(d) != int(num_of_levels):
            return []
        return [RGBDImage(a, b) for a, b in zip(c, d)]

    @staticmethod
    def filter_pyramid(rgbd_image_pyramid, filter_type):
        return [RGBDImage(*Image.filter_pyramid([level.color, level.depth], filter_type)) for level in rgbd_image_pyramid]

    @staticmethod
    def bilateral_filter_pyramid_depth(rgbd_image_pyramid, diameter, sigma_depth, sigma_space):
        return [RGBDImage(level.color, Image.bilateral_filter_pyramid([level.depth], diameter, sigma_depth, sigma_space)[0])
                for level in rgbd_image_pyramid]


def _create_from_depth_image(depth, intrinsic, extrinsic=None, depth_scale=1000.0, depth_trunc=1000.0, stride=1):
    """PointCloud::CreateFromDepthImage (pointcloud_factory.cu:329-351)"""
    d = _img(depth)
    name = str(d.dtype).replace("torch.", "")
    out = PointCloud()
    if d.ndim != 2 or name not in ("float32", "uint16"):
        print("[cupoch_amd] Error: [PointCloud::CreateFromDepthImage] Unsupported image format.")
        return out
    dev = d.device.index if (torch is not None and torch.is_tensor(d) and d.is_cuda) else None
    p, _, _ = get_engine(dev).create_from_depth(d, intrinsic.as4(), extrinsic, None, depth_scale, depth_trunc,
                                                -1.0, stride, False, False, True)
    out._points = utility.Vector3fVector(p)
    return out


def _create_from_rgbd_image(image, intrinsic, extrinsic=None, project_valid_depth_only=True, depth_cutoff=-1.0,
                            compute_normals=False):
    """PointCloud::CreateFromRGBDImage (pointcloud_factory.cu:353-376).  image.color may be
    None (depth-only frames, as KinFu's point-to-plane tracking uses them)."""
    out = PointCloud()
    d, c = image.depth, image.color
    if str(d.dtype).replace("torch.", "") != "float32":
        print("[cupoch_amd] Error: [PointCloud::CreateFromRGBDImage] Unsupported image format.")
        return out
    dev = d.device.index if (torch is not None and torch.is_tensor(d) and d.is_cuda) else None
    try:
        p, n, col = get_engine(dev).create_from_depth(d, intrinsic.as4(), extrinsic, c, 1000.0, 1000.0, depth_cutoff,
                                                      1, True, compute_normals, project_valid_depth_only)
    except TypeError:
        print("[cupoch_amd] Error: [PointCloud::CreateFromRGBDImage] Unsupported image format.")
        return out
    out._points = utility.Vector3fVector(p)
    if n is not None:
        out._normals = utility.Vector3fVector(n)
    if col is not None:
        out._colors = utility.Vector3fVector(col)
    return out


def disparity_q(left_intrinsic, right_intrinsic, baseline):
    """the seven entries {q00, q03, q11, q13, q23, q32, q33} of CreateFromDisparity's matrix (pointcloud_factory.cu:444-455),
    formed in fp32 from left to right"""
    F = np.float32
    (fx, fy), (cx, cy) = [tuple(F(v) for v in pair) for pair in (left_intrinsic.get_focal_length(), left_intrinsic.get_principal_point())]
    cxr = F(right_intrinsic.get_principal_point()[0])
    tx = -F(baseline)
    return np.array([fy * tx, -fy * cx * tx, fx * tx, -fx * cy * tx, fx * fy * tx, -fy, fy * (cx - cxr)], F)


def _create_from_disparity(disp, color, left_intrinsic, right_intrinsic, baseline):
    """PointCloud::CreateFromDisparity (pointcloud_factory.cu:432-482): one point and one colour per pixel in raster
    order, nothing left out -- a disparity at which w = 0 gives non-finite coordinates (remove_none_finite_points takes
    them out).  disp 1 x uint8, color the same size with 3 channels of uint8 or uint16; anything else is logged and
    gives an empty cloud."""
    disp, color = (x if isinstance(x, Image) else Image(x) for x in (disp, color))
    out = PointCloud()
    if not (disp._is(1, 1) and (color._is(3, 1) or color._is(3, 2)) and (disp.width, disp.height) == (color.width, color.height)):
        print("[cupoch_amd] Error: [PointCloud::CreateFromDisparity] Unsupported image format.")
        return out
    eng, d = disp._staged()
    c = color.data
    if not (_is_torch(c) and c.is_cuda):
        c = torch.from_numpy(np.ascontiguousarray(c.detach().numpy() if _is_torch(c) else np.asarray(c))).to(d.device)
    p, col = eng.create_from_disparity(d.reshape(disp.height, disp.width), c.contiguous(),
                                       disparity_q(left_intrinsic, right_intrinsic, baseline))
    out._points = utility.Vector3fVector(p)
    out._colors = utility.Vector3fVector(col)
    return out


PointCloud.create_from_depth_image = staticmethod(_create_from_depth_image)
PointCloud.create_from_disparity = staticmethod(_create_from_disparity)
PointCloud.create_from_rgbd_image = staticmethod(_create_from_rgbd_image)


class OccupancyVoxel:
    """geometry::OccupancyVoxel (occupancygrid.h:31-51): grid index, log odds, colour"""

    def __init__(self, grid_index=(0, 0, 0), prob_log=float("nan"), color=(0.0, 0.0, 1.0)):
        self.grid_index = np.asarray(grid_index, np.int32).reshape(3).copy()
        self.prob_log = float(np.float32(prob_log))
        self.color = np.asarray(color, np.float32).reshape(3).copy()

    def __repr__(self):
        g, c = self.grid_index, self.color
        return "geometry::OccupancyVoxel with grid_index: (%d, %d, %d), prob_log: %g, color: (%g, %g, %g)" % (
            g[0], g[1], g[2], self.prob_log, c[0], c[1], c[2])


class OccupancyVoxels:
    """what an extraction returns: grid_index [m, 3] int32 and prob_log [m] as device tensors, ascending in linear
    index; every colour is (0, 0, 1).  len() and [] give OccupancyVoxel objects."""

    def __init__(self, grid_index, prob_log):
        self.grid_index = grid_index
        self.prob_log = prob_log

    def __len__(self):
        return int(self.prob_log.shape[0])

    def __getitem__(self, i):
        return OccupancyVoxel(self.grid_index[i].cpu().numpy(), float(self.prob_log[i]))

    def cpu(self):
        """-> (grid_index, prob_log) as numpy arrays"""
        return self.grid_index.cpu().numpy(), self.prob_log.cpu().numpy()


class OccupancyGrid:
    """geometry::OccupancyGrid (occupancygrid.h:71-142).  The attributes are the reference's public members and are
    read when a call is made; the voxels live on the GPU, made on first use (a changed `resolution` rebuilds the grid,
    every voxel unknown, as reconstruct does).  Deviations from the reference: DESIGN.md section 6."""

    KNOWN, FREE, OCCUPIED = 0, 1, 2

    def __init__(self, voxel_size=0.05, resolution=512, origin=(0.0, 0.0, 0.0), device=None):
        self.voxel_size = float(np.float32(voxel_size))
        self.resolution = int(resolution)
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self.clamping_thres_min = -2.0
        self.clamping_thres_max = 3.5
        self.prob_hit_log = 0.85
        self.prob_miss_log = -0.4
        self.occ_prob_thres_log = 0.0
        self.visualize_free_area = True
        self._device = device
        self._eng = None
        self._grid = None
        self._made_res = 0

    def __del__(self):
        try:
            if self._eng is not None:
                self._eng.occgrid_destroy(self._grid)
        except Exception:
            pass
        self._grid = None

    # the engine, the grid handle and the parameter block of this call
    def _call(self):
        if self._eng is None:
            self._eng = get_engine(self._device)
        if self._grid is None:
            self._grid = self._eng.occgrid_create(self.resolution)
            self._made_res = int(self.resolution)
        elif self._made_res != int(self.resolution):
            self._eng.occgrid_reconstruct(self._grid, self.resolution)
            self._made_res = int(self.resolution)
        return self._eng, self._grid, self._eng.occgrid_params(
            self.voxel_size, self.origin, self.clamping_thres_min, self.clamping_thres_max, self.prob_hit_log,
            self.prob_miss_log, self.occ_prob_thres_log)

    def clear(self):
        """every voxel unknown, the bounds back to the centre; size and memory stay"""
        if self._grid is not None and self._made_res == int(self.resolution):
            self._eng.occgrid_reset(self._grid)
        return self

    def reconstruct(self, voxel_size, resolution):
        self.voxel_size = float(np.float32(voxel_size))
        self.resolution = int(resolution)
        if self._grid is not None:
            self._eng.occgrid_reconstruct(self._grid, self.resolution)
            self._made_res = self.resolution
        return self

    def insert(self, pointcloud, viewpoint, max_range=-1.0):
        """Insert(points | PointCloud, viewpoint, max_range)"""
        pts = pointcloud.points.tensor if isinstance(pointcloud, PointCloud) else (
            pointcloud.tensor if isinstance(pointcloud, utility.Vector3fVector) else pointcloud)
        e, g, p = self._call()
        e.occgrid_insert(g, p, pts, viewpoint, max_range)
        return self

    def add_voxel(self, voxel, occupied=False):
        return self.add_voxels(np.asarray(voxel, np.int32).reshape(1, 3), occupied)

    def add_voxels(self, voxels, occupied=False):
        e, g, p = self._call()
        e.occgrid_add_voxels(g, p, voxels, occupied)
        return self

    def set_free_area(self, min_bound, max_bound):
        e, g, p = self._call()
        e.occgrid_set_free_area(g, p, min_bound, max_bound)
        return self

    # ---- queries
    def get_prob_log(self, points):
        """batched: [n, 3] points -> [n] log-odds on the device, NaN for unknown or outside the grid"""
        e, g, p = self._call()
        return e.occgrid_query(g, p, points)[0]

    def get_voxel(self, point):
        """-> (known, OccupancyVoxel)"""
        e, g, p = self._call()
        prob, idx = e.occgrid_query(g, p, np.asarray(point, np.float32).reshape(1, 3))
        v = float(prob[0])
        if v != v:
            return False, OccupancyVoxel()
        return True, OccupancyVoxel(idx[0].cpu().numpy(), v)

    def is_occupied(self, point):
        known, v = self.get_voxel(point)
        return known and v.prob_log > float(np.float32(self.occ_prob_thres_log))

    def is_unknown(self, point):
        return not self.get_voxel(point)[0]

    # ---- extraction
    def _extract(self, which):
        e, g, p = self._call()
        idx, prob, _ = e.occgrid_extract(g, p, which)
        return OccupancyVoxels(idx, prob)

    def extract_known_voxels(self):
        return self._extract(self.KNOWN)

    def extract_free_voxels(self):
        return self._extract(self.FREE)

    def extract_occupied_voxels(self):
        return self._extract(self.OCCUPIED)

    @property
    def voxels(self):
        return self.extract_known_voxels()

    def has_voxels(self):
        return True

    def has_colors(self):
        return True

    def __repr__(self):
        e, g, p = self._call()
        return "geometry::OccupancyGrid with %d voxels." % e.occgrid_count(g, p, self.KNOWN)

    # ---- bounds (voxel indices, inclusive) and GeometryBase3D
    @property
    def min_bound(self):
        e, g, _ = self._call()
        return e.occgrid_get_bounds(g)[0]

    @property
    def max_bound(self):
        e, g, _ = self._call()
        return e.occgrid_get_bounds(g)[1]

    def get_min_bound(self):
        h = int(self.resolution) // 2
        return ((self.min_bound - h).astype(np.float32) * np.float32(self.voxel_size) + np.asarray(self.origin, np.float32)).astype(np.float32)

    def get_max_bound(self):
        h = int(self.resolution) // 2
        return ((self.max_bound - (h - 1)).astype(np.float32) * np.float32(self.voxel_size) + np.asarray(self.origin, np.float32)).astype(np.float32)

    def get_center(self):
        return np.asarray(self.origin, np.float32).copy()

    def get_axis_aligned_bounding_box(self):
        return AxisAlignedBoundingBox(self.get_min_bound(), self.get_max_bound())

    def is_empty(self):
        return False

    def translate(self, translation, relative=True):
        t = np.asarray(translation, np.float32).reshape(3)
        self.origin = (np.asarray(self.origin, np.float32) + t).astype(np.float32) if relative else t.copy()
        return self

    def scale(self, scale, center=True):
        self.voxel_size = float(np.float32(self.voxel_size) * np.float32(scale))
        return self

    def transform(self, transformation):
        raise RuntimeError("OccupancyGrid::Transform is not supported")

    def rotate(self, R, center=True):
        raise RuntimeError("OccupancyGrid::Rotate is not supported")

    def get_voxels(self):
        """the whole log-odds plane, [resolution^3] on the device, indexed (x*res + y)*res + z; NaN: unknown"""
        e, g, _ = self._call()
        return e.occgrid_get_voxels(g, int(self.resolution) ** 3)


def _create_from_occupancy_grid(occgrid):
    """PointCloud::CreateFromOccupancyGrid (pointcloud_factory.cu:418-430): the occupied voxels' centres, all blue"""
    e, g, p = occgrid._call()
    _, _, xyz = e.occgrid_extract(g, p, OccupancyGrid.OCCUPIED, want_points=True)
    out = PointCloud()
    out._points = utility.Vector3fVector(xyz)
    col = torch.zeros_like(xyz)
    col[:, 2] = 1.0
    out._colors = utility.Vector3fVector(col)
    return out


PointCloud.create_from_occupancy_grid = staticmethod(_create_from_occupancy_grid)


class Voxel:
    """geometry::Voxel (voxelgrid.h:48-62): grid index and colour.  Voxel(), Voxel(grid_index), Voxel(color=...),
    Voxel(grid_index, color) are the reference's four constructors."""

    def __init__(self, grid_index=(0, 0, 0), color=(1.0, 1.0, 1.0)):
        self.grid_index = np.asarray(grid_index, np.int32).reshape(3).copy()
        self.color = np.asarray(color, np.float32).reshape(3).copy()

    def __repr__(self):
        g, c = self.grid_index, self.color
        return "geometry::Voxel with grid_index: (%d, %d, %d), color: (%g, %g, %g)" % (g[0], g[1], g[2], c[0], c[1], c[2])


class DeviceVoxelMap:
    """what VoxelGrid.voxels gives and takes: grid_index [m, 3] int32 and color [m, 3] float32, device tensors (numpy
    arrays are uploaded when the map is assigned).  len(), [] (a Voxel) and cpu()."""

    def __init__(self, grid_index=None, color=None):
        self.grid_index = grid_index
        self.color = color

    def __len__(self):
        return 0 if self.grid_index is None else int(self.grid_index.shape[0])

    def __getitem__(self, i):
        return Voxel(self.grid_index[i].cpu().numpy(), self.color[i].cpu().numpy())

    def cpu(self):
        """-> (grid_index, color) as numpy arrays"""
        if self.grid_index is None:
            return np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32)
        to = lambda a: a.cpu().numpy() if (torch is not None and torch.is_tensor(a)) else np.asarray(a)
        return to(self.grid_index).astype(np.int32).reshape(-1, 3), to(self.color).astype(np.float32).reshape(-1, 3)


def _floor_index(v):
    """floor(.) of fp32 values as int32, held inside +-1e9 first (the rule of include/mi_icp.h)"""
    return np.clip(np.floor(v), np.float32(-1.0e9), np.float32(1.0e9)).astype(np.int32)


def _index_list(indices):
    """a ULongVector, a tensor or anything numpy takes -> what the engine uploads as int64"""
    indices = getattr(indices, "tensor", indices)
    return indices if (torch is not None and torch.is_tensor(indices)) else np.asarray(indices, np.int64)


def _round_count(extent, voxel_size):
    """int(std::round(extent / voxel_size)) in fp32: halves away from zero"""
    q = float(np.float32(extent) / np.float32(voxel_size))
    return int(np.floor(q + 0.5)) if q >= 0.0 else -int(np.floor(-q + 0.5))


class VoxelGrid:
    """geometry::VoxelGrid (voxelgrid.h:84-214): voxel_size, origin and the voxels as two device tensors, keys int32
    [m, 3] and colours float32 [m, 3].  Every factory and +, += leave the keys distinct and ascending (x most significant).
    Deviations from the reference: DESIGN.md section 6."""

    def __init__(self, other=None, device=None):
        self.voxel_size = 0.0
        self.origin = np.zeros(3, np.float32)
        self._keys = None
        self._colors = None
        self._sorted = True
        self._device = device
        if other is not None:   # the copy constructor
            self.voxel_size = float(other.voxel_size)
            self.origin = np.asarray(other.origin, np.float32).reshape(3).copy()
            self._device = other._device
            self._sorted = other._sorted
            if other._keys is not None:
                self._keys, self._colors = other._keys.clone(), other._colors.clone()

    # ---- plumbing
    def _eng(self):
        return get_engine(self._device)

    def _set(self, keys, colors, is_sorted):
        self._keys, self._colors, self._sorted = keys, colors, bool(is_sorted)
        return self

    def _like(self, keys, colors, is_sorted):
        out = VoxelGrid(device=self._device)
        out.voxel_size, out.origin = float(self.voxel_size), np.asarray(self.origin, np.float32).reshape(3).copy()
        return out._set(keys, colors, is_sorted)

    def __len__(self):
        return 0 if self._keys is None else int(self._keys.shape[0])

    def _arrays(self):
        """the keys and colours as device tensors (an empty grid: two [0, 3] tensors)"""
        if self._keys is None:
            e = self._eng()
            return e._vg_dev(np.zeros((0, 3), np.int32), np.int32), e._vg_dev(np.zeros((0, 3), np.float32), np.float32)
        return self._keys, self._colors

    # ---- the voxels
    @property
    def voxels(self):
        return DeviceVoxelMap(self._keys, self._colors)

    @voxels.setter
    def voxels(self, v):
        """a DeviceVoxelMap, a (grid_index, color) pair of arrays, or a list of Voxel; taken as given, in any order"""
        if isinstance(v, DeviceVoxelMap):
            k, c = v.grid_index, v.color
        elif isinstance(v, (list, tuple)) and len(v) > 0 and isinstance(v[0], Voxel):
            k, c = np.stack([x.grid_index for x in v]), np.stack([x.color for x in v])
        elif isinstance(v, (list, tuple)) and len(v) == 2:
            k, c = v
        else:
            k, c = None, None
        if k is None or len(k) == 0:
            self._set(None, None, True)
            return
        e = self._eng()
        k, c = e._vg_dev(k, np.int32), e._vg_dev(c, np.float32)
        if int(k.shape[0]) != int(c.shape[0]):
            raise ValueError("VoxelGrid.voxels: %d keys, %d colours" % (int(k.shape[0]), int(c.shape[0])))
        self._set(k, c, False)

    def get_voxels(self):
        return self.voxels

    def set_voxels(self, voxels_keys, voxels_values=None):
        self.voxels = voxels_keys if voxels_values is None else (voxels_keys, voxels_values)

    def clear(self):
        self.voxel_size = 0.0
        self.origin = np.zeros(3, np.float32)
        self._set(None, None, True)
        return self

    def is_empty(self):
        return len(self) == 0

    def has_voxels(self):
        return len(self) > 0

    def has_colors(self):
        return True   # (the reference: by default the colours are (1, 1, 1))

    def __repr__(self):
        return "geometry::VoxelGrid with %d voxels." % len(self)

    # ---- GeometryBase3D
    def _index_bounds(self):
        return self._eng().voxelgrid_bounds(self._keys, self.voxel_size, self.origin)

    def get_min_bound(self):
        o = np.asarray(self.origin, np.float32).reshape(3)
        if self.is_empty():
            return o.copy()
        lo, _, _ = self._index_bounds()
        return (lo.astype(np.float32) * np.float32(self.voxel_size) + o).astype(np.float32)

    def get_max_bound(self):
        o = np.asarray(self.origin, np.float32).reshape(3)
        if self.is_empty():
            return o.copy()
        _, hi, _ = self._index_bounds()
        return ((hi.astype(np.float32) + np.float32(1.0)) * np.float32(self.voxel_size) + o).astype(np.float32)

    def get_center(self):
        if self.is_empty():
            return np.zeros(3, np.float32)
        _, _, s = self._index_bounds()
        return (s / float(len(self))).astype(np.float32)

    def get_axis_aligned_bounding_box(self):
        return AxisAlignedBoundingBox(self.get_min_bound(), self.get_max_bound())

    def translate(self, translation, relative=True):
        self.origin = (np.asarray(self.origin, np.float32).reshape(3) + np.asarray(translation, np.float32).reshape(3)).astype(np.float32)
        return self

    def scale(self, scale, center=True):
        self.voxel_size = float(np.float32(self.voxel_size) * np.float32(scale))
        return self

    def transform(self, transformation):
        raise RuntimeError("VoxelGrid::Transform is not supported")

    def rotate(self, R, center=True):
        raise RuntimeError("VoxelGrid::Rotate is not supported")

    # ---- merging
    def _merge(self, keys, colors, mode):
        ka, ca = self._arrays()
        k, c = self._eng().voxelgrid_merge(ka, ca, keys, colors, mode)
        return self._set(k, c, True) if int(k.shape[0]) else self._set(None, None, True)

    def __iadd__(self, other):
        if float(np.float32(self.voxel_size)) != float(np.float32(other.voxel_size)):
            raise RuntimeError("[VoxelGrid] Could not combine VoxelGrid because voxel_size differs (this=%f, other=%f)"
                               % (self.voxel_size, other.voxel_size))
        a, b = np.asarray(self.origin, np.float32).reshape(3), np.asarray(other.origin, np.float32).reshape(3)
        if not np.array_equal(a, b):
            raise RuntimeError("[VoxelGrid] Could not combine VoxelGrid because origin differs (this=%f,%f,%f, other=%f,%f,%f)"
                               % (a[0], a[1], a[2], b[0], b[1], b[2]))
        kb, cb = other._arrays()
        return self._merge(kb, cb, Engine.VOXELGRID_AVERAGE)

    def __add__(self, other):
        out = VoxelGrid(self)
        out += other
        return out

    def add_voxel(self, voxel):
        return self.add_voxels([voxel])

    def add_voxels(self, voxels):
        """a list of Voxel, a DeviceVoxelMap or a (grid_index, color) pair: an existing voxel stays as it is, and among
        added voxels of one index the first listed stays"""
        if isinstance(voxels, DeviceVoxelMap):
            k, c = voxels.grid_index, voxels.color
        elif isinstance(voxels, (list, tuple)) and len(voxels) > 0 and isinstance(voxels[0], Voxel):
            k, c = np.stack([x.grid_index for x in voxels]), np.stack([x.color for x in voxels])
        elif len(voxels) == 0:
            return self
        else:
            k, c = voxels
        e = self._eng()
        return self._merge(e._vg_dev(k, np.int32), e._vg_dev(c, np.float32), Engine.VOXELGRID_KEEP_FIRST)

    # ---- single voxels (host arithmetic in fp32, as the reference's host code)
    def get_voxel(self, point):
        p = np.asarray(point, np.float32).reshape(3)
        with np.errstate(all="ignore"):
            return _floor_index((p - np.asarray(self.origin, np.float32).reshape(3)) / np.float32(self.voxel_size))

    def _has_index(self, idx):
        """is the voxel `idx` in the grid?  (the query kernel on the unit grid: idx + 0.5 is exact below 2^22)"""
        idx = np.asarray(idx, np.int32).reshape(3)
        if self.is_empty():
            return False
        if np.abs(idx.astype(np.int64)).max() >= (1 << 22):
            raise ValueError("VoxelGrid: a single-voxel lookup takes indices below 2^22")
        q = (idx.astype(np.float32) + np.float32(0.5)).reshape(1, 3)
        inc, _ = self._eng().voxelgrid_query(self._keys, 1.0, (0.0, 0.0, 0.0), q, keys_sorted=self._sorted)
        return bool(int(inc[0]))

    def get_voxel_center_coordinate(self, idx):
        idx = np.asarray(idx, np.int32).reshape(3)
        if not self._has_index(idx):
            return np.zeros(3, np.float32)
        return ((idx.astype(np.float32) + np.float32(0.5)) * np.float32(self.voxel_size)
                + np.asarray(self.origin, np.float32).reshape(3)).astype(np.float32)

    def get_voxel_bounding_points(self, index):
        r = np.float32(np.float32(self.voxel_size) / np.float32(2.0))
        x = self.get_voxel_center_coordinate(index)
        signs = [(-1, -1, -1), (-1, -1, 1), (1, -1, -1), (1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, 1, -1), (1, 1, 1)]
        return [(x + np.asarray(sg, np.float32) * r).astype(np.float32) for sg in signs]

    # ---- batched operations
    def check_if_included(self, queries):
        """[nq, 3] points (numpy, a Vector3fVector or a tensor) -> numpy bool [nq]"""
        q = queries.tensor if isinstance(queries, utility.Vector3fVector) else queries
        k, _ = self._arrays()
        inc, _ = self._eng().voxelgrid_query(k, self.voxel_size, self.origin, q, keys_sorted=self._sorted)
        return inc.cpu().numpy().astype(bool)

    def paint_uniform_color(self, color):
        if not self.is_empty():
            self._eng().voxelgrid_paint(self._colors, color)
        return self

    def paint_indexed_color(self, indices, color):
        k, c = self._arrays()
        self._eng().voxelgrid_paint(c, color, _index_list(indices))
        return self

    def select_by_index(self, indices, invert=False):
        k, c = self._arrays()
        ok, oc = self._eng().voxelgrid_select_by_index(k, c, _index_list(indices), invert)
        return self._like(ok, oc, False) if int(ok.shape[0]) else self._like(None, None, True)

    def _carve(self, image, camera_params, keep_voxels_outside_image, what):
        img = _img(image)
        intr = camera_params.intrinsic
        if int(img.shape[0]) != int(intr.height) or int(img.shape[1]) != int(intr.width):
            raise RuntimeError("[VoxelGrid] provided %s dimensions are not compatible with the provided camera_parameters" % what)
        if self.is_empty():
            return self
        k, c = self._eng().voxelgrid_carve(self._keys, self._colors, self.voxel_size, self.origin, img, intr.as4(),
                                           camera_params.extrinsic, keep_voxels_outside_image)
        return self._set(k, c, self._sorted) if int(k.shape[0]) else self._set(None, None, True)

    def carve_depth_map(self, depth_map, camera_params, keep_voxels_outside_image=False):
        return self._carve(depth_map, camera_params, keep_voxels_outside_image, "depth_map")

    def carve_silhouette(self, silhouette_mask, camera_params, keep_voxels_outside_image=False):
        return self._carve(silhouette_mask, camera_params, keep_voxels_outside_image, "silhouette_mask")

    # ---- factories
    @staticmethod
    def create_dense(origin, voxel_size, width, height, depth, device=None):
        out = VoxelGrid(device=device)
        out.origin = np.asarray(origin, np.float32).reshape(3).copy()
        out.voxel_size = float(np.float32(voxel_size))
        nw, nh, nd = (_round_count(x, voxel_size) for x in (width, height, depth))
        k, c = out._eng().voxelgrid_dense(nw, nh, nd)
        return out._set(k, c, True) if int(k.shape[0]) else out

    @staticmethod
    def create_from_point_cloud_within_bounds(input, voxel_size, min_bound, max_bound):
        pts = input.points.tensor if input.has_points() else None
        out = VoxelGrid(device=None if pts is None else pts.device.index)
        lo = np.asarray(min_bound, np.float32).reshape(3)
        out.voxel_size, out.origin = float(np.float32(voxel_size)), lo.copy()
        if pts is None:
            pts = np.zeros((0, 3), np.float32)
        col = input.colors.tensor if input.has_colors() else None
        k, c = out._eng().voxelgrid_from_points(pts, voxel_size, lo, max_bound, col)
        return out._set(k, c, True) if int(k.shape[0]) else out

    @staticmethod
    def create_from_point_cloud(input, voxel_size):
        half = np.float32(voxel_size) * np.float32(0.5)
        lo = (np.asarray(input.get_min_bound(), np.float32) - half).astype(np.float32)
        hi = (np.asarray(input.get_max_bound(), np.float32) + half).astype(np.float32)
        return VoxelGrid.create_from_point_cloud_within_bounds(input, voxel_size, lo, hi)

    @staticmethod
    def create_from_occupancy_grid(input):
        """the occupied voxels of an OccupancyGrid, their grid indices as keys (ascending), every colour (0, 0, 1)"""
        if not (float(input.voxel_size) > 0.0):
            raise RuntimeError("[CreateFromOccupancyGrid] occupancy grid  voxel_size <= 0.")
        e, g, p = input._call()
        out = VoxelGrid(device=e.device)
        out.voxel_size, out.origin = float(np.float32(input.voxel_size)), np.asarray(input.origin, np.float32).reshape(3).copy()
        idx, _, _ = e.occgrid_extract(g, p, OccupancyGrid.OCCUPIED)
        if int(idx.shape[0]) == 0:
            return out
        idx = idx.contiguous()
        col = torch.empty((int(idx.shape[0]), 3), dtype=torch.float32, device=idx.device)
        e.voxelgrid_paint(col, (0.0, 0.0, 1.0))
        return out._set(idx, col, True)


def _log_error(msg):
    print("[cupoch_amd] Error: %s" % msg, file=sys.stderr)   # utility::LogError: logs, keeps going


class DistanceVoxel:
    """geometry::DistanceVoxel (distancetransform.h:30-49): the nearest site's grid index and the distance to it.
    Without a site the index is (-1, -1, -1) and the distance +inf."""

    def __init__(self, nearest_index=(0, 0, 0), distance=0.0):
        self.nearest_index = np.asarray(nearest_index, np.int32).reshape(3).copy()
        self.distance = float(np.float32(distance))

    def __repr__(self):
        g = self.nearest_index
        return "geometry::DistanceVoxel with nearest_index: (%d, %d, %d), distance: %g)" % (g[0], g[1], g[2], self.distance)


class DistanceVoxels:
    """the whole plane of a DistanceTransform: nearest_index [res^3, 3] int32 and distance [res^3] as device tensors,
    indexed (x*res + y)*res + z.  len() and [] give DistanceVoxel objects."""

    def __init__(self, nearest_index, distance):
        self.nearest_index = nearest_index
        self.distance = distance

    def __len__(self):
        return int(self.distance.shape[0])

    def __getitem__(self, i):
        return DistanceVoxel(self.nearest_index[i].cpu().numpy(), float(self.distance[i]))

    def cpu(self):
        """-> (nearest_index, distance) as numpy arrays"""
        return self.nearest_index.cpu().numpy(), self.distance.cpu().numpy()


class DistanceTransform:
    """geometry::DistanceTransform (distancetransform.h:51-78): the exact Euclidean distance from every cell of a dense
    resolution^3 grid to the nearest site.  The attributes are the reference's public members and are read when a call
    is made; the cells live on the GPU, made on first use (a changed `resolution` rebuilds the transform without sites,
    as reconstruct does).  Every compute replaces the site set.  Deviations from the reference: DESIGN.md section 6."""

    def __init__(self, voxel_size=0.05, resolution=512, origin=(0.0, 0.0, 0.0), device=None):
        self.voxel_size = float(np.float32(voxel_size))
        self.resolution = int(resolution)
        self.origin = np.asarray(origin, np.float32).reshape(3).copy()
        self.dropped = None     # cells outside the grid at the last compute with count_dropped=True
        self._device = device
        self._eng = None
        self._dt = None
        self._made_res = 0

    def __del__(self):
        try:
            if self._eng is not None:
                self._eng.dt_destroy(self._dt)
        except Exception:
            pass
        self._dt = None

    # the engine and the handle of this call
    def _call(self):
        if self._eng is None:
            self._eng = get_engine(self._device)
        if self._dt is None:
            self._dt = self._eng.dt_create(self.resolution)
            self._made_res = int(self.resolution)
        elif self._made_res != int(self.resolution):
            try:
                self._eng.dt_reconstruct(self._dt, self.resolution)
            except _lib.MiIcpError as e:
                if e.code == _lib.MI_ICP_ERR_HIP:      # the planes could not be made: the handle is gone
                    self._dt, self._made_res = None, 0
                raise                                   # (a refused resolution leaves the transform as it was)
            self._made_res = int(self.resolution)
        return self._eng, self._dt

    def clear(self):
        """no sites; size and memory stay (the reference's Clear() frees the voxels and zeroes the resolution)"""
        if self._dt is not None and self._made_res == int(self.resolution):
            self._eng.dt_compute_cells(self._dt, np.zeros((0, 3), np.int32))
        return self

    def reconstruct(self, voxel_size, resolution):
        self.voxel_size = float(np.float32(voxel_size))
        self.resolution = int(resolution)
        self._call()
        return self

    def compute_edt(self, x, count_dropped=False):
        """x: a VoxelGrid, an OccupancyGrid, or [n, 3] integer cells (tensor / array).  With count_dropped the number
        of cells that fell outside the grid is left in self.dropped (it costs the call a wait)."""
        if isinstance(x, VoxelGrid):
            if abs(float(np.float32(self.voxel_size)) - float(np.float32(x.voxel_size))) > float(np.finfo(np.float32).eps):
                _log_error("Unsupport computing Voronoi diagrams from different voxel size.")
                return self
            e, h = self._call()
            keys = x._keys if x._keys is not None else np.zeros((0, 3), np.int32)
            self.dropped = e.dt_compute_voxelgrid(h, self.voxel_size, self.origin, keys, x.voxel_size, x.origin, count_dropped)
        elif isinstance(x, OccupancyGrid):
            if int(x.resolution) != int(self.resolution):
                raise ValueError("DistanceTransform.compute_edt: the occupancy grid's resolution differs")
            e, h = self._call()
            e2, g, _ = x._call()
            if e2 is not e:
                raise ValueError("DistanceTransform.compute_edt: the occupancy grid lives on another device")
            e.dt_compute_occgrid(h, g, float(np.float32(x.occ_prob_thres_log)))
            self.dropped = 0 if count_dropped else None
        else:
            cells = getattr(x, "tensor", x)
            if not (torch is not None and torch.is_tensor(cells)):
                cells = np.asarray(cells)
                if cells.size and not np.issubdtype(cells.dtype, np.integer):
                    raise TypeError("DistanceTransform.compute_edt: cells must be integers")
                cells = cells.astype(np.int32).reshape(-1, 3)
            elif cells.is_floating_point():
                raise TypeError("DistanceTransform.compute_edt: cells must be integers")
            e, h = self._call()
            self.dropped = e.dt_compute_cells(h, cells, count_dropped)
        return self

    # the distance is derived from the nearest index, so the reference's two calls are one here
    compute_voronoi_diagram = compute_edt

    # ---- queries
    def get_distances(self, queries):
        """batched: [n, 3] points -> [n] distances on the device, NaN outside the grid, +inf without a site"""
        e, h = self._call()
        queries = queries.points.tensor if isinstance(queries, PointCloud) else getattr(queries, "tensor", queries)
        return e.dt_query(h, self.voxel_size, self.origin, queries)[0]

    def get_nearest_indices(self, queries):
        """batched: [n, 3] points -> (distance [n], nearest site [n, 3] int32), device tensors"""
        e, h = self._call()
        return e.dt_query(h, self.voxel_size, self.origin, getattr(queries, "tensor", queries))

    def get_distance(self, query):
        return float(self.get_distances(np.asarray(query, np.float32).reshape(1, 3))[0])

    def get_voxel(self, point):
        """-> (inside the grid, DistanceVoxel)"""
        dist, idx = self.get_nearest_indices(np.asarray(point, np.float32).reshape(1, 3))
        d = float(dist[0])
        if d != d:
            return False, DistanceVoxel()
        return True, DistanceVoxel(idx[0].cpu().numpy(), d)

    @property
    def voxels(self):
        """the whole plane (DistanceVoxels); 16 bytes per cell on the device"""
        e, h = self._call()
        return DistanceVoxels(*e.dt_get_voxels(h, self.voxel_size, int(self.resolution) ** 3))

    def get_nearest_index_plane(self):
        """[resolution^3, 3] int32 on the device, indexed (x*res + y)*res + z; -1 without a site"""
        e, h = self._call()
        return e.dt_get_voxels(h, self.voxel_size, int(self.resolution) ** 3, want_distance=False)[0]

    def get_distance_plane(self):
        """[resolution^3] float32 on the device, indexed (x*res + y)*res + z; +inf without a site"""
        e, h = self._call()
        return e.dt_get_voxels(h, self.voxel_size, int(self.resolution) ** 3, want_nearest=False)[1]

    def has_voxels(self):
        return True

    def __repr__(self):
        return "geometry::DistanceTransform with %d resolution." % int(self.resolution)

    # ---- DenseGrid / GeometryBase3D (densegrid.inl:53-125)
    def get_min_bound(self):
        length = np.float32(np.float32(self.voxel_size) * np.float32(self.resolution)) * np.float32(0.5)
        return (np.asarray(self.origin, np.float32) - length).astype(np.float32)

    def get_max_bound(self):
        length = np.float32(np.float32(self.voxel_size) * np.float32(self.resolution)) * np.float32(0.5)
        return (np.asarray(self.origin, np.float32) + length).astype(np.float32)

    def get_center(self):
        return np.asarray(self.origin, np.float32).copy()

    def get_axis_aligned_bounding_box(self):
        return AxisAlignedBoundingBox(self.get_min_bound(), self.get_max_bound())

    def is_empty(self):
        return False

    def translate(self, translation, relative=True):
        t = np.asarray(translation, np.float32).reshape(3)
        self.origin = (np.asarray(self.origin, np.float32) + t).astype(np.float32) if relative else t.copy()
        return self

    def scale(self, scale, center=True):
        self.voxel_size = float(np.float32(self.voxel_size) * np.float32(scale))
        return self

    def transform(self, transformation):
        _log_error("DenseGrid::Transform is not supported")
        return self

    def rotate(self, R, center=True):
        _log_error("DenseGrid::Rotate is not supported")
        return self

    @staticmethod
    def create_from_occupancy_grid(input):
        """the COMPUTED transform of the occupied voxels of an OccupancyGrid, with its voxel_size, resolution and origin"""
        if not (float(input.voxel_size) > 0.0):
            _log_error("[CreateOccupancyGrid] occupancy grid  voxel_size <= 0.")
        out = DistanceTransform(input.voxel_size, input.resolution, input.origin, device=input._call()[0].device)
        return out.compute_edt(input)


class LineSet:
    """geometry::LineSet<3> (lineset.h): points float32 [n, 3], lines int32 [l, 2] (point indices) and optional colours
    float32 [l, 3], one per line, as device vectors.  The bounds and the moves are the point cloud's, through the same
    entry points."""

    def __init__(self, points=None, lines=None):
        self._points = utility.Vector3fVector() if points is None else _v3(points)
        self._lines = utility.Vector2iVector() if lines is None else _v2i(lines)
        self._colors = None

    @property
    def points(self):
        return self._points

    @points.setter
    def points(self, v):
        self._points = _v3(v)

    @property
    def lines(self):
        return self._lines

    @lines.setter
    def lines(self, v):
        self._lines = _v2i(v)

    @property
    def colors(self):
        return self._colors if self._colors is not None else utility.Vector3fVector()

    @colors.setter
    def colors(self, v):
        self._colors = _v3(v)

    def has_points(self):
        return len(self._points) > 0

    def has_lines(self):
        return self.has_points() and len(self._lines) > 0

    def has_colors(self):
        return self.has_lines() and self._colors is not None and len(self._colors) == len(self._lines)

    def is_empty(self):
        return not self.has_points()

    def clear(self):
        self._points, self._lines, self._colors = utility.Vector3fVector(), utility.Vector2iVector(), None
        return self

    def __repr__(self):
        return "geometry::LineSet with %d lines." % len(self._lines)

    def _engine(self):
        return get_engine(self._points.tensor.device.index if self._points.tensor.is_cuda else None)

    def _bounds(self):
        return self._engine().compute_bounds(self._points.tensor)

    def get_min_bound(self):
        return self._bounds()[0]

    def get_max_bound(self):
        return self._bounds()[1]

    def get_center(self):
        return self._bounds()[2]

    def get_axis_aligned_bounding_box(self):
        mn, mx, _ = self._bounds()
        return AxisAlignedBoundingBox(mn, mx)

    def get_line_coordinate(self, line_index):
        """-> the two end points of a line (numpy [3] each); zeros for an index, of the line or of a point, that is out
        of range, as the C++ surface gives"""
        i = int(line_index)
        zero = np.zeros(3, np.float32)
        if not 0 <= i < len(self._lines):
            return zero, zero.copy()
        a, b = [int(v) for v in self._lines.tensor[i].cpu().numpy()]
        if not (0 <= a < len(self._points) and 0 <= b < len(self._points)):
            return zero, zero.copy()
        p = self._points.tensor[[a, b]].cpu().numpy()
        return p[0], p[1]

    def paint_uniform_color(self, color):
        c = np.asarray(color, np.float32).reshape(1, 3)
        self._colors = utility.Vector3fVector(np.repeat(c, len(self._lines), axis=0))
        return self

    def translate(self, translation, relative=True):
        t = np.asarray(translation, np.float32).reshape(3)
        if not relative:
            t = (t - self.get_center()).astype(np.float32)
        self._engine().affine(self._points.tensor, translate=t)
        return self

    def scale(self, scale, center=True):
        c = self.get_center() if center and len(self._points) else None
        self._engine().affine(self._points.tensor, scale=float(scale), center=c)
        return self

    def rotate(self, R, center=True):
        c = self.get_center() if center and len(self._points) else None
        self._engine().affine(self._points.tensor, R=np.asarray(R, np.float32).reshape(3, 3), center=c)
        return self

    def transform(self, transformation):
        self._engine().transform(np.asarray(transformation, np.float32), self._points.tensor, None, None)
        return self

    _BOX_LINES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))

    @staticmethod
    def create_from_axis_aligned_bounding_box(box):
        """the twelve edges of a box: corners in the order (x, y, z) = (min|max) with x fastest on each z face"""
        lo, hi = np.asarray(box.get_min_bound(), np.float32), np.asarray(box.get_max_bound(), np.float32)
        corners = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]],
                            [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32)
        return LineSet(corners, np.array(LineSet._BOX_LINES, np.int32))


def _v3(v):
    return v if isinstance(v, utility.Vector3fVector) else utility.Vector3fVector(v)


def _v2i(v):
    return v if isinstance(v, utility.Vector2iVector) else utility.Vector2iVector(v)


def _t2i(eng, edges):
    """edges as an int32 [k, 2] tensor on the engine's GPU"""
    if isinstance(edges, utility.DeviceVector):
        edges = edges.tensor
    return eng._vg_dev(edges, np.int32, 2)


class Graph(LineSet):
    """geometry::Graph<3> (graph.h): a LineSet whose lines are directed edges, with one weight per edge and, once
    constructed, the lines sorted by (first, second) and a CSR offset per node.  An undirected graph (is_directed =
    False, the default) holds both directions of every edge.  The contract is in include/mi_icp.h ("graph"): the sort,
    the lattice, the weight and removal updates and the shortest-path search run on the GPU through the
    mi_icp_graph_* family.  Not built: Graph2D, create_from_triangle_mesh, visualisation, file I/O.  Deviations from
    the reference: DESIGN.md section 6."""

    def __init__(self, points=None):
        if isinstance(points, Graph):
            other = points
            LineSet.__init__(self, other._points.tensor.clone(), other._lines.tensor.clone())
            self._colors = None if other._colors is None else utility.Vector3fVector(other._colors.tensor.clone())
            self._weights = None if other._weights is None else other._weights.clone()
            self._offsets = None if other._offsets is None else other._offsets.clone()
            self._node_colors = None if other._node_colors is None else utility.Vector3fVector(other._node_colors.tensor.clone())
            self._sorted, self.is_directed = other._sorted, other.is_directed
            return
        LineSet.__init__(self, points, None)
        self._weights = None          # float32 [m] on the device
        self._offsets = None          # int32 [n + 1] on the device
        self._node_colors = None
        self._sorted = False          # the lines are as construct_graph left them
        self.is_directed = False

    def clone(self):
        return Graph(self)

    # ---- members
    @property
    def lines(self):
        return self._lines

    @lines.setter
    def lines(self, v):
        self._lines = _v2i(v)
        self._sorted = False

    edges = lines

    @property
    def edge_weights(self):
        return self._weights if self._weights is not None else self._engine()._vg_dev(np.zeros(0, np.float32), np.float32, 1)

    @edge_weights.setter
    def edge_weights(self, v):
        self._weights = self._engine()._vg_dev(v, np.float32, 1)

    @property
    def edge_index_offsets(self):
        return self._offsets if self._offsets is not None else self._engine()._vg_dev(np.zeros(0, np.int32), np.int32, 1)

    @edge_index_offsets.setter
    def edge_index_offsets(self, v):
        self._offsets = self._engine()._vg_dev(v, np.int32, 1)

    @property
    def node_colors(self):
        return self._node_colors if self._node_colors is not None else utility.Vector3fVector()

    @node_colors.setter
    def node_colors(self, v):
        self._node_colors = _v3(v)

    def has_weights(self):
        return self.has_lines() and self._weights is not None and int(self._weights.shape[0]) == len(self._lines)

    def has_node_colors(self):
        return self.has_points() and self._node_colors is not None and len(self._node_colors) == len(self._points)

    def is_constructed(self):
        return self._sorted and self._offsets is not None and int(self._offsets.shape[0]) == len(self._points) + 1

    def clear(self):
        LineSet.clear(self)
        self._weights = self._offsets = self._node_colors = None
        self._sorted = False
        return self

    def __repr__(self):
        return "geometry::Graph with %d nodes and %d edges." % (len(self._points), len(self._lines))

    def _m(self):
        return len(self._lines)

    def _fill_weights(self):
        """every line has a weight: missing ones are 1.0 (the reference's resize)"""
        m = self._m()
        have = 0 if self._weights is None else int(self._weights.shape[0])
        if have != m:
            w = torch.ones(m, dtype=torch.float32, device=self._lines.tensor.device)
            if have:
                w[:min(have, m)] = self._weights[:min(have, m)]
            self._weights = w

    # ---- ConstructGraph and the weights
    def construct_graph(self, set_edge_weights_from_distance=True):
        if self._m() == 0:
            _log_error("[ConstructGraph] Graph has no edges.")
            return self
        self._fill_weights()
        col = self._colors.tensor if self.has_colors() else None
        self._offsets = self._engine().graph_construct(self._lines.tensor, len(self._points), self._weights, col)
        self._sorted = True
        if set_edge_weights_from_distance:
            self.set_edge_weights_from_distance()
        return self

    def set_edge_weights_from_distance(self):
        self._weights = self._engine().graph_weights_from_distance(self._points.tensor, self._lines.tensor)
        return self

    def set_edge_weights(self, edges, weight):
        """every line equal to a listed edge (undirected: or to its reverse) gets `weight`"""
        if self._m() == 0:
            return self
        if not self.is_constructed():
            self.construct_graph(False)
        self._fill_weights()
        eng = self._engine()
        e = _t2i(eng, edges)
        if int(e.shape[0]):
            eng.graph_set_edge_weights(self._lines.tensor, self._weights, e, weight, self.is_directed)
            eng.synchronize()    # (an uploaded list may go)
        return self

    # ---- edges in and out
    def add_edges(self, edges, weights=None, lazy_add=False):
        eng = self._engine()
        e = _t2i(eng, edges)
        k = int(e.shape[0])
        if weights is not None:
            w = eng._vg_dev(weights.tensor if isinstance(weights, utility.DeviceVector) else weights, np.float32, 1)
            if int(w.shape[0]) == 0:
                w = None
            elif int(w.shape[0]) != k:
                _log_error("[AddEdges] edges size is not equal to weights size.")
                return self
        else:
            w = None
        if w is None:
            w = torch.ones(k, dtype=torch.float32, device=e.device)   # (the reference's resize here is wrong: DESIGN section 6)
        self._fill_weights()
        had_colors = self.has_colors()
        new_l, new_w = (e, w) if self.is_directed else (torch.cat([e, e.flip(1)]), torch.cat([w, w]))
        old_w = self._weights if self._weights is not None else w[:0]
        self._lines = utility.Vector2iVector(torch.cat([self._lines.tensor, new_l]))
        self._weights = torch.cat([old_w, new_w])
        if had_colors:
            ones = torch.ones((int(new_l.shape[0]), 3), dtype=torch.float32, device=e.device)
            self._colors = utility.Vector3fVector(torch.cat([self._colors.tensor, ones]))
        self._sorted = False
        return self if lazy_add else self.construct_graph(False)

    def add_edge(self, edge, weight=1.0, lazy_add=False):
        return self.add_edges(np.asarray(edge, np.int32).reshape(1, 2), np.array([weight], np.float32), lazy_add)

    def remove_edges(self, edges):
        if self._m() == 0:
            return self
        if not self.is_constructed():
            self.construct_graph(False)
        self._fill_weights()
        eng = self._engine()
        col = self._colors.tensor if self.has_colors() else None
        m, off = eng.graph_remove_edges(self._lines.tensor, len(self._points), _t2i(eng, edges), self.is_directed,
                                        self._weights, col)
        self._lines = utility.Vector2iVector(self._lines.tensor[:m])
        self._weights = self._weights[:m]
        if col is not None:
            self._colors = utility.Vector3fVector(col[:m])
        self._offsets = off
        return self

    def remove_edge(self, edge):
        return self.remove_edges(np.asarray(edge, np.int32).reshape(1, 2))

    def connect_to_nearest_neighbors(self, max_edge_distance, max_num_edges=30):
        """ConnectToNearestNeighbors: every node to its max_num_edges nearest nodes within max_edge_distance (a radius
        search of max_num_edges + 1, the node itself among them); the weight is the distance; undirected: the reverse
        of every new edge too; an edge already there is not added again."""
        n = len(self._points)
        if n == 0:
            return self
        knn = int(max_num_edges) + 1
        if not 1 <= knn <= 100:
            raise ValueError("connect_to_nearest_neighbors: max_num_edges + 1 must be in [1, 100]")
        eng = self._engine()
        pts = self._points.tensor
        found, idx, _ = KDTreeFlann(self._points).search_radius(pts, float(max_edge_distance), knn)   # (a tree of its own)
        if found < 0:
            return self
        i = torch.arange(n, device=pts.device, dtype=torch.int64).reshape(n, 1).expand(n, knn)
        j = idx.to(torch.int64)
        keep = (j >= 0) & (j != i)
        key = i[keep] * n + j[keep]
        if not self.is_directed:
            key = torch.cat([key, j[keep] * n + i[keep]])
        key = torch.unique(key)
        if self._m():
            have = self._lines.tensor.to(torch.int64)
            key = key[~torch.isin(key, have[:, 0] * n + have[:, 1])]
        new = torch.stack([key // n, key % n], dim=1).to(torch.int32).contiguous()
        self._fill_weights()
        had_colors = self.has_colors()
        old_w = self._weights if self._weights is not None else torch.zeros(0, dtype=torch.float32, device=pts.device)
        self._lines = utility.Vector2iVector(torch.cat([self._lines.tensor, new]))
        self._weights = torch.cat([old_w, eng.graph_weights_from_distance(pts, new)])
        if had_colors:
            ones = torch.ones((int(new.shape[0]), 3), dtype=torch.float32, device=pts.device)
            self._colors = utility.Vector3fVector(torch.cat([self._colors.tensor, ones]))
        self._sorted = False
        return self.construct_graph(False)

    def add_node_and_connect(self, point, max_edge_distance=0.0, lazy_add=False):
        """AddNodeAndConnect: the new node n gets an edge (i, n) from every node i strictly nearer than
        max_edge_distance (and (n, i) when undirected), weighted by that distance"""
        eng = self._engine()
        q = np.asarray(point, np.float32).reshape(3)
        pts = self._points.tensor
        n = int(pts.shape[0])
        qt = torch.from_numpy(q.copy()).to(pts.device).reshape(1, 3) if n else eng._vg_dev(q.reshape(1, 3), np.float32)
        if n:
            d = eng.graph_node_distances(pts, q)
            near = torch.nonzero(d < float(np.float32(max_edge_distance))).reshape(-1)
            edges = torch.stack([near.to(torch.int32), torch.full_like(near, n, dtype=torch.int32)], dim=1)
            w = d[near]
        else:
            edges, w = torch.zeros((0, 2), dtype=torch.int32, device=qt.device), torch.zeros(0, dtype=torch.float32, device=qt.device)
        self._points = utility.Vector3fVector(torch.cat([pts, qt]))
        if self._node_colors is not None:
            self._node_colors = None if not len(self._node_colors) else utility.Vector3fVector(
                torch.cat([self._node_colors.tensor, torch.ones((1, 3), dtype=torch.float32, device=qt.device)]))
        self._sorted = False
        if int(edges.shape[0]) == 0:
            return self if lazy_add or self._m() == 0 else self.construct_graph(False)
        return self.add_edges(edges, w, lazy_add)

    # ---- colours
    def _line_match(self, edges):
        eng = self._engine()
        e = _t2i(eng, edges).to(torch.int64)
        if not self.is_directed:
            e = torch.cat([e, e.flip(1)])
        l = self._lines.tensor.to(torch.int64)
        big = 1 << 32
        return torch.isin(l[:, 0] * big + l[:, 1], e[:, 0] * big + e[:, 1])

    def paint_edges_color(self, edges, color):
        if not self.has_colors():
            self._colors = utility.Vector3fVector(torch.ones((self._m(), 3), dtype=torch.float32, device=self._lines.tensor.device))
        c = torch.tensor(np.asarray(color, np.float32).reshape(3), device=self._lines.tensor.device)
        self._colors.tensor[self._line_match(edges)] = c
        return self

    def paint_edge_color(self, edge, color):
        return self.paint_edges_color(np.asarray(edge, np.int32).reshape(1, 2), color)

    def paint_nodes_color(self, nodes, color):
        """paints the listed nodes (the reference paints all of them: DESIGN section 6)"""
        dev = self._points.tensor.device
        if not self.has_node_colors():
            self._node_colors = utility.Vector3fVector(torch.ones((len(self._points), 3), dtype=torch.float32, device=dev))
        if isinstance(nodes, utility.DeviceVector):
            nodes = nodes.tensor
        idx = torch.as_tensor(np.asarray(nodes.cpu() if _is_torch(nodes) else nodes, np.int64).reshape(-1), device=dev)
        self._node_colors.tensor[idx] = torch.tensor(np.asarray(color, np.float32).reshape(3), device=dev)
        return self

    def paint_node_color(self, node, color):
        return self.paint_nodes_color([int(node)], color)

    # ---- the search
    def dijkstra_paths(self, start_node_index, end_node_index=-1, want_info=False):
        """-> (dist float32 [n], prev int32 [n]) on the device: include/mi_icp.h states both exactly"""
        n = len(self._points)
        if not self.is_constructed():
            _log_error("[DijkstraPath] this graph is not constructed.")
            dev = self._points.tensor.device
            return (torch.full((n,), float("inf"), dtype=torch.float32, device=dev),
                    torch.full((n,), -1, dtype=torch.int32, device=dev))
        self._fill_weights()
        return self._engine().graph_sssp(self._offsets, self._lines.tensor, self._weights, n, start_node_index,
                                         end_node_index, want_info)

    def dijkstra_path(self, start_node_index, end_node_index):
        """-> (node indices from start to end, length); ([], inf) when there is no path, ([start], 0.0) for start == end"""
        start, end = int(start_node_index), int(end_node_index)
        dist, prev = self.dijkstra_paths(start, end)
        prev, length = prev.cpu().numpy(), float(dist[end].item())
        if prev[end] < 0:
            return [], float("inf")
        nodes = [end]
        while nodes[-1] != start:
            nodes.append(int(prev[nodes[-1]]))
            if len(nodes) > len(prev):
                raise _lib.MiIcpError("dijkstra_path: the predecessors cycle")
        return nodes[::-1], length

    @staticmethod
    def create_from_axis_aligned_bounding_box(*args):
        """(bbox, resolutions) or (min_bound, max_bound, resolutions): a lattice of resolutions nodes, 26-connected,
        constructed, weighted by distance; steps = (max - min) / resolutions, so the last node is one step short of max"""
        if len(args) == 2:
            box, res = args
            lo, hi = box.get_min_bound(), box.get_max_bound()
        else:
            lo, hi, res = args
        out = Graph()
        p, l, w, o = out._engine().graph_lattice(lo, hi, res)
        out._points, out._lines = utility.Vector3fVector(p), utility.Vector2iVector(l)
        out._weights, out._offsets, out._sorted = w, o, True
        return out


def _is_torch(a):
    return torch is not None and isinstance(a, torch.Tensor)


# ---- geometry::LaserScanBuffer (geometry/laserscanbuffer.h; python surface cupoch_pybind/geometry/laserscanbuffer.cpp) ----
_QUARTER_TURN_X = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)   # exact -pi/2 about X


def _matmul4(a, b):
    """a*b in fp32, every element ((a0*b0 + a1*b1) + a2*b2) + a3*b3 (include/mi_icp.h "laserscan")"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.empty((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]) + a[r, 3] * b[3, c]
    return out


class LaserScanBuffer:
    """A ring of scans from a planar laser range-finder, each with the pose (origin) it was taken from.

    ranges / intensities live on the GPU as [num_max_scans, num_steps] torch tensors, the origins on the host as
    [num_max_scans, 4, 4]; include/mi_icp.h ("laserscan") states what every operation computes.  The ring: the newest
    scan goes to slot bottom % num_max_scans; a full ring overwrites its oldest scan and advances top; the live scans
    are slots top .. bottom - 1 (mod num_max_scans), oldest first.  A buffer has intensities when the first scan added
    to it while empty carried them.
    Defaults follow the reference's Python (num_max_scans=10) except min_angle, which is -pi here: the reference's
    binding says +pi, which with max_angle=+pi makes an empty angle range.
    As in the reference, errors are printed and the call returns (self, None or an empty result); nothing is raised."""

    def __init__(self, num_steps, num_max_scans=10, min_angle=-np.pi, max_angle=np.pi, device=None):
        self._num_steps = int(num_steps)
        self._num_max_scans = int(num_max_scans)
        self.min_angle = float(np.float32(min_angle))
        self.max_angle = float(np.float32(max_angle))
        self._device = device
        self.top_ = 0
        self.bottom_ = 0
        self._ranges = None          # [num_max_scans, num_steps], made with the first scan
        self._intensities = None
        self._origins = np.tile(np.eye(4, dtype=np.float32), (max(self._num_max_scans, 0), 1, 1))

    # ---- attributes of the reference's binding
    @property
    def num_steps(self):
        return self._num_steps

    @property
    def num_max_scans(self):
        return self._num_max_scans

    @property
    def num_scans(self):
        return self.bottom_ - self.top_

    @property
    def ranges(self):
        """the live scans, oldest first: a [num_scans * num_steps] device tensor (GetRanges keeps them on the host)"""
        return self._live(self._ranges)

    @property
    def intensities(self):
        return self._live(self._intensities)

    @property
    def origins(self):
        """the live scans' origins, oldest first: [num_scans, 4, 4] numpy"""
        return self._origins[self._slots()].copy()

    def _eng(self):
        if self._device is None:
            self._device = utility.default_device()
        return get_engine(self._device)

    def _slots(self):
        return [(self.top_ + k) % self._num_max_scans for k in range(self.num_scans)]

    def _live(self, store):
        if store is None or self.num_scans == 0:
            return self._eng()._vg_dev(np.zeros(0, np.float32), np.float32, 1)
        return store[self._slots()].reshape(-1)

    def _row(self, values):
        return self._eng()._vg_dev(values, np.float32, 1)

    @staticmethod
    def _size(v):
        if v is None:
            return 0
        return int(v.numel()) if _is_torch(v) else int(np.asarray(v).size)

    # ---- laserscanbuffer.h:67-73
    def has_intensities(self):
        return self._intensities is not None

    def get_angle_increment(self):
        with np.errstate(all="ignore"):
            return float((np.float32(self.max_angle) - np.float32(self.min_angle)) / np.float32(self._num_steps - 1))

    def is_full(self):
        return self.num_scans == self._num_max_scans

    def get_num_scans(self):
        return self.num_scans

    def is_empty(self):
        return self.bottom_ == self.top_

    def clear(self):
        self.top_ = self.bottom_ = 0
        self._ranges = self._intensities = None
        self._origins[:] = np.eye(4, dtype=np.float32)
        return self

    def get_ranges(self):
        """GetRanges: the live scans oldest first, on the host"""
        return self.ranges.cpu().numpy()

    def get_intensities(self):
        return self.intensities.cpu().numpy()

    def _unsupported(self, what):
        _log_error("LaserScanBuffer::%s is not supported" % what)
        return np.zeros(3, np.float32)

    def get_min_bound(self):
        return self._unsupported("GetMinBound")

    def get_max_bound(self):
        return self._unsupported("GetMaxBound")

    def get_center(self):
        return self._unsupported("GetCenter")

    def get_axis_aligned_bounding_box(self):
        self._unsupported("GetAxisAlignedBoundingBox")
        return AxisAlignedBoundingBox()

    # ---- AddRanges / Merge / Pop
    def add_ranges(self, ranges, transformation=None, intensities=None):
        n, ni = self._size(ranges), self._size(intensities)
        if n != self._num_steps or self._num_max_scans < 1:
            _log_error("[AddRanges] Invalid size of input ranges.")
            return self
        if self.has_intensities() and n != ni:
            _log_error("[AddRanges] Invalid size of intensities.")
            return self
        T = np.eye(4, dtype=np.float32) if transformation is None else np.asarray(transformation, np.float32).reshape(4, 4)
        row = self._row(ranges)
        if self._ranges is None:
            self._ranges = torch.full((self._num_max_scans, self._num_steps), float("nan"), dtype=torch.float32, device=row.device)
        if self.is_empty() and self._intensities is None and ni == n:
            self._intensities = torch.zeros_like(self._ranges)
        if self.is_full():
            self.top_ += 1
        slot = self.bottom_ % self._num_max_scans
        self._ranges[slot] = row
        if self._intensities is not None:
            self._intensities[slot] = self._row(intensities)
        self._origins[slot] = T
        self.bottom_ += 1
        return self

    def add_host_ranges(self, ranges, transformation=None, intensities=None):
        return self.add_ranges(ranges, transformation, intensities)

    def merge(self, other):
        if other.is_empty():
            _log_error("[Merge] Input buffer is empty.")
            return self
        if other.num_steps != self._num_steps:
            _log_error("[Merge] Input buffer has different num_steps.")
            return self
        if other.has_intensities() != self.has_intensities():
            _log_error("[Merge] Input buffer has different intensities.")
            return self
        if other.min_angle != self.min_angle or other.max_angle != self.max_angle:
            _log_error("[Merge] Input buffer has different angle range.")
            return self
        if other.num_scans + self.num_scans > self._num_max_scans:
            _log_error("[Merge] Buffer is full.")
            return self
        for s in other._slots():
            self.add_ranges(other._ranges[s], other._origins[s], None if other._intensities is None else other._intensities[s])
        return self

    def _pop_slot(self):
        if self.is_empty():
            _log_error("[PopRange] Buffer is empty.")
            return None
        slot = self.top_ % self._num_max_scans
        self.top_ += 1
        return slot

    def pop_one_scan(self):
        slot = self._pop_slot()
        if slot is None:
            return None
        out = LaserScanBuffer(self._num_steps, self._num_max_scans, self.min_angle, self.max_angle, self._device)
        out.add_ranges(self._ranges[slot], self._origins[slot], None if self._intensities is None else self._intensities[slot])
        return out

    def pop_host_one_scan(self):
        """-> (ranges, intensities) of the oldest scan as numpy arrays (intensities empty without them)"""
        slot = self._pop_slot()
        if slot is None:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        r = self._ranges[slot].cpu().numpy()
        return r, (np.zeros(0, np.float32) if self._intensities is None else self._intensities[slot].cpu().numpy())

    # ---- the filters: a new buffer that keeps origins, intensities, top and bottom
    def _like(self, new_ranges):
        out = LaserScanBuffer(self._num_steps, self._num_max_scans, self.min_angle, self.max_angle, self._device)
        out.top_, out.bottom_ = self.top_, self.bottom_
        out._ranges = new_ranges
        out._intensities = None if self._intensities is None else self._intensities.clone()
        out._origins = self._origins.copy()
        return out

    def range_filter(self, min_range, max_range):
        if max_range <= min_range:
            _log_error("[RangeFilter] Invalid parameter with min_range greater than max_range.")
        if self._ranges is None:
            return self._like(None)
        return self._like(self._eng().laserscan_range_filter(self._ranges, min_range, max_range))

    def scan_shadow_filter(self, min_angle, max_angle, window, neighbors=0, remove_shadow_start_point=False):
        if self._ranges is None:
            return self._like(None)
        return self._like(self._eng().laserscan_shadow_filter(self._ranges, self._num_steps, self.min_angle, self.max_angle,
                                                              min_angle, max_angle, window, neighbors,
                                                              remove_shadow_start_point))

    # ---- GeometryBase3D: the origins' arithmetic on the host, Scale on the ranges
    def transform(self, transformation):
        T = np.asarray(transformation, np.float32).reshape(4, 4)
        for s in range(self._num_max_scans):
            self._origins[s] = _matmul4(self._origins[s], T)
        return self

    def translate(self, translation, relative=True):
        t = np.asarray(translation, np.float32).reshape(3)
        self._origins[:, :3, 3] = self._origins[:, :3, 3] + t
        return self

    def rotate(self, R, center=True):
        R = np.asarray(R, np.float32).reshape(3, 3)
        for s in range(self._num_max_scans):
            a = self._origins[s, :3, :3].copy()
            for r in range(3):
                for c in range(3):
                    self._origins[s, r, c] = (a[r, 0] * R[0, c] + a[r, 1] * R[1, c]) + a[r, 2] * R[2, c]
        return self

    def scale(self, scale, center=True):
        if self._ranges is not None:
            self._eng().laserscan_scale(self._ranges, scale)
        return self

    # ---- the virtual lidars
    @staticmethod
    def _factory_check(what, low_name, angle_increment, low, high, min_range, max_range, min_angle, max_angle):
        msg = None
        if not angle_increment > 0.0:
            msg = "angle_increment must be positive."
        elif not low < high:
            msg = "%s must be smaller than %s." % (low_name, low_name.replace("min", "max"))
        elif not min_range < max_range:
            msg = "min_range must be smaller than max_range."
        elif not min_angle < max_angle:
            msg = "min_angle must be smaller than max_angle."
        if msg:
            _log_error("[LaserScanBuffer::%s] %s" % (what, msg))
        return msg is None

    @staticmethod
    def _from_bins(bins, device, low, high, divisions, min_angle, max_angle, left=None):
        steps = int(bins.shape[1])
        out = LaserScanBuffer(steps, max(50, divisions), min_angle, max_angle, device)
        out._ranges = torch.full((out._num_max_scans, steps), float("nan"), dtype=torch.float32, device=bins.device)
        out._ranges[:divisions] = bins
        lo, hi = np.float32(low), np.float32(high)
        for i in range(out._num_max_scans):
            O = np.eye(4, dtype=np.float32)
            O[2, 3] = lo + ((hi - lo) * np.float32(i)) / np.float32(divisions)
            out._origins[i] = O if left is None else _matmul4(left, O)
        out.bottom_ = divisions
        return out

    @staticmethod
    def create_from_point_cloud(pcd, angle_increment, min_height, max_height, num_vertical_divisions=1, min_range=0.0,
                                max_range=float("inf"), min_angle=-np.pi, max_angle=np.pi):
        if not LaserScanBuffer._factory_check("CreateFromPointCloud", "min_height", angle_increment, min_height, max_height,
                                              min_range, max_range, min_angle, max_angle):
            return None
        pts = pcd.points.tensor
        eng = get_engine(pts.device.index)
        try:
            bins, _ = eng.laserscan_from_points(pts, angle_increment, min_height, max_height, num_vertical_divisions,
                                                min_range, max_range, min_angle, max_angle)
        except _lib.MiIcpError as e:
            if e.code != _lib.MI_ICP_ERR_INVALID:
                raise
            _log_error("[LaserScanBuffer::CreateFromPointCloud] %s" % e)
            return None
        return LaserScanBuffer._from_bins(bins, eng.device, min_height, max_height, int(num_vertical_divisions),
                                          float(np.float32(min_angle)), float(np.float32(max_angle)))

    @staticmethod
    def create_from_depth_image(depth, intrinsic, angle_increment, min_y, max_y, num_vertical_divisions=1, min_range=0.0,
                                max_range=float("inf"), min_angle=-np.pi, max_angle=np.pi, depth_scale=1000.0,
                                depth_trunc=1000.0, stride=1):
        if not LaserScanBuffer._factory_check("CreateFromDepthImage", "min_y", angle_increment, min_y, max_y, min_range,
                                              max_range, min_angle, max_angle):
            return None
        d = _img(depth)
        if not _is_torch(d):
            d = torch.from_numpy(np.ascontiguousarray(d)).to(torch.device("cuda", utility.default_device()))
        eng = get_engine(d.device.index)
        try:
            bins, _ = eng.laserscan_from_depth(d, intrinsic.as4(), angle_increment, min_y, max_y, num_vertical_divisions,
                                               min_range, max_range, min_angle, max_angle, depth_scale, depth_trunc, stride)
        except (TypeError, _lib.MiIcpError) as e:
            if isinstance(e, _lib.MiIcpError) and e.code != _lib.MI_ICP_ERR_INVALID:
                raise
            _log_error("[LaserScanBuffer::CreateFromDepthImage] %s" % e)
            return None
        return LaserScanBuffer._from_bins(bins, eng.device, min_y, max_y, int(num_vertical_divisions),
                                          float(np.float32(min_angle)), float(np.float32(max_angle)), left=_QUARTER_TURN_X)


def _create_from_laserscanbuffer(scan, min_range, max_range):
    """PointCloud::CreateFromLaserScanBuffer (pointcloud_factory.cu:375-420): the live scans' readings inside
    [min_range, max_range] as points in the frame of their origins, oldest scan first; intensities become grey colours."""
    out = PointCloud()
    if scan.is_empty() or scan._ranges is None:
        _log_error("[PointCloud::CreateFromLaserScanBuffer] Empty scan, return empty pointcloud.")
        return out
    if min_range >= max_range:
        _log_error("[PointCloud::CreateFromLaserScanBuffer] min_range must be smaller than max_range.")
        return out
    p, c, _ = scan._eng().laserscan_to_points(scan._ranges, scan._intensities, scan._origins, scan.num_steps, scan.num_max_scans,
                                              scan.top_ % scan.num_max_scans, scan.num_scans, scan.min_angle, scan.max_angle,
                                              min_range, max_range)
    out._points = utility.Vector3fVector(p)
    if c is not None:
        out._colors = utility.Vector3fVector(c)
    return out


PointCloud.create_from_laserscanbuffer = staticmethod(_create_from_laserscanbuffer)
