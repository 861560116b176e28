"""cupoch.collision mirror (src/cupoch/collision/{collision,primitives}.h, python surface
src/python/cupoch_pybind/collision): the primitives, PrimitiveArray, CollisionResult, compute_intersection between a
VoxelGrid or an OccupancyGrid and another grid, a LineSet or primitives, and create_voxel_grid of a primitive.  The
contract is in include/mi_icp.h ("collision"); every query runs on the GPU through mi_icp_collision_compute.
Not built: Primitives x Primitives, create_voxel_grid_with_sweeping, create_triangle_mesh, Mesh primitives, a
DistanceTransform as a target."""
import enum

import numpy as np

from . import geometry
from ._lib import MiIcpError

_RECORD = np.dtype([("type", np.int32), ("transform", np.float32, 16), ("param", np.float32, 3)])


class Primitive:
    """collision::Primitive: a type and a 4x4 transform (row, column)"""

    class Type(enum.IntEnum):
        Unspecified = 0
        Box = 1
        Sphere = 2
        Capsule = 3
        Cylinder = 4
        Mesh = 5

    def __init__(self, type=None, transform=None):
        self.type = Primitive.Type.Unspecified if type is None else Primitive.Type(int(type))
        self.transform = np.eye(4, dtype=np.float32) if transform is None else np.asarray(transform, np.float32).reshape(4, 4).copy()

    def _param(self):
        return (0.0, 0.0, 0.0)

    def _record(self):
        rec = np.zeros(1, _RECORD)
        rec["type"][0] = int(self.type)
        rec["transform"][0] = np.asarray(self.transform, np.float32).reshape(4, 4).T.reshape(16)
        rec["param"][0] = np.asarray(self._param(), np.float32)
        return rec

    def get_axis_aligned_bounding_box(self):
        from .engine import Engine
        lo, hi = Engine.primitive_aabb(self._record())
        return geometry.AxisAlignedBoundingBox(lo, hi)

    def __repr__(self):
        return "collision::Primitive(%s)" % self.type.name


class Box(Primitive):
    def __init__(self, lengths=(0.0, 0.0, 0.0), transform=None):
        super().__init__(Primitive.Type.Box, transform)
        self.lengths = np.asarray(lengths, np.float32).reshape(3).copy()

    def _param(self):
        return self.lengths


class Sphere(Primitive):
    def __init__(self, radius=0.0, center=None):
        super().__init__(Primitive.Type.Sphere)
        self.radius = float(radius)
        if center is not None:
            self.transform[:3, 3] = np.asarray(center, np.float32).reshape(3)

    def _param(self):
        return (self.radius, 0.0, 0.0)


class Capsule(Primitive):
    def __init__(self, radius=0.0, height=0.0, transform=None):
        super().__init__(Primitive.Type.Capsule, transform)
        self.radius, self.height = float(radius), float(height)

    def _param(self):
        return (self.radius, self.height, 0.0)


class Cylinder(Primitive):
    def __init__(self, radius=0.0, height=0.0, transform=None):
        super().__init__(Primitive.Type.Cylinder, transform)
        self.radius, self.height = float(radius), float(height)

    def _param(self):
        return (self.radius, self.height, 0.0)


class PrimitiveArray:
    """device_vector<PrimitivePack>: a list of primitives; the records travel to the GPU when a query is made"""

    def __init__(self, primitives=()):
        self._items = list(primitives)

    def append(self, primitive):
        self._items.append(primitive)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        return self._items[i]

    def __iter__(self):
        return iter(self._items)

    def _records(self):
        return np.concatenate([p._record() for p in self._items]) if self._items else np.zeros(0, _RECORD)


class CollisionResult:
    """collision::CollisionResult: first / second name the kinds of the two arguments; collision_index_pairs is int32
    [m, 2] on the device, column 0 indexing the first argument, column 1 the second"""

    class CollisionType(enum.IntEnum):
        Unspecified = 0
        Primitives = 1
        VoxelGrid = 2
        OccupancyGrid = 3
        LineSet = 4

    def __init__(self, first=None, second=None, collision_index_pairs=None):
        self.first = CollisionResult.CollisionType.Unspecified if first is None else first
        self.second = CollisionResult.CollisionType.Unspecified if second is None else second
        self.collision_index_pairs = collision_index_pairs

    def _pairs(self):
        if self.collision_index_pairs is None:
            return np.zeros((0, 2), np.int32)
        p = self.collision_index_pairs
        return p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p, np.int32)

    def is_collided(self):
        return self.collision_index_pairs is not None and len(self.collision_index_pairs) > 0

    def get_collision_index_pairs(self):
        return self._pairs()

    def get_first_collision_indices(self):
        return self._pairs()[:, 0].copy()

    def get_second_collision_indices(self):
        return self._pairs()[:, 1].copy()

    def __repr__(self):
        return "collision::CollisionResult with %d collisions." % len(self._pairs())


CollitionResult = CollisionResult     # (the reference's spelling of the python class)


def _kind(x):
    T = CollisionResult.CollisionType
    if isinstance(x, geometry.VoxelGrid):
        return T.VoxelGrid
    if isinstance(x, geometry.OccupancyGrid):
        return T.OccupancyGrid
    if isinstance(x, geometry.LineSet):
        return T.LineSet
    if isinstance(x, (PrimitiveArray, list, tuple)):
        return T.Primitives
    raise TypeError("compute_intersection: %r is not a VoxelGrid, OccupancyGrid, LineSet or PrimitiveArray" % type(x).__name__)


def _engine_of(a, b):
    for x in (a, b):
        if isinstance(x, geometry.OccupancyGrid):
            return x._call()[0]
    for x in (a, b):
        if isinstance(x, geometry.VoxelGrid):
            return x._eng()
    return geometry.get_engine()


def _side(eng, x):
    if isinstance(x, geometry.VoxelGrid):
        keys, _ = x._arrays()
        return eng.collision_voxel_side(keys, x.voxel_size, x.origin, keys_sorted=x._sorted)
    if isinstance(x, geometry.OccupancyGrid):
        e, grid, params = x._call()
        if e is not eng:
            raise MiIcpError("compute_intersection: the occupancy grid belongs to another device")
        return eng.collision_occgrid_side(grid, params)
    if isinstance(x, geometry.LineSet):
        return eng.collision_lineset_side(x.points.tensor, x.lines.tensor)
    arr = x if isinstance(x, PrimitiveArray) else PrimitiveArray(x)
    return eng.collision_primitives_side(arr._records())


def compute_intersection(a, b, margin=0.0, first_capacity=None):
    """collision::ComputeIntersection: every colliding element of the enumerated side (the lines when a LineSet is
    either argument, else b) gives one pair with the smallest colliding index of the other side; ascending.
    first_capacity: room for that many pairs on the first call (65536 when None); with more pairs than that the whole
    query is computed a second time, so a caller who expects many passes an upper bound (the enumerated side's count)."""
    ka, kb = _kind(a), _kind(b)
    eng = _engine_of(a, b)
    pairs = eng.collision_compute(_side(eng, a), _side(eng, b), margin, first_capacity)
    return CollisionResult(ka, kb, pairs)


def create_voxel_grid(primitive, voxel_size):
    """collision::CreateVoxelGrid: the cells of a lattice around the primitive that it collides with"""
    eng = geometry.get_engine()
    out = geometry.VoxelGrid()
    try:
        keys, colors, origin = eng.collision_voxelize_primitive(primitive._record(), voxel_size)
    except MiIcpError as e:
        if getattr(e, "code", None) != -1:
            raise
        geometry._log_error(str(e))
        return out
    out.voxel_size = float(np.float32(voxel_size))
    out.origin = origin
    if int(keys.shape[0]):
        out._set(keys, colors, True)
    return out
