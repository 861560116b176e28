// grid_rules.h -- the rules of the grid geometries that host and device share (OccupancyGrid, DistanceTransform, VoxelGrid,
// collision, the TSDF volumes): the cell of a point, the dense res^3 cube, an inclusive box of voxels, "occupied", and
// the search in ascending keys int32[m][3].  Plain C++: the kernels, the launchers and a stand-alone host program include it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MI_GRID_HD __host__ __device__ __forceinline__
#else
#define MI_GRID_HD inline
#endif

namespace mi {

struct GridFrame {  // voxel_size_ and origin_ at the time of the call
    float vs;
    float origin[3];
};

// floor to int with the value held inside +-1e9 first (a NaN becomes -1e9): no conversion is undefined
MI_GRID_HD int floor_int(float x) { return (int)fminf(fmaxf(floorf(x), -1.0e9f), 1.0e9f); }

// the cell of coordinate p along `axis`: floor((p - origin) / voxel_size), in fp32 and in that order
MI_GRID_HD int cell_of(const GridFrame& f, float p, int axis) { return floor_int((p - f.origin[axis]) / f.vs); }

MI_GRID_HD bool finite3(float x, float y, float z) { return (x - x == 0.0f) && (y - y == 0.0f) && (z - z == 0.0f); }

// a dense grid is res^3 cells, indexed (x*res + y)*res + z, z fastest
MI_GRID_HD bool cube_inside(int res, int x, int y, int z) { return x >= 0 && x < res && y >= 0 && y < res && z >= 0 && z < res; }
MI_GRID_HD int64_t cube_index(int res, int x, int y, int z) { return ((int64_t)x * res + y) * res + z; }

struct GridBox {  // the voxels [x0, x0+ex) x [y0, y0+ey) x [z0, z0+ez), count of them
    int x0, y0, z0, ex, ey, ez;
    int64_t count;
};

// the box of inclusive bounds min[3], max[3]; an empty one (all zero) when min > max on any axis
MI_GRID_HD GridBox box_of_bounds(const int b[6]) {
    GridBox box = {};
    if (b[0] > b[3] || b[1] > b[4] || b[2] > b[5]) return box;
    box.x0 = b[0];
    box.y0 = b[1];
    box.z0 = b[2];
    box.ex = b[3] - b[0] + 1;
    box.ey = b[4] - b[1] + 1;
    box.ez = b[5] - b[2] + 1;
    box.count = (int64_t)box.ex * box.ey * box.ez;
    return box;
}

// voxel t of the box, 0 <= t < count, z fastest: ascending t is ascending cube_index
MI_GRID_HD void box_voxel(const GridBox& b, int64_t t, int* x, int* y, int* z) {
    const int64_t eyz = (int64_t)b.ey * b.ez;
    const int yz = (int)(t % eyz);
    *x = b.x0 + (int)(t / eyz);
    *y = b.y0 + yz / b.ez;
    *z = b.z0 + yz % b.ez;
}

// a voxel of log-odds p is occupied when it is known (p is no NaN) and p > thres
MI_GRID_HD bool occupied(float p, float thres) { return p > thres; }  // (false for a NaN)

// ascending keys int32[m][3], x most significant: is key a below (x, y, z)?
MI_GRID_HD bool keys3_less(const int32_t* a, int32_t x, int32_t y, int32_t z) {
    if (a[0] != x) return a[0] < x;
    if (a[1] != y) return a[1] < y;
    return a[2] < z;
}

// the first position whose key is not less than (x, y, z)
MI_GRID_HD int64_t keys3_lower(const int32_t* keys, int64_t m, int32_t x, int32_t y, int32_t z) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys3_less(keys + mid * 3, x, y, z)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the first position whose key is greater than (x, y, z)
MI_GRID_HD int64_t keys3_upper(const int32_t* keys, int64_t m, int32_t x, int32_t y, int32_t z) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t* k = keys + mid * 3;
        const bool greater = k[0] != x ? k[0] > x : (k[1] != y ? k[1] > y : k[2] > z);
        if (greater) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace mi
