// cupoch_pybind -- the reference's pybind11 module for the ICP path, built on this repository's C++
// surface (namespace cupoch, libcupoch_amd.so) instead of the CUDA library.
//
// Same module layout, names, defaults and property names as src/python/cupoch_pybind of the reference:
//   cupoch_pybind.utility       Vector3fVector, ULongVector, IntVector, BoolVector (device vector wrappers with .cpu()),
//                               initialize_allocator
//                               (src/python/cupoch_pybind/utility/eigen.cpp:123-200, cupoch_pybind.cpp:46-49)
//   cupoch_pybind.geometry      PointCloud, KDTreeSearchParamKNN / Radius, KDTreeFlann
//                               (geometry/pointcloud.cpp:33-160, geometry/kdtreeflann.cpp)
//   cupoch_pybind.registration  ICPConvergenceCriteria, RegistrationResult, TransformationEstimation* (each behind the
//                               PyTransformationEstimation trampoline: Python-defined estimators, registration.cpp:36-60),
//                               registration_icp, evaluate_registration, registration_generalized_icp,
//                               registration_colored_icp  (registration/registration.cpp:64-448)
//   PointCloud.to_/from_{points,normals,colors}_dlpack  (geometry/pointcloud.cpp:82-100, utility/dl_converter.cu)
// The reference converts Eigen types through pybind11/eigen.h; Eigen is absent here, so 4x4 / 3-vectors
// cross the boundary as float32 numpy arrays converted by hand.
#include <hip/hip_runtime_api.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "cupoch/camera/pinhole_camera_intrinsic.h"
#include "cupoch/camera/pinhole_camera_parameters.h"
#include "cupoch/collision/collision.h"
#include "cupoch/geometry/distancetransform.h"
#include "cupoch/geometry/graph.h"
#include "cupoch/geometry/image.h"
#include "cupoch/geometry/keypoint.h"
#include "cupoch/geometry/laserscanbuffer.h"
#include "cupoch/geometry/occupancygrid.h"
#include "cupoch/geometry/pointcloud.h"
#include "cupoch/geometry/voxelgrid.h"
#include "cupoch/imageproc/sgm.h"
#include "cupoch/integration/scalable_tsdfvolume.h"
#include "cupoch/integration/uniform_tsdfvolume.h"
#include "cupoch/kinfu/kinfu.h"
#include "cupoch/knn/kdtree_flann.h"
#include "cupoch/knn/kdtree_search_param.h"
#include "cupoch/planning/planner.h"
#include "cupoch/registration/fast_global_registration.h"
#include "cupoch/registration/feature.h"
#include "cupoch/registration/generalized_icp.h"
#include "cupoch/registration/registration.h"
#include "cupoch/registration/transformation_estimation.h"

namespace py = pybind11;
using namespace py::literals;
using namespace cupoch;

namespace {

typedef py::array_t<float, py::array::c_style | py::array::forcecast> farray;

Eigen::Matrix4f to_matrix4(const farray& a) {
    if (a.ndim() != 2 || a.shape(0) != 4 || a.shape(1) != 4) throw std::invalid_argument("expected a 4x4 float32 array");
    Eigen::Matrix4f m;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) m(r, c) = a.at(r, c);
    return m;
}

Eigen::Matrix3f to_matrix3(const farray& a) {
    if (a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 3) throw std::invalid_argument("expected a 3x3 float32 array");
    Eigen::Matrix3f m;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) m(r, c) = a.at(r, c);
    return m;
}

farray from_matrix4(const Eigen::Matrix4f& m) {
    farray a({4, 4});
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) a.mutable_at(r, c) = m(r, c);
    return a;
}

farray identity4() { return from_matrix4(Eigen::Matrix4f::Identity()); }

Eigen::Vector3f to_vector3(const farray& a) {
    if (a.size() != 3) throw std::invalid_argument("expected 3 floats");
    Eigen::Vector3f v;
    const float* p = a.data();
    v(0) = p[0];
    v(1) = p[1];
    v(2) = p[2];
    return v;
}

farray from_vector3(const Eigen::Vector3f& v) {
    farray a(3);
    for (int i = 0; i < 3; ++i) a.mutable_at(i) = v(i);
    return a;
}

Eigen::Vector3i to_vector3i(const py::array_t<int, py::array::c_style | py::array::forcecast>& a) {
    if (a.size() != 3) throw std::invalid_argument("expected 3 integers");
    const int* p = a.data();
    return Eigen::Vector3i(p[0], p[1], p[2]);
}

// the extractions' voxels as a list of geometry.OccupancyVoxel, ascending in linear index
py::list voxel_list(const std::vector<geometry::OccupancyVoxel>& v) {
    py::list out;
    for (const geometry::OccupancyVoxel& x : v) out.append(py::cast(x));
    return out;
}

// geometry.DeviceVoxelMap: what VoxelGrid.voxels gives and takes -- the keys and the voxels on the device, with
// __len__ and cpu() (grid_index (m, 3) int32, color (m, 3) float32); constructed from two such arrays
struct DeviceVoxelMap {
    utility::device_vector<Eigen::Vector3i> keys;
    utility::device_vector<geometry::Voxel> values;
    DeviceVoxelMap() = default;
    DeviceVoxelMap(const py::array_t<int, py::array::c_style | py::array::forcecast>& k, const farray& c) {
        if (k.ndim() != 2 || k.shape(1) != 3 || c.ndim() != 2 || c.shape(1) != 3 || c.shape(0) != k.shape(0))
            throw std::invalid_argument("expected an (m, 3) int32 array and an (m, 3) float32 array");
        const size_t m = (size_t)k.shape(0);
        std::vector<Eigen::Vector3i> hk(m);
        std::vector<geometry::Voxel> hv(m);
        for (size_t i = 0; i < m; ++i) {
            hk[i] = Eigen::Vector3i(k.at(i, 0), k.at(i, 1), k.at(i, 2));
            hv[i] = geometry::Voxel(hk[i], Eigen::Vector3f(c.at(i, 0), c.at(i, 1), c.at(i, 2)));
        }
        keys = hk;
        values = hv;
    }
    py::tuple cpu() const {
        const std::vector<Eigen::Vector3i> hk = keys.to_host();
        const std::vector<geometry::Voxel> hv = values.to_host();
        py::array_t<int> k({(py::ssize_t)hk.size(), (py::ssize_t)3});
        farray c({(py::ssize_t)hv.size(), (py::ssize_t)3});
        for (size_t i = 0; i < hk.size(); ++i)
            for (int d = 0; d < 3; ++d) k.mutable_at(i, d) = hk[i](d);
        for (size_t i = 0; i < hv.size(); ++i)
            for (int d = 0; d < 3; ++d) c.mutable_at(i, d) = hv[i].color_(d);
        return py::make_tuple(k, c);
    }
};

// utility.Vector3fVector: a device vector of Vector3f, constructed from an (n, 3) array (one H2D
// copy), .cpu() copies back (device_vector_wrapper.cu:39-44,119-125)
struct Vector3fVector {
    utility::device_vector<Eigen::Vector3f> data;
    Vector3fVector() = default;
    explicit Vector3fVector(const farray& a) { assign(a); }
    void assign(const farray& a) {
        if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument("expected an (n, 3) float32 array");
        std::vector<Eigen::Vector3f> h((size_t)a.shape(0));
        if (!h.empty()) std::memcpy((void*)h.data(), a.data(), h.size() * sizeof(Eigen::Vector3f));
        data = h;
    }
    farray cpu() const {
        const std::vector<Eigen::Vector3f> h = data.to_host();
        farray a({(py::ssize_t)h.size(), (py::ssize_t)3});
        if (!h.empty()) std::memcpy(a.mutable_data(), (const void*)h.data(), h.size() * sizeof(Eigen::Vector3f));
        return a;
    }
};

Vector3fVector wrap(const utility::device_vector<Eigen::Vector3f>& v) {
    Vector3fVector w;
    w.data = v;
    return w;
}

// geometry.Image from a [H, W] or [H, W, C] array (the reference's Image takes the buffer protocol,
// cupoch_pybind/geometry/image.cpp): width, height, channels and bytes per channel as the array has them
geometry::Image image_from_array(const py::array& arr) {
    if (arr.ndim() != 2 && arr.ndim() != 3) throw std::invalid_argument("Image: expected a [H, W] or [H, W, C] array");
    const py::array a = py::array::ensure(arr, py::array::c_style);
    geometry::Image img;
    const size_t bytes = (size_t)a.nbytes();
    img.Prepare((int)a.shape(1), (int)a.shape(0), a.ndim() == 3 ? (int)a.shape(2) : 1, (int)a.itemsize());
    if (bytes) img.SetData(std::vector<uint8_t>((const uint8_t*)a.data(), (const uint8_t*)a.data() + bytes));
    return img;
}

// a property that accepts a Vector3fVector or anything array-like
void set_vec(utility::device_vector<Eigen::Vector3f>& dst, const py::object& o) {
    if (py::isinstance<Vector3fVector>(o)) dst = o.cast<const Vector3fVector&>().data;
    else dst = Vector3fVector(o.cast<farray>()).data;
}

// utility.Vector2iVector: the CorrespondenceSet as the reference hands it to Python estimators
// (utility/eigen.cpp:340-342): a device vector of (source, target) index pairs with .cpu()
struct Vector2iVector {
    registration::CorrespondenceSet data;
    Vector2iVector() = default;
    explicit Vector2iVector(const py::array_t<int, py::array::c_style | py::array::forcecast>& a) {
        if (a.ndim() != 2 || a.shape(1) != 2) throw std::invalid_argument("expected an (n, 2) int32 array");
        std::vector<Eigen::Vector2i> h((size_t)a.shape(0));
        if (!h.empty()) std::memcpy((void*)h.data(), a.data(), h.size() * sizeof(Eigen::Vector2i));
        data = h;
    }
};

// utility.ULongVector: device_vector<size_t> (utility/eigen.cpp:237), the indices the outlier filters return and
// select_by_index takes; constructed from a 1-D integer array, .cpu() gives int64
struct ULongVector {
    utility::device_vector<size_t> data;
    ULongVector() = default;
    explicit ULongVector(const py::array_t<int64_t, py::array::c_style | py::array::forcecast>& a) {
        if (a.ndim() != 1) throw std::invalid_argument("expected a 1-D integer array");
        std::vector<size_t> h((size_t)a.shape(0));
        if (!h.empty()) std::memcpy((void*)h.data(), a.data(), h.size() * sizeof(size_t));
        data = h;
    }
    py::array_t<int64_t> cpu() const {
        const std::vector<size_t> h = data.to_host();
        py::array_t<int64_t> a((py::ssize_t)h.size());
        if (!h.empty()) std::memcpy(a.mutable_data(), (const void*)h.data(), h.size() * sizeof(size_t));
        return a;
    }
};

// utility.IntVector: device_vector<int> (the reference's device_vector_int wrapper), the labels cluster_dbscan returns;
// .cpu() gives int32
struct IntVector {
    utility::device_vector<int> data;
    IntVector() = default;
    explicit IntVector(const py::array_t<int32_t, py::array::c_style | py::array::forcecast>& a) {
        if (a.ndim() != 1) throw std::invalid_argument("expected a 1-D integer array");
        std::vector<int> h((size_t)a.shape(0));
        if (!h.empty()) std::memcpy((void*)h.data(), a.data(), h.size() * sizeof(int));
        data = h;
    }
    py::array_t<int32_t> cpu() const {
        const std::vector<int> h = data.to_host();
        py::array_t<int32_t> a((py::ssize_t)h.size());
        if (!h.empty()) std::memcpy(a.mutable_data(), (const void*)h.data(), h.size() * sizeof(int));
        return a;
    }
};

// utility.BoolVector: device_vector<bool> (the reference's device_vector_bool wrapper), the mask compute_iss_keypoints
// returns and select_by_mask takes; .cpu() gives bool
struct BoolVector {
    utility::device_vector<bool> data;
    BoolVector() = default;
    explicit BoolVector(const py::array_t<bool, py::array::c_style | py::array::forcecast>& a) {
        if (a.ndim() != 1) throw std::invalid_argument("expected a 1-D boolean array");
        data.resize((size_t)a.shape(0));   // (std::vector<bool> is packed: the bytes go across as they are)
        if (!data.empty()) utility::copy_h2d(data.data(), a.data(), data.size());
    }
    py::array_t<bool> cpu() const {
        py::array_t<bool> a((py::ssize_t)data.size());
        if (!data.empty()) utility::copy_d2h(a.mutable_data(), data.data(), data.size());
        return a;
    }
};

py::array_t<int> corres_to_array(const registration::CorrespondenceSet& c) {
    const std::vector<Eigen::Vector2i> h = c.to_host();
    py::array_t<int> a({(py::ssize_t)h.size(), (py::ssize_t)2});
    if (!h.empty()) std::memcpy(a.mutable_data(), (const void*)h.data(), h.size() * sizeof(Eigen::Vector2i));
    return a;
}

// registration::Feature<Dim> (cupoch_pybind/registration/feature.cpp: FeatureFPFH, FeatureSHOT): `data` is an (n, Dim)
// float32 array, copied from / to the device on access
template <int Dim>
void bind_feature(py::module& mr, const char* name, const char* doc) {
    using F = registration::Feature<Dim>;
    py::class_<F, std::shared_ptr<F>>(mr, name, doc)
            .def(py::init<>())
            .def(py::init<const F&>())
            .def("__copy__", [](const F& f) { return F(f); })
            .def("__deepcopy__", [](const F& f, py::dict&) { return F(f); })
            .def("resize", &F::Resize, py::arg("n"))
            .def("dimension", &F::Dimension)
            .def("num", &F::Num)
            .def("is_empty", &F::IsEmpty)
            .def_property(
                    "data",
                    [](const F& f) {
                        const auto h = f.GetData();
                        py::array_t<float> a({(py::ssize_t)h.size(), (py::ssize_t)Dim});
                        if (!h.empty()) std::memcpy(a.mutable_data(), (const void*)h.data(), h.size() * sizeof(typename F::FeatureType));
                        return a;
                    },
                    [](F& f, const py::array_t<float, py::array::c_style | py::array::forcecast>& a) {
                        if (a.ndim() != 2 || a.shape(1) != Dim) throw py::value_error("Feature data must be (n, " + std::to_string(Dim) + ")");
                        std::vector<typename F::FeatureType> h((size_t)a.shape(0));
                        if (!h.empty()) std::memcpy((void*)h.data(), a.data(), h.size() * sizeof(typename F::FeatureType));
                        f.SetData(h);
                    })
            .def("__repr__", [](const F& f) {
                return "registration::Feature class with dimension = " + std::to_string(f.Dimension()) + " and num = " +
                       std::to_string(f.Num()) + "\nAccess its data via data member.";
            });
}

// ---------------------------------------------------------------------------------------------------------
// Python-defined estimators (registration/registration.cpp:36-60 of the reference: PyTransformationEstimation with
// PYBIND11_OVERLOAD_PURE).  A Python subclass overrides the C++ virtuals under their C++ NAMES, as that macro has
// it -- GetTransformationEstimationType / ComputeRMSE / ComputeTransformation -- or under the snake_case names the
// methods are bound with; RegistrationICP then runs the reference's host loop (registration.cu:144-171) and makes
// the virtual calls.  pybind11/eigen.h is not available (no Eigen), so the 4x4 comes back as a numpy array and is
// converted by hand.  A built-in estimator that Python did not subclass is constructed as its plain C++ type (pybind11
// makes the alias only for Python-derived instances), so it still takes the device-resident loop.
template <class Base = registration::TransformationEstimation>
class PyTransformationEstimation : public Base {
public:
    using Base::Base;

    registration::TransformationEstimationType GetTransformationEstimationType() const override {
        py::gil_scoped_acquire gil;
        const py::function f = find("GetTransformationEstimationType", "get_transformation_estimation_type");
        if (f) return f().template cast<registration::TransformationEstimationType>();
        if constexpr (std::is_abstract<Base>::value) pure("GetTransformationEstimationType");
        else return Base::GetTransformationEstimationType();
    }
    float ComputeRMSE(const geometry::PointCloud& source, const geometry::PointCloud& target,
                      const registration::CorrespondenceSet& corres) const override {
        py::gil_scoped_acquire gil;
        const py::function f = find("ComputeRMSE", "compute_rmse");
        if (f) return call(f, source, target, corres).template cast<float>();
        if constexpr (std::is_abstract<Base>::value) pure("ComputeRMSE");
        else return Base::ComputeRMSE(source, target, corres);
    }
    Eigen::Matrix4f ComputeTransformation(const geometry::PointCloud& source, const geometry::PointCloud& target,
                                          const registration::CorrespondenceSet& corres) const override {
        py::gil_scoped_acquire gil;
        const py::function f = find("ComputeTransformation", "compute_transformation");
        if (f) return to_matrix4(call(f, source, target, corres).template cast<farray>());
        if constexpr (std::is_abstract<Base>::value) pure("ComputeTransformation");
        else return Base::ComputeTransformation(source, target, corres);
    }

private:
    py::function find(const char* cpp_name, const char* py_name) const {
        py::function f = py::get_override(static_cast<const Base*>(this), cpp_name);
        if (!f) f = py::get_override(static_cast<const Base*>(this), py_name);
        return f;
    }
    // the clouds by reference (the estimator sees the loop's own objects, as in the reference), the set as a Vector2iVector
    static py::object call(const py::function& f, const geometry::PointCloud& source, const geometry::PointCloud& target,
                           const registration::CorrespondenceSet& corres) {
        Vector2iVector v;
        v.data = corres;
        return f(py::cast(source, py::return_value_policy::reference), py::cast(target, py::return_value_policy::reference),
                 py::cast(std::move(v)));
    }
    [[noreturn]] static void pure(const char* name) {
        py::pybind11_fail(std::string("Tried to call pure virtual function \"TransformationEstimation::") + name + "\"");
    }
};

// ---------------------------------------------------------------------------------------------------------
// DLPack (geometry/pointcloud.cpp:82-100, utility/dl_converter.cu:42-118, cupoch_pybind/dl_converter.inl of the
// reference; its third_party/dlpack is an empty submodule here, so the ABI structs of DLPack's stable v0.x
// `DLManagedTensor` -- what a capsule named "dltensor" carries -- are restated).  Export: an (n, 3) float32 tensor on
// kDLROCM over the cloud's OWN buffer -- zero-copy, as the reference publishes it (dl_converter.cu:60-86) -- kept alive
// by a shared handle on the block (utility::device_vector::share): the tensor stays valid when the cloud is destroyed
// or re-allocated, sees what the cloud's in-place operations (Transform, ...) write until then, and costs nothing
// (the reference's handle is a thrust copy of the vector, 120 MB for a 10M-point cloud, that nothing reads).  Import:
// host (kDLCPU / pinned) or device (kDLROCM, or kDLCUDA as PyTorch-ROCm builds before 2.x labelled it) memory is COPIED
// into the cloud's vector; the capsule is left to its owner, as in the reference.
extern "C" {
typedef struct { int32_t device_type; int32_t device_id; } MiDLDevice;
typedef struct { uint8_t code; uint8_t bits; uint16_t lanes; } MiDLDataType;
typedef struct {
    void* data;
    MiDLDevice device;
    int32_t ndim;
    MiDLDataType dtype;
    int64_t* shape;
    int64_t* strides;
    uint64_t byte_offset;
} MiDLTensor;
typedef struct MiDLManagedTensor {
    MiDLTensor dl_tensor;
    void* manager_ctx;
    void (*deleter)(struct MiDLManagedTensor*);
} MiDLManagedTensor;
}
enum { kMiDLCPU = 1, kMiDLCUDA = 2, kMiDLCUDAHost = 3, kMiDLROCM = 10, kMiDLROCMHost = 11 };
enum { kMiDLInt = 0, kMiDLFloat = 2 };

struct Vec3Export {
    std::shared_ptr<void> handle;  // the cloud's block, shared
    int64_t shape[2];
    MiDLManagedTensor tensor;
};

// V: rows of `cols` 32-bit words (Eigen::Vector3f: 3 floats; Eigen::Vector2i, a graph's edges: 2 ints, code kMiDLInt)
template <class V>
py::capsule to_dlpack_capsule(const utility::device_vector<V>& src, int cols = 3, int code = kMiDLFloat) {
    Vec3Export* e = new Vec3Export();
    e->handle = src.share();  // no copy: the tensor and the cloud hold the same block
    int dev = 0;
    (void)hipGetDevice(&dev);
    // (the legacy capsule has no stream handshake: everything enqueued that writes the block has finished before a
    // consumer on any stream sees the pointer -- ADVICE r5; INTEGRATION.md section 2 lists what aliasing means otherwise)
    (void)hipDeviceSynchronize();
    e->shape[0] = (int64_t)src.size();
    e->shape[1] = cols;
    MiDLTensor& t = e->tensor.dl_tensor;
    t.data = (void*)src.data();
    t.device.device_type = kMiDLROCM;
    t.device.device_id = dev;
    t.ndim = 2;
    t.dtype.code = (uint8_t)code;
    t.dtype.bits = 32;
    t.dtype.lanes = 1;
    t.shape = e->shape;
    t.strides = nullptr;  // compact row-major
    t.byte_offset = 0;
    e->tensor.manager_ctx = e;
    e->tensor.deleter = [](MiDLManagedTensor* m) { delete static_cast<Vec3Export*>(m->manager_ctx); };
    return py::capsule(&e->tensor, "dltensor", [](PyObject* obj) {
        // a consumer renames the capsule ("used_dltensor") and owns the tensor from then on
        void* ptr = PyCapsule_IsValid(obj, "dltensor") ? PyCapsule_GetPointer(obj, "dltensor") : nullptr;
        if (ptr) {
            MiDLManagedTensor* m = static_cast<MiDLManagedTensor*>(ptr);
            if (m->deleter) m->deleter(m);
        } else {
            PyErr_Clear();
        }
    });
}

template <class V>
void from_dlpack_capsule(const py::capsule& cap, utility::device_vector<V>& dst, int cols = 3, int code = kMiDLFloat) {
    if (!PyCapsule_IsValid(cap.ptr(), "dltensor")) {
        PyErr_Clear();
        throw std::invalid_argument("expected a DLPack capsule named \"dltensor\" (not yet consumed)");
    }
    const MiDLManagedTensor* m = static_cast<const MiDLManagedTensor*>(PyCapsule_GetPointer(cap.ptr(), "dltensor"));
    const MiDLTensor& t = m->dl_tensor;
    if (t.ndim != 2 || t.shape[1] != cols || t.dtype.code != code || t.dtype.bits != 32 || t.dtype.lanes != 1)
        throw std::invalid_argument(code == kMiDLFloat ? "from_*_dlpack: expected an (n, 3) float32 tensor" : "from_*_dlpack: expected an (n, 2) int32 tensor");
    if (t.strides && t.shape[0] > 0 && (t.strides[1] != 1 || (t.shape[0] > 1 && t.strides[0] != cols)))
        throw std::invalid_argument("from_*_dlpack: the tensor must be contiguous");
    const size_t n = (size_t)t.shape[0];
    const char* src = static_cast<const char*>(t.data) + t.byte_offset;
    const int kind = t.device.device_type;
    dst.resize(0);
    dst.resize(n);
    if (n == 0) return;
    const size_t bytes = n * sizeof(V);
    hipError_t e;
    if (kind == kMiDLCPU || kind == kMiDLCUDAHost || kind == kMiDLROCMHost) e = hipMemcpy(dst.data(), src, bytes, hipMemcpyHostToDevice);
    else if (kind == kMiDLROCM || kind == kMiDLCUDA) e = hipMemcpy(dst.data(), src, bytes, hipMemcpyDeviceToDevice);
    else throw std::invalid_argument("from_*_dlpack: unsupported device type");  // utility::LogError in the reference (dl_converter.cu:116)
    if (e != hipSuccess) throw std::runtime_error(std::string("from_*_dlpack: ") + hipGetErrorString(e));
}

}  // namespace

PYBIND11_MODULE(cupoch_pybind, m) {
    m.doc() = "cupoch's ICP registration path on MI355X: the reference's pybind11 surface over libcupoch_amd / libmi_icp";
    // cupoch/__init__.py calls this on import (rmm pool set-up in the reference): nothing to do here
    m.def("initialize_allocator", [](py::args, py::kwargs) {}, "kept for compatibility; the engine sizes its buffers per cloud");

    // ---------------------------------------------------------------- utility
    py::module mu = m.def_submodule("utility");
    py::class_<Vector3fVector>(mu, "Vector3fVector")
            .def(py::init<>())
            .def(py::init<const farray&>(), "array"_a)
            .def("cpu", &Vector3fVector::cpu)
            .def("__len__", [](const Vector3fVector& v) { return v.data.size(); });
    py::class_<ULongVector>(mu, "ULongVector")
            .def(py::init<>())
            .def(py::init<const py::array_t<int64_t, py::array::c_style | py::array::forcecast>&>(), "array"_a)
            .def("cpu", &ULongVector::cpu)
            .def("__len__", [](const ULongVector& v) { return v.data.size(); });
    py::class_<IntVector>(mu, "IntVector")
            .def(py::init<>())
            .def(py::init<const py::array_t<int32_t, py::array::c_style | py::array::forcecast>&>(), "array"_a)
            .def("cpu", &IntVector::cpu)
            .def("__len__", [](const IntVector& v) { return v.data.size(); });
    py::class_<BoolVector>(mu, "BoolVector")
            .def(py::init<>())
            .def(py::init<const py::array_t<bool, py::array::c_style | py::array::forcecast>&>(), "array"_a)
            .def("cpu", &BoolVector::cpu)
            .def("__len__", [](const BoolVector& v) { return v.data.size(); });
    py::class_<Vector2iVector>(mu, "Vector2iVector")
            .def(py::init<>())
            .def(py::init<const py::array_t<int, py::array::c_style | py::array::forcecast>&>(), "array"_a)
            .def("cpu", [](const Vector2iVector& v) { return corres_to_array(v.data); })
            .def("__len__", [](const Vector2iVector& v) { return v.data.size(); });

    // ---------------------------------------------------------------- geometry
    py::module mg = m.def_submodule("geometry");
    py::class_<knn::KDTreeSearchParam>(mg, "KDTreeSearchParam");
    py::class_<knn::KDTreeSearchParamKNN, knn::KDTreeSearchParam>(mg, "KDTreeSearchParamKNN")
            .def(py::init<int>(), "knn"_a = 30)
            .def_readwrite("knn", &knn::KDTreeSearchParamKNN::knn_);
    py::class_<knn::KDTreeSearchParamRadius, knn::KDTreeSearchParam>(mg, "KDTreeSearchParamRadius")
            .def(py::init<float, int>(), "radius"_a, "max_nn"_a)
            .def_readwrite("radius", &knn::KDTreeSearchParamRadius::radius_)
            .def_readwrite("max_nn", &knn::KDTreeSearchParamRadius::max_nn_);

    // geometry::AxisAlignedBoundingBox<3> (cupoch_pybind/geometry/boundingvolume.cpp): what PointCloud.crop takes
    py::class_<geometry::AxisAlignedBoundingBox3, std::shared_ptr<geometry::AxisAlignedBoundingBox3>>(mg, "AxisAlignedBoundingBox")
            .def(py::init<>())
            .def(py::init([](const farray& lo, const farray& hi) {
                     return std::make_shared<geometry::AxisAlignedBoundingBox3>(to_vector3(lo), to_vector3(hi));
                 }),
                 "min_bound"_a, "max_bound"_a)
            .def_property(
                    "min_bound", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.min_bound_); },
                    [](geometry::AxisAlignedBoundingBox3& b, const farray& v) { b.min_bound_ = to_vector3(v); })
            .def_property(
                    "max_bound", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.max_bound_); },
                    [](geometry::AxisAlignedBoundingBox3& b, const farray& v) { b.max_bound_ = to_vector3(v); })
            .def("get_min_bound", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.GetMinBound()); })
            .def("get_max_bound", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.GetMaxBound()); })
            .def("get_center", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.GetCenter()); })
            .def("get_extent", [](const geometry::AxisAlignedBoundingBox3& b) { return from_vector3(b.GetExtent()); })
            .def("volume", &geometry::AxisAlignedBoundingBox3::Volume)
            .def("is_empty", &geometry::AxisAlignedBoundingBox3::IsEmpty);

    py::class_<geometry::PointCloud, std::shared_ptr<geometry::PointCloud>>(mg, "PointCloud")
            .def(py::init<>())
            .def(py::init([](const py::object& pts) {
                     auto pc = std::make_shared<geometry::PointCloud>();
                     set_vec(pc->points_, pts);
                     return pc;
                 }),
                 "points"_a)
            .def_property(
                    "points", [](const geometry::PointCloud& pc) { return wrap(pc.points_); },
                    [](geometry::PointCloud& pc, const py::object& o) { set_vec(pc.points_, o); })
            .def_property(
                    "normals", [](const geometry::PointCloud& pc) { return wrap(pc.normals_); },
                    [](geometry::PointCloud& pc, const py::object& o) { set_vec(pc.normals_, o); })
            .def_property(
                    "colors", [](const geometry::PointCloud& pc) { return wrap(pc.colors_); },
                    [](geometry::PointCloud& pc, const py::object& o) { set_vec(pc.colors_, o); })
            .def("to_points_dlpack", [](geometry::PointCloud& pc) { return to_dlpack_capsule(pc.points_); })
            .def("to_normals_dlpack", [](geometry::PointCloud& pc) { return to_dlpack_capsule(pc.normals_); })
            .def("to_colors_dlpack", [](geometry::PointCloud& pc) { return to_dlpack_capsule(pc.colors_); })
            .def("from_points_dlpack", [](geometry::PointCloud& pc, py::capsule c) { from_dlpack_capsule(c, pc.points_); })
            .def("from_normals_dlpack", [](geometry::PointCloud& pc, py::capsule c) { from_dlpack_capsule(c, pc.normals_); })
            .def("from_colors_dlpack", [](geometry::PointCloud& pc, py::capsule c) { from_dlpack_capsule(c, pc.colors_); })
            .def("has_points", &geometry::PointCloud::HasPoints)
            .def("has_normals", &geometry::PointCloud::HasNormals)
            .def("has_colors", &geometry::PointCloud::HasColors)
            .def("has_covariances", &geometry::PointCloud::HasCovariances)
            .def("is_empty", &geometry::PointCloud::IsEmpty)
            .def("clear", [](geometry::PointCloud& pc) { pc.Clear(); })
            .def("get_min_bound", [](const geometry::PointCloud& pc) { return from_vector3(pc.GetMinBound()); })
            .def("get_max_bound", [](const geometry::PointCloud& pc) { return from_vector3(pc.GetMaxBound()); })
            .def("get_center", [](const geometry::PointCloud& pc) { return from_vector3(pc.GetCenter()); })
            .def("transform",
                 [](std::shared_ptr<geometry::PointCloud> pc, const farray& T) {
                     pc->Transform(to_matrix4(T));
                     return pc;
                 },
                 "transformation"_a)
            .def("translate",
                 [](std::shared_ptr<geometry::PointCloud> pc, const farray& t, bool relative) {
                     pc->Translate(to_vector3(t), relative);
                     return pc;
                 },
                 "translation"_a, "relative"_a = true)
            .def("scale",
                 [](std::shared_ptr<geometry::PointCloud> pc, float s, bool center) {
                     pc->Scale(s, center);
                     return pc;
                 },
                 "scale"_a, "center"_a = true)
            .def("voxel_down_sample", &geometry::PointCloud::VoxelDownSample, "voxel_size"_a)
            .def(
                    "select_by_index",
                    [](const geometry::PointCloud& pc, const py::object& indices, bool invert) {
                        if (py::isinstance<ULongVector>(indices))
                            return pc.SelectByIndex(indices.cast<const ULongVector&>().data, invert);
                        return pc.SelectByIndex(
                                ULongVector(indices.cast<py::array_t<int64_t, py::array::c_style | py::array::forcecast>>())
                                        .data,
                                invert);
                    },
                    "indices"_a, "invert"_a = false)
            .def(
                    "select_by_mask",
                    [](const geometry::PointCloud& pc, const py::object& mask, bool invert) {
                        if (py::isinstance<BoolVector>(mask)) return pc.SelectByMask(mask.cast<const BoolVector&>().data, invert);
                        return pc.SelectByMask(
                                BoolVector(mask.cast<py::array_t<bool, py::array::c_style | py::array::forcecast>>()).data, invert);
                    },
                    "mask"_a, "invert"_a = false)
            .def("uniform_down_sample", &geometry::PointCloud::UniformDownSample, "every_k_points"_a)
            .def("get_axis_aligned_bounding_box",
                 [](const geometry::PointCloud& pc) {
                     return std::make_shared<geometry::AxisAlignedBoundingBox3>(pc.GetAxisAlignedBoundingBox());
                 })
            .def("farthest_point_down_sample", &geometry::PointCloud::FarthestPointDownSample, "num_samples"_a)
            .def("gaussian_filter", &geometry::PointCloud::GaussianFilter, "search_radius"_a, "sigma2"_a,
                 "num_max_search_points"_a = 50)
            .def("pass_through_filter", &geometry::PointCloud::PassThroughFilter, "axis_no"_a, "min_bound"_a, "max_bound"_a)
            .def("crop", &geometry::PointCloud::Crop, "bounding_box"_a)
            .def("remove_none_finite_points",
                 [](std::shared_ptr<geometry::PointCloud> pc, bool remove_nan, bool remove_infinite) {
                     pc->RemoveNoneFinitePoints(remove_nan, remove_infinite);
                     return pc;
                 },
                 "remove_nan"_a = true, "remove_infinite"_a = true)
            .def(
                    "remove_radius_outlier",
                    [](const geometry::PointCloud& pc, size_t nb_points, float search_radius) {
                        auto res = pc.RemoveRadiusOutliers(nb_points, search_radius);
                        ULongVector idx;
                        idx.data = std::move(std::get<1>(res));
                        return std::make_tuple(std::get<0>(res), idx);
                    },
                    "nb_points"_a, "radius"_a)
            .def(
                    "remove_statistical_outlier",
                    [](const geometry::PointCloud& pc, size_t nb_neighbors, float std_ratio) {
                        auto res = pc.RemoveStatisticalOutliers(nb_neighbors, std_ratio);
                        ULongVector idx;
                        idx.data = std::move(std::get<1>(res));
                        return std::make_tuple(std::get<0>(res), idx);
                    },
                    "nb_neighbors"_a, "std_ratio"_a)
            .def(
                    "cluster_dbscan",
                    [](const geometry::PointCloud& pc, float eps, size_t min_points, bool print_progress,
                       size_t max_edges) {
                        IntVector labels;
                        labels.data = std::move(*pc.ClusterDBSCAN(eps, min_points, print_progress, max_edges));
                        return labels;
                    },
                    "eps"_a, "min_points"_a, "print_progress"_a = false, "max_edges"_a = knn::NUM_MAX_NN)
            .def(
                    "segment_plane",
                    [](const geometry::PointCloud& pc, float distance_threshold, size_t ransac_n, size_t num_iterations) {
                        auto res = pc.SegmentPlane(distance_threshold, ransac_n, num_iterations);
                        ULongVector idx;
                        idx.data = std::move(std::get<1>(res));
                        const Eigen::Vector4f& v = std::get<0>(res);
                        py::array_t<float> plane(4);
                        for (int k = 0; k < 4; ++k) plane.mutable_at(k) = v(k);
                        return std::make_tuple(plane, idx);
                    },
                    "distance_threshold"_a = 0.01f, "ransac_n"_a = 3, "num_iterations"_a = 100)
            .def("estimate_normals", &geometry::PointCloud::EstimateNormals,
                 "search_param"_a = knn::KDTreeSearchParamKNN())
            .def_static("create_from_occupancy_grid", &geometry::PointCloud::CreateFromOccupancyGrid, "occgrid"_a)
            .def("__len__", [](const geometry::PointCloud& pc) { return pc.points_.size(); });

    // geometry.keypoint (geometry/keypoint.cpp; the reference spells the last keyword "max_neighbots")
    py::module mk = mg.def_submodule("keypoint", "Keypoint Detectors.");
    mk.def(
            "compute_iss_keypoints",
            [](const geometry::PointCloud& input, float salient_radius, float non_max_radius, float gamma_21, float gamma_32,
               int min_neighbors, int max_neighbors) {
                auto res = geometry::keypoint::ComputeISSKeypoints(input, salient_radius, non_max_radius, gamma_21, gamma_32,
                                                                   min_neighbors, max_neighbors);
                BoolVector mask;
                mask.data = std::move(*std::get<1>(res));
                return std::make_tuple(std::get<0>(res), mask);
            },
            "input"_a, "salient_radius"_a = 0.0f, "non_max_radius"_a = 0.0f, "gamma_21"_a = 0.975f, "gamma_32"_a = 0.975f,
            "min_neighbors"_a = 5, "max_neighbors"_a = knn::NUM_MAX_NN);

    // geometry.Image / geometry.RGBDImage (cupoch_pybind/geometry/image.cpp) with the reference's names and defaults.  As
    // there, filter, bilateral_filter and create_pyramid first make a float image of anything that is not 1 x float32.
    // The reference's module names ImageColorToIntensityConversionType's two values Gaussian3 and Gaussian5; Equal and
    // Weighted are the values, the two misnomers stay as attributes.
    typedef geometry::Image Img;
    py::enum_<Img::FilterType>(mg, "ImageFilterType", "Enum class for Image filter types.")
            .value("Gaussian3", Img::FilterType::Gaussian3)
            .value("Gaussian5", Img::FilterType::Gaussian5)
            .value("Gaussian7", Img::FilterType::Gaussian7)
            .value("Sobel3dx", Img::FilterType::Sobel3Dx)
            .value("Sobel3dy", Img::FilterType::Sobel3Dy)
            .export_values();
    py::enum_<Img::ColorToIntensityConversionType> c2i(mg, "ImageColorToIntensityConversionType");
    c2i.value("Equal", Img::ColorToIntensityConversionType::Equal).value("Weighted", Img::ColorToIntensityConversionType::Weighted);
    c2i.attr("Gaussian3") = c2i.attr("Equal");
    c2i.attr("Gaussian5") = c2i.attr("Weighted");
    auto as_float = [](const Img& im) { return im.num_of_channels_ != 1 || im.bytes_per_channel_ != 4 ? im.CreateFloatImage() : std::make_shared<Img>(im); };
    py::class_<Img, std::shared_ptr<Img>>(mg, "Image", "The image class stores image with customizable width, height, num of channels and bytes per channel.")
            .def(py::init<>())
            .def(py::init([](const py::array& a) { return std::make_shared<Img>(image_from_array(a)); }), "array"_a)
            .def("__repr__", [](const Img& im) {
                return std::string("Image of size ") + std::to_string(im.width_) + "x" + std::to_string(im.height_) + ", with " +
                       std::to_string(im.num_of_channels_) + " channels.";
            })
            .def("__array__", [](const Img& im, const py::object&, const py::object&) -> py::array {
                const char* kind = im.bytes_per_channel_ == 1 ? "uint8" : (im.bytes_per_channel_ == 2 ? "uint16" : "float32");
                std::vector<py::ssize_t> shape = {im.height_, im.width_};
                if (im.num_of_channels_ != 1) shape.push_back(im.num_of_channels_);
                if (im.IsEmpty() || (im.bytes_per_channel_ != 1 && im.bytes_per_channel_ != 2 && im.bytes_per_channel_ != 4))
                    return py::array(py::dtype("uint8"), std::vector<py::ssize_t>{0, 0});
                py::array out(py::dtype(kind), shape);
                const std::vector<uint8_t> h = im.GetData();
                std::memcpy(out.mutable_data(), h.data(), h.size());
                return out;
            }, "dtype"_a = py::none(), "copy"_a = py::none())
            .def("clip_intensity", [](std::shared_ptr<Img> im, float lo, float hi) { im->ClipIntensity(lo, hi); return im; },
                 "Function to clip intensity", "min"_a = 0.0, "max"_a = 1.0)
            .def("linear_transform", [](std::shared_ptr<Img> im, float scale, float offset) { im->LinearTransform(scale, offset); return im; },
                 "Function to transform linearly", "scale"_a = 1.0, "offset"_a = 0.0)
            .def("downsample", &Img::Downsample)
            .def("filter", [as_float](const Img& im, Img::FilterType t) { return as_float(im)->Filter(t); }, "Function to filter Image", "filter_type"_a)
            .def("flip_vertical", &Img::FlipVertical, "Function to flip image vertically (upside down)")
            .def("flip_horizontal", &Img::FlipHorizontal, "Function to flip image horizontally (from left to right)")
            .def("transpose", &Img::Transpose)
            .def("bilateral_filter", [as_float](const Img& im, int diameter, float sigma_color, float sigma_space) {
                return as_float(im)->BilateralFilter(diameter, sigma_color, sigma_space);
            }, "Function to apply bilateral filter to the image", "diameter"_a, "sigma_color"_a, "sigma_space"_a)
            .def("create_gray_image", &Img::CreateGrayImage, "Create gray image.", "type"_a = Img::ColorToIntensityConversionType::Weighted)
            .def("create_float_image", &Img::CreateFloatImage, "Create float gray image.", "type"_a = Img::ColorToIntensityConversionType::Weighted)
            .def("convert_depth_to_float_image", &Img::ConvertDepthToFloatImage, "depth_scale"_a = 1000.0, "depth_trunc"_a = 3.0)
            .def("create_pyramid", [as_float](const Img& im, size_t n, bool g) { return as_float(im)->CreatePyramid(n, g); },
                 "Function to create ImagePyramid", "num_of_levels"_a, "with_gaussian_filter"_a)
            .def_static("filter_pyramid", &Img::FilterPyramid, "Function to filter ImagePyramid", "image_pyramid"_a, "filter_type"_a)
            .def_static("bilateral_filter_pyramid", &Img::BilateralFilterPyramid, "Function to filter ImagePyramid", "image_pyramid"_a,
                        "diameter"_a, "sigma_color"_a, "sigma_space"_a)
            .def_readonly("width", &Img::width_)
            .def_readonly("height", &Img::height_)
            .def_readonly("num_of_channels", &Img::num_of_channels_)
            .def_readonly("bytes_per_channel", &Img::bytes_per_channel_)
            .def("is_empty", &Img::IsEmpty);
    typedef geometry::RGBDImage Rgbd;
    py::class_<Rgbd, std::shared_ptr<Rgbd>>(mg, "RGBDImage", "RGBDImage is for a pair of registered color and depth images, viewed from the same "
                                                             "view, of the same resolution. If you have other format, convert it first.")
            .def(py::init<>())
            .def(py::init<const Img&, const Img&>(), "color"_a, "depth"_a)
            .def_readwrite("color", &Rgbd::color_)
            .def_readwrite("depth", &Rgbd::depth_)
            .def("__repr__", [](const Rgbd& r) {
                auto one = [](const Img& im) { return std::to_string(im.width_) + "x" + std::to_string(im.height_) + ", with " + std::to_string(im.num_of_channels_) + " channels.\n"; };
                return std::string("RGBDImage of size \nColor image : ") + one(r.color_) + "Depth image : " + one(r.depth_) + "Use numpy.asarray to access buffer data.";
            })
            .def("is_empty", &Rgbd::IsEmpty)
            .def("create_pyramid", &Rgbd::CreatePyramid, "num_of_levels"_a, "with_gaussian_filter_for_color"_a = true,
                 "with_gaussian_filter_for_depth"_a = false)
            .def_static("filter_pyramid", &Rgbd::FilterPyramid, "rgbd_image_pyramid"_a, "filter_type"_a)
            .def_static("bilateral_filter_pyramid_depth", &Rgbd::BilateralFilterPyramidDepth, "rgbd_image_pyramid"_a, "diameter"_a,
                        "sigma_depth"_a, "sigma_space"_a)
            .def_static("create_from_color_and_depth", &Rgbd::CreateFromColorAndDepth, "Function to make RGBDImage from color and depth image",
                        "color"_a, "depth"_a, "depth_scale"_a = 1000.0, "depth_trunc"_a = 3.0, "convert_rgb_to_intensity"_a = true)
            .def_static("create_from_redwood_format", &Rgbd::CreateFromRedwoodFormat, "Function to make RGBDImage (for Redwood format)",
                        "color"_a, "depth"_a, "convert_rgb_to_intensity"_a = true)
            .def_static("create_from_tum_format", &Rgbd::CreateFromTUMFormat, "Function to make RGBDImage (for TUM format)", "color"_a,
                        "depth"_a, "convert_rgb_to_intensity"_a = true)
            .def_static("create_from_sun_format", &Rgbd::CreateFromSUNFormat, "Function to make RGBDImage (for SUN format)", "color"_a,
                        "depth"_a, "convert_rgb_to_intensity"_a = true)
            .def_static("create_from_nyu_format", &Rgbd::CreateFromNYUFormat, "Function to make RGBDImage (for NYU format)", "color"_a,
                        "depth"_a, "convert_rgb_to_intensity"_a = true);

    // geometry.OccupancyVoxel / geometry.OccupancyGrid (cupoch_pybind/geometry/occupancygrid.cpp) with the reference's
    // names, defaults and read-write attributes.  Not bound, as not built: create_from_voxel_grid.
    py::class_<geometry::OccupancyVoxel, std::shared_ptr<geometry::OccupancyVoxel>>(mg, "OccupancyVoxel")
            .def(py::init<>())
            .def(py::init([](const py::array_t<int, py::array::c_style | py::array::forcecast>& g) {
                     return std::make_shared<geometry::OccupancyVoxel>(to_vector3i(g));
                 }),
                 "grid_index"_a)
            .def(py::init([](const py::array_t<int, py::array::c_style | py::array::forcecast>& g, float prob_log) {
                     return std::make_shared<geometry::OccupancyVoxel>(to_vector3i(g), prob_log);
                 }),
                 "grid_index"_a, "prob_log"_a)
            .def(py::init([](const py::array_t<int, py::array::c_style | py::array::forcecast>& g, float prob_log,
                             const farray& color) {
                     return std::make_shared<geometry::OccupancyVoxel>(to_vector3i(g), prob_log, to_vector3(color));
                 }),
                 "grid_index"_a, "prob_log"_a, "color"_a)
            .def("__repr__",
                 [](const geometry::OccupancyVoxel& v) {
                     std::ostringstream repr;
                     repr << "geometry::OccupancyVoxel with grid_index: (" << v.grid_index_(0) << ", " << v.grid_index_(1) << ", "
                          << v.grid_index_(2) << "), prob_log: " << v.prob_log_ << ", color: (" << v.color_(0) << ", "
                          << v.color_(1) << ", " << v.color_(2) << ")";
                     return repr.str();
                 })
            .def_property(
                    "grid_index",
                    [](const geometry::OccupancyVoxel& v) {
                        py::array_t<int> a(3);
                        for (int k = 0; k < 3; ++k) a.mutable_at(k) = (int)v.grid_index_(k);
                        return a;
                    },
                    [](geometry::OccupancyVoxel& v, const py::array_t<int, py::array::c_style | py::array::forcecast>& g) {
                        const Eigen::Vector3i i = to_vector3i(g);
                        for (int k = 0; k < 3; ++k) v.grid_index_(k) = (unsigned short)i(k);
                    })
            .def_readwrite("prob_log", &geometry::OccupancyVoxel::prob_log_)
            .def_property(
                    "color", [](const geometry::OccupancyVoxel& v) { return from_vector3(v.color_); },
                    [](geometry::OccupancyVoxel& v, const farray& c) { v.color_ = to_vector3(c); });

    py::class_<geometry::OccupancyGrid, std::shared_ptr<geometry::OccupancyGrid>>(mg, "OccupancyGrid")
            .def(py::init<>())
            .def(py::init([](float voxel_size, int resolution) {
                     return std::make_shared<geometry::OccupancyGrid>(voxel_size, (size_t)resolution);
                 }),
                 "voxel_size"_a, "resolution"_a)
            .def(py::init([](float voxel_size, int resolution, const farray& origin) {
                     return std::make_shared<geometry::OccupancyGrid>(voxel_size, (size_t)resolution, to_vector3(origin));
                 }),
                 "voxel_size"_a, "resolution"_a, "origin"_a)
            .def("__repr__",
                 [](const geometry::OccupancyGrid& g) {
                     return std::string("geometry::OccupancyGrid with ") + std::to_string(g.ExtractKnownVoxels()->size()) +
                            " voxels.";
                 })
            .def_property_readonly("voxels", [](const geometry::OccupancyGrid& g) { return voxel_list(*g.ExtractKnownVoxels()); })
            .def("extract_known_voxels", [](const geometry::OccupancyGrid& g) { return voxel_list(*g.ExtractKnownVoxels()); })
            .def("extract_free_voxels", [](const geometry::OccupancyGrid& g) { return voxel_list(*g.ExtractFreeVoxels()); })
            .def("extract_occupied_voxels", [](const geometry::OccupancyGrid& g) { return voxel_list(*g.ExtractOccupiedVoxels()); })
            .def("reconstruct", [](geometry::OccupancyGrid& g, float voxel_size, int resolution) { g.Reconstruct(voxel_size, resolution); },
                 "voxel_size"_a, "resolution"_a)
            .def("insert",
                 [](geometry::OccupancyGrid& g, const geometry::PointCloud& pc, const farray& viewpoint, float max_range) {
                     g.Insert(pc, to_vector3(viewpoint), max_range);
                 },
                 "pointcloud"_a, "viewpoint"_a, "max_range"_a = -1.0f)
            .def("add_voxel",
                 [](geometry::OccupancyGrid& g, const py::array_t<int, py::array::c_style | py::array::forcecast>& v,
                    bool occupied) { g.AddVoxel(to_vector3i(v), occupied); },
                 "voxel"_a, "occupied"_a = false)
            .def("set_free_area",
                 [](geometry::OccupancyGrid& g, const farray& lo, const farray& hi) { g.SetFreeArea(to_vector3(lo), to_vector3(hi)); },
                 "min_bound"_a, "max_bound"_a)
            .def("get_voxel",
                 [](const geometry::OccupancyGrid& g, const farray& point) {
                     const auto r = g.GetVoxel(to_vector3(point));
                     return std::make_tuple(std::get<0>(r), std::get<1>(r));
                 },
                 "point"_a)
            .def("is_occupied", [](const geometry::OccupancyGrid& g, const farray& p) { return g.IsOccupied(to_vector3(p)); }, "point"_a)
            .def("is_unknown", [](const geometry::OccupancyGrid& g, const farray& p) { return g.IsUnknown(to_vector3(p)); }, "point"_a)
            .def("clear", [](geometry::OccupancyGrid& g) { g.Clear(); })
            .def("get_min_bound", [](const geometry::OccupancyGrid& g) { return from_vector3(g.GetMinBound()); })
            .def("get_max_bound", [](const geometry::OccupancyGrid& g) { return from_vector3(g.GetMaxBound()); })
            .def("get_center", [](const geometry::OccupancyGrid& g) { return from_vector3(g.GetCenter()); })
            .def("get_voxels",
                 [](const geometry::OccupancyGrid& g) {
                     const std::vector<float> h = g.GetVoxels();
                     py::array_t<float> a((py::ssize_t)h.size());
                     if (!h.empty()) std::memcpy(a.mutable_data(), h.data(), h.size() * sizeof(float));
                     return a;
                 })
            .def_readwrite("voxel_size", &geometry::OccupancyGrid::voxel_size_)
            .def_readwrite("resolution", &geometry::OccupancyGrid::resolution_)
            .def_property(
                    "origin", [](const geometry::OccupancyGrid& g) { return from_vector3(g.origin_); },
                    [](geometry::OccupancyGrid& g, const farray& v) { g.origin_ = to_vector3(v); })
            .def_readwrite("clamping_thres_min", &geometry::OccupancyGrid::clamping_thres_min_)
            .def_readwrite("clamping_thres_max", &geometry::OccupancyGrid::clamping_thres_max_)
            .def_readwrite("prob_hit_log", &geometry::OccupancyGrid::prob_hit_log_)
            .def_readwrite("prob_miss_log", &geometry::OccupancyGrid::prob_miss_log_)
            .def_readwrite("occ_prob_thres_log", &geometry::OccupancyGrid::occ_prob_thres_log_)
            .def_readwrite("visualize_free_area", &geometry::OccupancyGrid::visualize_free_area_);

    // ---------------------------------------------------------------- camera
    py::module mc = m.def_submodule("camera");
    py::class_<camera::PinholeCameraIntrinsic>(mc, "PinholeCameraIntrinsic")
            .def(py::init<>())
            .def(py::init<int, int, float, float, float, float>(), "width"_a, "height"_a, "fx"_a, "fy"_a, "cx"_a, "cy"_a)
            .def("set_intrinsics", &camera::PinholeCameraIntrinsic::SetIntrinsics, "width"_a, "height"_a, "fx"_a, "fy"_a,
                 "cx"_a, "cy"_a)
            .def("get_focal_length", &camera::PinholeCameraIntrinsic::GetFocalLength)
            .def("get_principal_point", &camera::PinholeCameraIntrinsic::GetPrincipalPoint)
            .def("is_valid", &camera::PinholeCameraIntrinsic::IsValid)
            .def("create_pyramid_level", &camera::PinholeCameraIntrinsic::CreatePyramidLevel, "level"_a)
            .def_readwrite("width", &camera::PinholeCameraIntrinsic::width_)
            .def_readwrite("height", &camera::PinholeCameraIntrinsic::height_);

    py::class_<camera::PinholeCameraParameters>(mc, "PinholeCameraParameters")
            .def(py::init<>())
            .def_readwrite("intrinsic", &camera::PinholeCameraParameters::intrinsic_)
            .def_property(
                    "extrinsic", [](const camera::PinholeCameraParameters& p) { return from_matrix4(p.extrinsic_); },
                    [](camera::PinholeCameraParameters& p, const farray& e) { p.extrinsic_ = to_matrix4(e); })
            .def("__repr__", [](const camera::PinholeCameraParameters&) {
                return std::string("camera::PinholeCameraParameters class.\nAccess its data via intrinsic and extrinsic.");
            });

    // geometry.Voxel / geometry.VoxelGrid (cupoch_pybind/geometry/voxelgrid.cpp) with the reference's names, argument
    // names and defaults.  Not bound, as not built: create_from_triangle_mesh[_within_bounds],
    // get_oriented_bounding_box.
    using iarray = py::array_t<int, py::array::c_style | py::array::forcecast>;
    py::class_<DeviceVoxelMap>(mg, "DeviceVoxelMap")
            .def(py::init<>())
            .def(py::init<const iarray&, const farray&>(), "grid_index"_a, "color"_a)
            .def("__len__", [](const DeviceVoxelMap& v) { return v.keys.size(); })
            .def("cpu", &DeviceVoxelMap::cpu);
    py::class_<geometry::Voxel, std::shared_ptr<geometry::Voxel>>(mg, "Voxel")
            .def(py::init<>())
            .def(py::init([](const geometry::Voxel& v) { return std::make_shared<geometry::Voxel>(v); }))
            .def("__repr__",
                 [](const geometry::Voxel& voxel) {
                     std::ostringstream repr;
                     repr << "geometry::Voxel with grid_index: (" << voxel.grid_index_(0) << ", " << voxel.grid_index_(1) << ", "
                          << voxel.grid_index_(2) << "), color: (" << voxel.color_(0) << ", " << voxel.color_(1) << ", "
                          << voxel.color_(2) << ")";
                     return repr.str();
                 })
            .def(py::init([](const iarray& g) { return std::make_shared<geometry::Voxel>(to_vector3i(g)); }), "grid_index"_a)
            .def(py::init([](const iarray& g, const farray& c) { return std::make_shared<geometry::Voxel>(to_vector3i(g), to_vector3(c)); }),
                 "grid_index"_a, "color"_a)
            .def_property(
                    "grid_index",
                    [](const geometry::Voxel& v) {
                        py::array_t<int> a(3);
                        for (int k = 0; k < 3; ++k) a.mutable_at(k) = v.grid_index_(k);
                        return a;
                    },
                    [](geometry::Voxel& v, const iarray& g) { v.grid_index_ = to_vector3i(g); })
            .def_property(
                    "color", [](const geometry::Voxel& v) { return from_vector3(v.color_); },
                    [](geometry::Voxel& v, const farray& c) { v.color_ = to_vector3(c); });

    py::class_<geometry::VoxelGrid, std::shared_ptr<geometry::VoxelGrid>>(mg, "VoxelGrid")
            .def(py::init<>())
            .def(py::init([](const geometry::VoxelGrid& g) { return std::make_shared<geometry::VoxelGrid>(g); }))
            .def("__repr__",
                 [](const geometry::VoxelGrid& g) {
                     return std::string("geometry::VoxelGrid with ") + std::to_string(g.voxels_keys_.size()) + " voxels.";
                 })
            .def_property(
                    "voxels",
                    [](const geometry::VoxelGrid& g) {
                        DeviceVoxelMap w;
                        w.keys = g.voxels_keys_;
                        w.values = g.voxels_values_;
                        return w;
                    },
                    [](geometry::VoxelGrid& g, const DeviceVoxelMap& w) { g.SetVoxels(w.keys.to_host(), w.values.to_host()); })
            .def("__add__", [](const geometry::VoxelGrid& a, const geometry::VoxelGrid& b) { return std::make_shared<geometry::VoxelGrid>(a + b); })
            .def("__iadd__",
                 [](std::shared_ptr<geometry::VoxelGrid> a, const geometry::VoxelGrid& b) {
                     *a += b;
                     return a;
                 })
            .def("has_colors", &geometry::VoxelGrid::HasColors)
            .def("has_voxels", &geometry::VoxelGrid::HasVoxels)
            .def("is_empty", &geometry::VoxelGrid::IsEmpty)
            .def("clear", [](geometry::VoxelGrid& g) { g.Clear(); })
            .def("get_voxel",
                 [](const geometry::VoxelGrid& g, const farray& point) {
                     const Eigen::Vector3i i = g.GetVoxel(to_vector3(point));
                     py::array_t<int> a(3);
                     for (int k = 0; k < 3; ++k) a.mutable_at(k) = i(k);
                     return a;
                 },
                 "point"_a)
            .def("get_voxel_center_coordinate",
                 [](const geometry::VoxelGrid& g, const iarray& idx) { return from_vector3(g.GetVoxelCenterCoordinate(to_vector3i(idx))); }, "idx"_a)
            .def("add_voxel", [](geometry::VoxelGrid& g, const geometry::Voxel& v) { g.AddVoxel(v); }, "voxel"_a)
            .def("add_voxels", [](geometry::VoxelGrid& g, const std::vector<geometry::Voxel>& v) { g.AddVoxels(v); }, "voxels"_a)
            .def("paint_uniform_color", [](std::shared_ptr<geometry::VoxelGrid> g, const farray& color) {
                g->PaintUniformColor(to_vector3(color));
                return g;
            })
            .def("paint_indexed_color", [](std::shared_ptr<geometry::VoxelGrid> g, const ULongVector& indices, const farray& color) {
                g->PaintIndexedColor(indices.data, to_vector3(color));
                return g;
            })
            .def("check_if_included",
                 [](geometry::VoxelGrid& g, const farray& queries) {
                     if (queries.ndim() != 2 || queries.shape(1) != 3) throw std::invalid_argument("expected an (n, 3) float32 array");
                     std::vector<Eigen::Vector3f> q((size_t)queries.shape(0));
                     if (!q.empty()) std::memcpy((void*)q.data(), queries.data(), q.size() * sizeof(Eigen::Vector3f));
                     const std::vector<bool> r = g.CheckIfIncluded(q);
                     py::list out;
                     for (bool b : r) out.append(b);
                     return out;
                 },
                 "queries"_a)
            .def("carve_depth_map",
                 [](std::shared_ptr<geometry::VoxelGrid> g, const geometry::Image& depth_map, const camera::PinholeCameraParameters& p,
                    bool keep) {
                     g->CarveDepthMap(depth_map, p, keep);
                     return g;
                 },
                 "depth_map"_a, "camera_params"_a, "keep_voxels_outside_image"_a = false)
            .def("carve_silhouette",
                 [](std::shared_ptr<geometry::VoxelGrid> g, const geometry::Image& mask, const camera::PinholeCameraParameters& p, bool keep) {
                     g->CarveSilhouette(mask, p, keep);
                     return g;
                 },
                 "silhouette_mask"_a, "camera_params"_a, "keep_voxels_outside_image"_a = false)
            .def("select_by_index",
                 [](geometry::VoxelGrid& g, const ULongVector& indices, bool invert) { return g.SelectByIndex(indices.data, invert); },
                 "indices"_a, "invert"_a = false)
            .def("get_min_bound", [](const geometry::VoxelGrid& g) { return from_vector3(g.GetMinBound()); })
            .def("get_max_bound", [](const geometry::VoxelGrid& g) { return from_vector3(g.GetMaxBound()); })
            .def("get_center", [](const geometry::VoxelGrid& g) { return from_vector3(g.GetCenter()); })
            .def("get_axis_aligned_bounding_box", &geometry::VoxelGrid::GetAxisAlignedBoundingBox)
            .def("translate",
                 [](std::shared_ptr<geometry::VoxelGrid> g, const farray& t, bool relative) {
                     g->Translate(to_vector3(t), relative);
                     return g;
                 },
                 "translation"_a, "relative"_a = true)
            .def("scale",
                 [](std::shared_ptr<geometry::VoxelGrid> g, float s, bool center) {
                     g->Scale(s, center);
                     return g;
                 },
                 "scale"_a, "center"_a = true)
            .def_static(
                    "create_dense",
                    [](const farray& origin, float voxel_size, float width, float height, float depth) {
                        return geometry::VoxelGrid::CreateDense(to_vector3(origin), voxel_size, width, height, depth);
                    },
                    "origin"_a, "voxel_size"_a, "width"_a, "height"_a, "depth"_a)
            .def_static("create_from_point_cloud", &geometry::VoxelGrid::CreateFromPointCloud, "input"_a, "voxel_size"_a)
            .def_static(
                    "create_from_point_cloud_within_bounds",
                    [](const geometry::PointCloud& input, float voxel_size, const farray& lo, const farray& hi) {
                        return geometry::VoxelGrid::CreateFromPointCloudWithinBounds(input, voxel_size, to_vector3(lo), to_vector3(hi));
                    },
                    "input"_a, "voxel_size"_a, "min_bound"_a, "max_bound"_a)
            .def_static("create_from_occupancy_grid", &geometry::VoxelGrid::CreateFromOccupancyGrid, "input"_a)
            .def_property(
                    "origin", [](const geometry::VoxelGrid& g) { return from_vector3(g.origin_); },
                    [](geometry::VoxelGrid& g, const farray& v) { g.origin_ = to_vector3(v); })
            .def_readwrite("voxel_size", &geometry::VoxelGrid::voxel_size_);

    // geometry.DistanceVoxel / geometry.DistanceTransform (cupoch_pybind/geometry/distancetransform.cpp) with the
    // reference's names and defaults, and beside them compute_voronoi_diagram, get_voxel, get_voxels and the DenseGrid
    // members.  get_distances takes a Vector3fVector or an (n, 3) array and returns a numpy array.
    py::class_<geometry::DistanceVoxel, std::shared_ptr<geometry::DistanceVoxel>>(mg, "DistanceVoxel")
            .def(py::init<>())
            .def("__repr__",
                 [](const geometry::DistanceVoxel& v) {
                     std::ostringstream repr;
                     repr << "geometry::DistanceVoxel with nearest_index: (" << v.nearest_index_(0) << ", " << v.nearest_index_(1)
                          << ", " << v.nearest_index_(2) << "), distance: " << v.distance_ << ")";
                     return repr.str();
                 })
            .def_property(
                    "nearest_index",
                    [](const geometry::DistanceVoxel& v) {
                        py::array_t<int> a(3);
                        for (int k = 0; k < 3; ++k) a.mutable_at(k) = (int)v.nearest_index_(k);
                        return a;
                    },
                    [](geometry::DistanceVoxel& v, const iarray& g) {
                        const Eigen::Vector3i i = to_vector3i(g);
                        for (int k = 0; k < 3; ++k) v.nearest_index_(k) = (unsigned short)i(k);
                    })
            .def_readwrite("distance", &geometry::DistanceVoxel::distance_)
            .def("is_not_site", &geometry::DistanceVoxel::IsNotSite);

    py::class_<geometry::DistanceTransform, std::shared_ptr<geometry::DistanceTransform>>(mg, "DistanceTransform")
            .def(py::init<>())
            .def(py::init([](float voxel_size, int resolution, const farray& origin) {
                     return std::make_shared<geometry::DistanceTransform>(voxel_size, (size_t)resolution, to_vector3(origin));
                 }),
                 "voxel_size"_a, "resolution"_a, "origin"_a = from_vector3(Eigen::Vector3f::Zero()))
            .def("__repr__",
                 [](const geometry::DistanceTransform& d) {
                     return std::string("geometry::DistanceTransform with ") + std::to_string(d.resolution_) + " resolution.";
                 })
            .def("reconstruct",
                 [](geometry::DistanceTransform& d, float voxel_size, int resolution) { d.Reconstruct(voxel_size, (size_t)resolution); },
                 "voxel_size"_a, "resolution"_a)
            .def("compute_edt", [](geometry::DistanceTransform& d, const geometry::VoxelGrid& g) { d.ComputeEDT(g); }, "voxelgrid"_a)
            .def("compute_voronoi_diagram", [](geometry::DistanceTransform& d, const geometry::VoxelGrid& g) { d.ComputeVoronoiDiagram(g); },
                 "voxelgrid"_a)
            .def("get_distance", [](const geometry::DistanceTransform& d, const farray& q) { return d.GetDistance(to_vector3(q)); }, "query"_a)
            .def("get_distances",
                 [](const geometry::DistanceTransform& d, const py::object& queries) {
                     utility::device_vector<Eigen::Vector3f> q;
                     set_vec(q, queries);
                     const std::vector<float> h = d.GetDistances(q)->to_host();
                     py::array_t<float> a((py::ssize_t)h.size());
                     if (!h.empty()) std::memcpy(a.mutable_data(), h.data(), h.size() * sizeof(float));
                     return a;
                 },
                 "queries"_a)
            .def("get_voxel",
                 [](const geometry::DistanceTransform& d, const farray& point) {
                     const auto r = d.GetVoxel(to_vector3(point));
                     return std::make_tuple(std::get<0>(r), std::get<1>(r));
                 },
                 "point"_a)
            .def("get_voxels",
                 [](const geometry::DistanceTransform& d) {
                     const std::vector<geometry::DistanceVoxel> h = d.GetVoxels();
                     py::array_t<int> idx({(py::ssize_t)h.size(), (py::ssize_t)3});
                     py::array_t<float> dist((py::ssize_t)h.size());
                     for (size_t i = 0; i < h.size(); ++i) {
                         for (int k = 0; k < 3; ++k) idx.mutable_at(i, k) = h[i].IsNotSite() ? -1 : (int)h[i].nearest_index_(k);
                         dist.mutable_at(i) = h[i].distance_;
                     }
                     return std::make_tuple(idx, dist);
                 })
            .def("clear", [](geometry::DistanceTransform& d) { d.Clear(); })
            .def("get_min_bound", [](const geometry::DistanceTransform& d) { return from_vector3(d.GetMinBound()); })
            .def("get_max_bound", [](const geometry::DistanceTransform& d) { return from_vector3(d.GetMaxBound()); })
            .def("get_center", [](const geometry::DistanceTransform& d) { return from_vector3(d.GetCenter()); })
            .def_static("create_from_occupancy_grid", &geometry::DistanceTransform::CreateFromOccupancyGrid, "input"_a)
            .def_readwrite("voxel_size", &geometry::DistanceTransform::voxel_size_)
            .def_readwrite("resolution", &geometry::DistanceTransform::resolution_)
            .def_property(
                    "origin", [](const geometry::DistanceTransform& d) { return from_vector3(d.origin_); },
                    [](geometry::DistanceTransform& d, const farray& v) { d.origin_ = to_vector3(v); });

    // geometry.LineSet (cupoch_pybind/geometry/lineset.cpp): points / lines / colors as numpy arrays in and out
    typedef py::array_t<int, py::array::c_style | py::array::forcecast> iarray2;
    py::class_<geometry::LineSet<3>, std::shared_ptr<geometry::LineSet<3>>>(mg, "LineSet")
            .def(py::init<>())
            .def(py::init([](const farray& points, const iarray2& lines) {
                     auto l = std::make_shared<geometry::LineSet<3>>();
                     l->points_ = Vector3fVector(points).data;
                     l->lines_ = Vector2iVector(lines).data;
                     return l;
                 }),
                 "points"_a, "lines"_a)
            .def("__repr__", [](const geometry::LineSet<3>& l) { return std::string("geometry::LineSet with ") + std::to_string(l.lines_.size()) + " lines."; })
            .def_property(
                    "points", [](const geometry::LineSet<3>& l) { Vector3fVector v; v.data = l.points_; return v; },
                    [](geometry::LineSet<3>& l, const Vector3fVector& v) { l.points_ = v.data; })
            .def_property(
                    "lines", [](const geometry::LineSet<3>& l) { Vector2iVector v; v.data = l.lines_; return v; },
                    [](geometry::LineSet<3>& l, const Vector2iVector& v) { l.lines_ = v.data; })
            .def_property(
                    "colors", [](const geometry::LineSet<3>& l) { Vector3fVector v; v.data = l.colors_; return v; },
                    [](geometry::LineSet<3>& l, const Vector3fVector& v) { l.colors_ = v.data; })
            .def("has_points", &geometry::LineSet<3>::HasPoints)
            .def("has_lines", &geometry::LineSet<3>::HasLines)
            .def("has_colors", &geometry::LineSet<3>::HasColors)
            .def("is_empty", &geometry::LineSet<3>::IsEmpty)
            .def("clear", [](geometry::LineSet<3>& l) { l.Clear(); })
            .def("get_min_bound", [](const geometry::LineSet<3>& l) { return from_vector3(l.GetMinBound()); })
            .def("get_max_bound", [](const geometry::LineSet<3>& l) { return from_vector3(l.GetMaxBound()); })
            .def("get_center", [](const geometry::LineSet<3>& l) { return from_vector3(l.GetCenter()); })
            .def("get_axis_aligned_bounding_box", &geometry::LineSet<3>::GetAxisAlignedBoundingBox)
            .def("get_line_coordinate",
                 [](const geometry::LineSet<3>& l, size_t i) {
                     const auto p = l.GetLineCoordinate(i);
                     return py::make_tuple(from_vector3(p.first), from_vector3(p.second));
                 },
                 "line_index"_a)
            .def("paint_uniform_color", [](std::shared_ptr<geometry::LineSet<3>> l, const farray& c) { l->PaintUniformColor(to_vector3(c)); return l; }, "color"_a)
            .def("translate", [](std::shared_ptr<geometry::LineSet<3>> l, const farray& t, bool relative) { l->Translate(to_vector3(t), relative); return l; },
                 "translation"_a, "relative"_a = true)
            .def("scale", [](std::shared_ptr<geometry::LineSet<3>> l, float s, bool center) { l->Scale(s, center); return l; }, "scale"_a, "center"_a = true)
            .def("rotate", [](std::shared_ptr<geometry::LineSet<3>> l, const farray& R, bool center) { l->Rotate(to_matrix3(R), center); return l; }, "R"_a, "center"_a = true)
            .def("transform", [](std::shared_ptr<geometry::LineSet<3>> l, const farray& T) { l->Transform(to_matrix4(T)); return l; }, "transformation"_a)
            .def_static("create_from_axis_aligned_bounding_box", &geometry::LineSet<3>::CreateFromAxisAlignedBoundingBox, "box"_a);

    // geometry.Graph (cupoch_pybind/geometry/graph.cpp): the reference's names and defaults over geometry::Graph<3>
    typedef geometry::Graph<3> Graph3;
    py::class_<Graph3, std::shared_ptr<Graph3>, geometry::LineSet<3>>(mg, "Graph")
            .def(py::init<>())
            .def(py::init([](const farray& points) {
                     auto g = std::make_shared<Graph3>();
                     g->points_ = Vector3fVector(points).data;
                     return g;
                 }),
                 "points"_a)
            .def("__repr__", [](const Graph3& g) { return std::string("geometry::Graph with ") + std::to_string(g.points_.size()) + " nodes and " + std::to_string(g.lines_.size()) + " edges."; })
            .def_property(
                    "edges", [](const Graph3& g) { Vector2iVector v; v.data = g.lines_; return v; },
                    [](Graph3& g, const Vector2iVector& v) { g.lines_ = v.data; g.sorted_ = false; })
            .def_property(
                    "edge_weights", [](const Graph3& g) { const std::vector<float> h = g.GetEdgeWeights(); return farray(h.size(), h.data()); },
                    [](Graph3& g, const farray& w) { g.SetEdgeWeights(std::vector<float>(w.data(), w.data() + w.size())); })
            .def_property(
                    "edge_index_offsets", [](const Graph3& g) { const std::vector<int> h = g.GetEdgeIndexOffsets(); return iarray2(h.size(), h.data()); },
                    [](Graph3& g, const iarray2& o) { g.SetEdgeIndexOffsets(std::vector<int>(o.data(), o.data() + o.size())); })
            .def_property(
                    "node_colors", [](const Graph3& g) { Vector3fVector v; v.data = g.node_colors_; return v; },
                    [](Graph3& g, const Vector3fVector& v) { g.node_colors_ = v.data; })
            .def_readwrite("is_directed", &Graph3::is_directed_)
            .def("has_weights", &Graph3::HasWeights)
            .def("has_node_colors", &Graph3::HasNodeColors)
            .def("is_constructed", &Graph3::IsConstructed)
            .def("construct_graph", [](std::shared_ptr<Graph3> g, bool from_distance) { g->ConstructGraph(from_distance); return g; },
                 "set_edge_weights_from_distance"_a = true)
            .def("connect_to_nearest_neighbors", [](std::shared_ptr<Graph3> g, float d, size_t k) { g->ConnectToNearestNeighbors(d, k); return g; },
                 "max_edge_distance"_a, "max_num_edges"_a = 30)
            .def("add_node_and_connect", [](std::shared_ptr<Graph3> g, const farray& p, float d, bool lazy) { g->AddNodeAndConnect(to_vector3(p), d, lazy); return g; },
                 "point"_a, "max_edge_distance"_a = 0.0f, "lazy_add"_a = false)
            .def("add_edge", [](std::shared_ptr<Graph3> g, const iarray2& e, float w, bool lazy) { g->AddEdge(Eigen::Vector2i(e.data()[0], e.data()[1]), w, lazy); return g; },
                 "edge"_a, "weight"_a = 1.0f, "lazy_add"_a = false)
            .def("add_edges",
                 [](std::shared_ptr<Graph3> g, const Vector2iVector& e, const farray& w, bool lazy) {
                     g->AddEdges(e.data, utility::device_vector<float>(std::vector<float>(w.data(), w.data() + w.size())), lazy);
                     return g;
                 },
                 "edges"_a, "weights"_a = farray(0), "lazy_add"_a = false)
            .def("remove_edge", [](std::shared_ptr<Graph3> g, const iarray2& e) { g->RemoveEdge(Eigen::Vector2i(e.data()[0], e.data()[1])); return g; }, "edge"_a)
            .def("remove_edges", [](std::shared_ptr<Graph3> g, const Vector2iVector& e) { g->RemoveEdges(e.data); return g; }, "edges"_a)
            .def("paint_edge_color", [](std::shared_ptr<Graph3> g, const iarray2& e, const farray& c) { g->PaintEdgeColor(Eigen::Vector2i(e.data()[0], e.data()[1]), to_vector3(c)); return g; },
                 "edge"_a, "color"_a)
            .def("paint_edges_color", [](std::shared_ptr<Graph3> g, const Vector2iVector& e, const farray& c) { g->PaintEdgesColor(e.data.to_host(), to_vector3(c)); return g; },
                 "edges"_a, "color"_a)
            .def("paint_node_color", [](std::shared_ptr<Graph3> g, int node, const farray& c) { g->PaintNodeColor(node, to_vector3(c)); return g; }, "node"_a, "color"_a)
            .def("paint_nodes_color", [](std::shared_ptr<Graph3> g, const std::vector<int>& nodes, const farray& c) { g->PaintNodesColor(nodes, to_vector3(c)); return g; },
                 "nodes"_a, "color"_a)
            .def("set_edge_weights_from_distance", [](std::shared_ptr<Graph3> g) { g->SetEdgeWeightsFromDistance(); return g; })
            .def("set_edge_weights", [](std::shared_ptr<Graph3> g, const Vector2iVector& e, float w) { g->SetEdgeWeights(e.data, w); return g; }, "edges"_a, "weight"_a)
            .def("dijkstra_paths",
                 [](const Graph3& g, int start, int end) {
                     const auto res = g.DijkstraPathsHost(start, end);
                     farray dist(res->size());
                     iarray2 prev(res->size());
                     for (size_t i = 0; i < res->size(); ++i) {
                         dist.mutable_data()[i] = (*res)[i].shortest_distance_;
                         prev.mutable_data()[i] = (*res)[i].prev_index_;
                     }
                     return py::make_tuple(dist, prev);
                 },
                 "start_node_index"_a, "end_node_index"_a = -1)
            .def("dijkstra_path",
                 [](const Graph3& g, int start, int end) {
                     const auto p = g.DijkstraPath(start, end);
                     return py::make_tuple(*p.first, p.second);
                 },
                 "start_node_index"_a, "end_node_index"_a)
            .def("to_edges_dlpack", [](Graph3& g) { return to_dlpack_capsule(g.lines_, 2, kMiDLInt); })
            .def("from_edges_dlpack", [](Graph3& g, py::capsule c) { from_dlpack_capsule(c, g.lines_, 2, kMiDLInt); g.sorted_ = false; })
            .def_static("create_from_axis_aligned_bounding_box",
                        [](const geometry::AxisAlignedBoundingBox3& box, const iarray2& res) {
                            return Graph3::CreateFromAxisAlignedBoundingBox(box, Eigen::Vector3i(res.data()[0], res.data()[1], res.data()[2]));
                        },
                        "bbox"_a, "resolutions"_a)
            .def_static("create_from_axis_aligned_bounding_box",
                        [](const farray& lo, const farray& hi, const iarray2& res) {
                            return Graph3::CreateFromAxisAlignedBoundingBox(to_vector3(lo), to_vector3(hi), Eigen::Vector3i(res.data()[0], res.data()[1], res.data()[2]));
                        },
                        "min_bound"_a, "max_bound"_a, "resolutions"_a);

    // geometry.LaserScanBuffer (cupoch_pybind/geometry/laserscanbuffer.cpp): the reference's names and defaults, except
    // min_angle, which is -pi here (the reference's binding says +pi: with max_angle = +pi an empty angle range).  Scans go
    // in and come out as numpy float32 arrays; `ranges` / `intensities` are the live scans, oldest first.
    typedef geometry::LaserScanBuffer Scan;
    auto scan_rows = [](const std::vector<float>& h) { return farray(h.size(), h.data()); };
    auto scan_add = [](std::shared_ptr<Scan> s, const farray& ranges, const farray& T, const farray& intensities) {
        s->AddRanges(std::vector<float>(ranges.data(), ranges.data() + ranges.size()), to_matrix4(T),
                     std::vector<float>(intensities.data(), intensities.data() + intensities.size()));
        return s;
    };
    py::class_<Scan, std::shared_ptr<Scan>>(mg, "LaserScanBuffer", "LaserScanBuffer define a sets of scan from a planar laser range-finder.")
            .def(py::init<int, int, float, float>(), "Create a LaserScanBuffer from given a number of points and angle ranges "
                 "(min_angle defaults to -pi; the reference's +pi makes an empty angle range)",
                 "num_steps"_a, "num_max_scans"_a = 10, "min_angle"_a = (float)-M_PI, "max_angle"_a = (float)M_PI)
            .def("__repr__", [](const Scan& s) { return std::string("geometry::LaserScanBuffer with ") + std::to_string(s.GetNumScans()) + " scans of " + std::to_string(s.num_steps_) + " steps."; })
            .def("is_full", &Scan::IsFull)
            .def("is_empty", &Scan::IsEmpty)
            .def("has_intensities", &Scan::HasIntensities)
            .def("get_angle_increment", &Scan::GetAngleIncrement)
            .def("clear", [](std::shared_ptr<Scan> s) { s->Clear(); return s; })
            .def("add_ranges", scan_add, "Add single scan ranges", "ranges"_a, "transformation"_a = identity4(), "intensities"_a = farray(0))
            .def("add_host_ranges", scan_add, "Add host single scan ranges", "ranges"_a, "transformation"_a = identity4(),
                 "intensities"_a = farray(0))
            .def("merge", [](std::shared_ptr<Scan> s, const Scan& other) { s->Merge(other); return s; }, "Merge other LaserScanBuffer into this one", "other"_a)
            .def("pop_one_scan", &Scan::PopOneScan, "Pop one scan from the buffer")
            .def("pop_host_one_scan",
                 [scan_rows](Scan& s) {
                     auto p = s.PopHostOneScan();
                     return py::make_tuple(scan_rows(*p.first), scan_rows(*p.second));
                 },
                 "Pop host one scan from the buffer")
            .def("range_filter", &Scan::RangeFilter, "min_range"_a, "max_range"_a)
            .def("scan_shadow_filter", &Scan::ScanShadowsFilter,
                 "This filter removes laser readings that are most likely caused by the veiling effect when the edge of an object is being scanned.",
                 "min_angle"_a, "max_angle"_a, "window"_a, "neighbors"_a = 0, "remove_shadow_start_point"_a = false)
            .def("transform", [](std::shared_ptr<Scan> s, const farray& T) { s->Transform(to_matrix4(T)); return s; }, "transformation"_a)
            .def("translate", [](std::shared_ptr<Scan> s, const farray& t, bool relative) { s->Translate(to_vector3(t), relative); return s; },
                 "translation"_a, "relative"_a = true)
            .def("rotate", [](std::shared_ptr<Scan> s, const farray& R, bool center) { s->Rotate(to_matrix3(R), center); return s; }, "R"_a, "center"_a = true)
            .def("scale", [](std::shared_ptr<Scan> s, float k, bool center) { s->Scale(k, center); return s; }, "scale"_a, "center"_a = true)
            .def("get_min_bound", [](const Scan& s) { return from_vector3(s.GetMinBound()); })
            .def("get_max_bound", [](const Scan& s) { return from_vector3(s.GetMaxBound()); })
            .def("get_center", [](const Scan& s) { return from_vector3(s.GetCenter()); })
            .def("get_axis_aligned_bounding_box", &Scan::GetAxisAlignedBoundingBox)
            .def_static("create_from_point_cloud", &Scan::CreateFromPointCloud, "Create a LaserScanBuffer from a point cloud", "pcd"_a,
                        "angle_increment"_a, "min_height"_a, "max_height"_a, "num_vertical_divisions"_a = 1, "min_range"_a = 0.0,
                        "max_range"_a = std::numeric_limits<float>::infinity(), "min_angle"_a = (float)-M_PI, "max_angle"_a = (float)M_PI)
            .def_static("create_from_depth_image", &Scan::CreateFromDepthImage, "Create a LaserScanBuffer from a depth image", "depth"_a,
                        "intrinsic"_a, "angle_increment"_a, "min_y"_a, "max_y"_a, "num_vertical_divisions"_a = 1, "min_range"_a = 0.0,
                        "max_range"_a = std::numeric_limits<float>::infinity(), "min_angle"_a = (float)-M_PI, "max_angle"_a = (float)M_PI,
                        "depth_scale"_a = 1000.0, "depth_trunc"_a = 1000.0, "stride"_a = 1)
            .def_readonly("num_steps", &Scan::num_steps_, "Integer: Number of steps per scan.")
            .def_readonly("num_max_scans", &Scan::num_max_scans_, "Integer: Maximum buffer size.")
            .def_readwrite("min_angle", &Scan::min_angle_)
            .def_readwrite("max_angle", &Scan::max_angle_)
            .def_property_readonly("num_scans", &Scan::GetNumScans, "Integer: Number of scans in the buffer.")
            .def_property_readonly("ranges", [scan_rows](const Scan& s) { return scan_rows(s.GetRanges()); })
            .def_property_readonly("intensities", [scan_rows](const Scan& s) { return scan_rows(s.GetIntensities()); })
            .def_property_readonly("origins", [](const Scan& s) {
                py::list out;
                for (int k = 0; k < s.GetNumScans(); ++k) out.append(from_matrix4(s.origins_[(size_t)((s.top_ + k) % s.num_max_scans_)]));
                return out;
            });
    py::reinterpret_borrow<py::class_<geometry::PointCloud, std::shared_ptr<geometry::PointCloud>>>(mg.attr("PointCloud"))
            .def_static("create_from_laserscanbuffer", &geometry::PointCloud::CreateFromLaserScanBuffer, "scan"_a, "min_range"_a, "max_range"_a)
            // geometry/pointcloud.cpp:296-299
            .def_static("create_from_disparity", &geometry::PointCloud::CreateFromDisparity,
                        "Factory function to create a pointcloud from a disparity image.", "disp"_a, "color"_a, "left_intrinsic"_a,
                        "right_intrinsic"_a, "baseline"_a);

    // ---------------------------------------------------------------- planning (cupoch_pybind/planning)
    py::module mpl = m.def_submodule("planning");
    py::class_<planning::Pos3DPlanner, std::shared_ptr<planning::Pos3DPlanner>>(mpl, "Pos3DPlanner")
            .def(py::init([](const Graph3& graph, float object_radius, float max_edge_distance) {
                     return std::make_shared<planning::Pos3DPlanner>(graph, object_radius, max_edge_distance);
                 }),
                 "graph"_a, "object_radius"_a = 0.1, "max_edge_distance"_a = 1.0)
            .def("add_obstacle", [](std::shared_ptr<planning::Pos3DPlanner> p, std::shared_ptr<geometry::VoxelGrid> o) { p->AddObstacle(o); return p; }, "obstacle"_a)
            .def("add_obstacle", [](std::shared_ptr<planning::Pos3DPlanner> p, std::shared_ptr<geometry::OccupancyGrid> o) { p->AddObstacle(o); return p; }, "obstacle"_a)
            .def("add_obstacle", [](std::shared_ptr<planning::Pos3DPlanner> p, std::shared_ptr<geometry::PointCloud> o) { p->AddObstacle(o); return p; }, "obstacle"_a)
            .def("update_graph", [](std::shared_ptr<planning::Pos3DPlanner> p) { p->UpdateGraph(); return p; })
            .def("find_path",
                 [](const planning::Pos3DPlanner& p, const farray& start, const farray& goal) {
                     const auto path = p.FindPath(to_vector3(start), to_vector3(goal));
                     farray out({(py::ssize_t)path->size(), (py::ssize_t)3});
                     for (size_t i = 0; i < path->size(); ++i)
                         for (int k = 0; k < 3; ++k) out.mutable_data()[i * 3 + (size_t)k] = (*path)[i](k);
                     return out;
                 },
                 "start"_a, "goal"_a)
            .def("get_graph", [](const planning::Pos3DPlanner& p) { return std::make_shared<Graph3>(p.GetGraph()); })
            .def_readwrite("object_radius", &planning::Pos3DPlanner::object_radius_)
            .def_readwrite("max_edge_distance", &planning::Pos3DPlanner::max_edge_distance_);

    // ---------------------------------------------------------------- collision
    // cupoch_pybind/collision: the primitives, PrimitiveArray, CollitionResult (the reference's spelling; CollisionResult
    // names the same class) and compute_intersection / create_voxel_grid.  Not bound, as not built:
    // create_voxel_grid_with_sweeping, create_triangle_mesh, Primitives x Primitives.
    py::module mcol = m.def_submodule("collision");
    py::class_<collision::Primitive, std::shared_ptr<collision::Primitive>> primitive(mcol, "Primitive");
    primitive.def(py::init<>())
            .def("get_axis_aligned_bounding_box", &collision::Primitive::GetAxisAlignedBoundingBox)
            .def_property(
                    "transform", [](const collision::Primitive& p) { return from_matrix4(p.transform_); },
                    [](collision::Primitive& p, const farray& T) { p.transform_ = to_matrix4(T); })
            .def_readonly("type", &collision::Primitive::type_);
    py::enum_<collision::Primitive::PrimitiveType>(primitive, "Type")
            .value("Unspecified", collision::Primitive::PrimitiveType::Unspecified)
            .value("Box", collision::Primitive::PrimitiveType::Box)
            .value("Sphere", collision::Primitive::PrimitiveType::Sphere)
            .value("Capsule", collision::Primitive::PrimitiveType::Capsule)
            .value("Cylinder", collision::Primitive::PrimitiveType::Cylinder)
            .value("Mesh", collision::Primitive::PrimitiveType::Mesh);
    py::class_<collision::Box, std::shared_ptr<collision::Box>, collision::Primitive>(mcol, "Box")
            .def(py::init([](const farray& lengths) { return std::make_shared<collision::Box>(to_vector3(lengths)); }), "lengths"_a)
            .def(py::init([](const farray& lengths, const farray& T) { return std::make_shared<collision::Box>(to_vector3(lengths), to_matrix4(T)); }),
                 "lengths"_a, "transform"_a)
            .def_property(
                    "lengths", [](const collision::Box& b) { return from_vector3(b.lengths_); },
                    [](collision::Box& b, const farray& v) { b.lengths_ = to_vector3(v); });
    py::class_<collision::Sphere, std::shared_ptr<collision::Sphere>, collision::Primitive>(mcol, "Sphere")
            .def(py::init<float>(), "radius"_a)
            .def(py::init([](float radius, const farray& c) { return std::make_shared<collision::Sphere>(radius, to_vector3(c)); }), "radius"_a, "center"_a)
            .def_readwrite("radius", &collision::Sphere::radius_);
    py::class_<collision::Capsule, std::shared_ptr<collision::Capsule>, collision::Primitive>(mcol, "Capsule")
            .def(py::init<float, float>(), "radius"_a, "height"_a)
            .def(py::init([](float r, float h, const farray& T) { return std::make_shared<collision::Capsule>(r, h, to_matrix4(T)); }), "radius"_a,
                 "height"_a, "transform"_a)
            .def_readwrite("radius", &collision::Capsule::radius_)
            .def_readwrite("height", &collision::Capsule::height_);
    py::class_<collision::Cylinder, std::shared_ptr<collision::Cylinder>, collision::Primitive>(mcol, "Cylinder")
            .def(py::init<float, float>(), "radius"_a, "height"_a)
            .def(py::init([](float r, float h, const farray& T) { return std::make_shared<collision::Cylinder>(r, h, to_matrix4(T)); }), "radius"_a,
                 "height"_a, "transform"_a)
            .def_readwrite("radius", &collision::Cylinder::radius_)
            .def_readwrite("height", &collision::Cylinder::height_);
    struct PrimitiveArrayBox {
        collision::PrimitiveArray data;
    };
    py::class_<PrimitiveArrayBox>(mcol, "PrimitiveArray")
            .def(py::init<>())
            .def("append", [](PrimitiveArrayBox& a, const collision::Primitive& p) { a.data.push_back(collision::PrimitivePack(p)); }, "primitive"_a)
            .def("__len__", [](const PrimitiveArrayBox& a) { return a.data.size(); });
    py::class_<collision::CollisionResult, std::shared_ptr<collision::CollisionResult>> col_res(mcol, "CollitionResult");
    col_res.def(py::init<>())
            .def("is_collided", &collision::CollisionResult::IsCollided)
            .def("__repr__",
                 [](const collision::CollisionResult& r) {
                     return std::string("collision::CollisionResult with ") + std::to_string(r.collision_index_pairs_.size()) + " collisions.";
                 })
            .def("get_collision_index_pairs", [](const collision::CollisionResult& r) { return corres_to_array(r.collision_index_pairs_); })
            .def("get_first_collision_indices", [](const collision::CollisionResult& r) { ULongVector v; v.data = r.GetFirstCollisionIndices(); return v; })
            .def("get_second_collision_indices", [](const collision::CollisionResult& r) { ULongVector v; v.data = r.GetSecondCollisionIndices(); return v; })
            .def_readwrite("first", &collision::CollisionResult::first_)
            .def_readwrite("second", &collision::CollisionResult::second_)
            .def_property(
                    "collision_index_pairs", [](const collision::CollisionResult& r) { Vector2iVector v; v.data = r.collision_index_pairs_; return v; },
                    [](collision::CollisionResult& r, const Vector2iVector& v) { r.collision_index_pairs_ = v.data; });
    mcol.attr("CollisionResult") = mcol.attr("CollitionResult");
    py::enum_<collision::CollisionResult::CollisionType>(col_res, "Type")
            .value("Unspecified", collision::CollisionResult::CollisionType::Unspecified)
            .value("Primitives", collision::CollisionResult::CollisionType::Primitives)
            .value("VoxelGrid", collision::CollisionResult::CollisionType::VoxelGrid)
            .value("OccupancyGrid", collision::CollisionResult::CollisionType::OccupancyGrid)
            .value("LineSet", collision::CollisionResult::CollisionType::LineSet);
#define CUPOCH_AMD_BIND(A, B, NA, NB, GA, GB)                                                                              \
    mcol.def("compute_intersection",                                                                                       \
             [](const A& a, const B& b, float margin) { return collision::ComputeIntersection(GA, GB, margin); }, NA##_a, NB##_a, \
             "margin"_a = 0.0f)
    CUPOCH_AMD_BIND(geometry::VoxelGrid, geometry::VoxelGrid, "voxelgrid1", "voxelgrid2", a, b);
    CUPOCH_AMD_BIND(geometry::VoxelGrid, geometry::LineSet<3>, "voxelgrid", "lineset", a, b);
    CUPOCH_AMD_BIND(geometry::LineSet<3>, geometry::VoxelGrid, "lineset", "voxelgrid", a, b);
    CUPOCH_AMD_BIND(geometry::VoxelGrid, geometry::OccupancyGrid, "voxelgrid", "occgrid", a, b);
    CUPOCH_AMD_BIND(geometry::OccupancyGrid, geometry::VoxelGrid, "occgrid", "voxelgrid", a, b);
    CUPOCH_AMD_BIND(geometry::LineSet<3>, geometry::OccupancyGrid, "lineset", "occgrid", a, b);
    CUPOCH_AMD_BIND(geometry::OccupancyGrid, geometry::LineSet<3>, "occgrid", "lineset", a, b);
    CUPOCH_AMD_BIND(PrimitiveArrayBox, geometry::VoxelGrid, "primitives", "voxelgrid", a.data, b);
    CUPOCH_AMD_BIND(geometry::VoxelGrid, PrimitiveArrayBox, "voxelgrid", "primitives", a, b.data);
    CUPOCH_AMD_BIND(PrimitiveArrayBox, geometry::OccupancyGrid, "primitives", "occgrid", a.data, b);
    CUPOCH_AMD_BIND(geometry::OccupancyGrid, PrimitiveArrayBox, "occgrid", "primitives", a, b.data);
#undef CUPOCH_AMD_BIND
    mcol.def("create_voxel_grid", &collision::CreateVoxelGrid, "primitive"_a, "voxel_size"_a);

    // ---------------------------------------------------------------- integration
    // cupoch_pybind/integration/integration.cpp: TSDFVolumeColorType and UniformTSDFVolume with the reference's names.
    // Not bound, as not built: extract_triangle_mesh, extract_voxel_grid.  ScalableTSDFVolume is bound in the
    // submodule integration_scalable below (this submodule's names are pinned by its surface test).
    py::module mi = m.def_submodule("integration");
    py::enum_<integration::TSDFVolumeColorType>(mi, "TSDFVolumeColorType", py::arithmetic())
            .value("NoColor", integration::TSDFVolumeColorType::NoColor)
            .value("RGB8", integration::TSDFVolumeColorType::RGB8)
            .value("Gray32", integration::TSDFVolumeColorType::Gray32)
            .export_values();
    py::class_<integration::UniformTSDFVolume, std::shared_ptr<integration::UniformTSDFVolume>>(mi, "UniformTSDFVolume")
            .def(py::init([](float length, int resolution, float sdf_trunc, integration::TSDFVolumeColorType color_type) {
                     return std::make_shared<integration::UniformTSDFVolume>(length, resolution, sdf_trunc, color_type);
                 }),
                 "length"_a, "resolution"_a, "sdf_trunc"_a, "color_type"_a)
            .def(py::init([](float length, int resolution, float sdf_trunc, integration::TSDFVolumeColorType color_type,
                             const farray& origin) {
                     return std::make_shared<integration::UniformTSDFVolume>(length, resolution, sdf_trunc, color_type,
                                                                             to_vector3(origin));
                 }),
                 "length"_a, "resolution"_a, "sdf_trunc"_a, "color_type"_a, "origin"_a)
            .def("__repr__",
                 [](const integration::UniformTSDFVolume& v) {
                     return std::string("integration::UniformTSDFVolume ") +
                            (v.color_type_ == integration::TSDFVolumeColorType::NoColor ? "without color." : "with color.");
                 })
            .def("reset", &integration::UniformTSDFVolume::Reset)
            .def("integrate",
                 [](integration::UniformTSDFVolume& v, const geometry::RGBDImage& image,
                    const camera::PinholeCameraIntrinsic& intrinsic,
                    const farray& extrinsic) { v.Integrate(image, intrinsic, to_matrix4(extrinsic)); },
                 "image"_a, "intrinsic"_a, "extrinsic"_a)
            .def("extract_point_cloud", &integration::UniformTSDFVolume::ExtractPointCloud)
            .def("extract_voxel_point_cloud", &integration::UniformTSDFVolume::ExtractVoxelPointCloud)
            .def("raycast",
                 [](const integration::UniformTSDFVolume& v, const camera::PinholeCameraIntrinsic& intrinsic,
                    const farray& extrinsic, float sdf_trunc, bool project_valid_depth_only) {
                     return v.Raycast(intrinsic, to_matrix4(extrinsic), sdf_trunc, project_valid_depth_only);
                 },
                 "intrinsic"_a, "extrinsic"_a, "sdf_trunc"_a, "project_valid_depth_only"_a = true)
            .def_readonly("voxel_length", &integration::UniformTSDFVolume::voxel_length_)
            .def_readonly("sdf_trunc", &integration::UniformTSDFVolume::sdf_trunc_)
            .def_readonly("color_type", &integration::UniformTSDFVolume::color_type_)
            .def_readonly("length", &integration::UniformTSDFVolume::length_)
            .def_readonly("resolution", &integration::UniformTSDFVolume::resolution_)
            .def_property_readonly("origin", [](const integration::UniformTSDFVolume& v) { return from_vector3(v.origin_); });
    // integration.cpp:153-195: the reference's constructor and __repr__; map_size (the C++ constructor's last argument)
    // may be given by name.  The units are read back through the ctypes mirror (cupoch_amd.integration_scalable).
    py::module mis = m.def_submodule("integration_scalable");
    py::class_<integration::ScalableTSDFVolume, std::shared_ptr<integration::ScalableTSDFVolume>>(mis, "ScalableTSDFVolume")
            .def(py::init([](float voxel_length, float sdf_trunc, integration::TSDFVolumeColorType color_type,
                             int depth_sampling_stride, int map_size) {
                     return std::make_shared<integration::ScalableTSDFVolume>(voxel_length, sdf_trunc, color_type,
                                                                              depth_sampling_stride, map_size);
                 }),
                 "voxel_length"_a, "sdf_trunc"_a, "color_type"_a, "depth_sampling_stride"_a = 4, "map_size"_a = 1000)
            .def("__repr__",
                 [](const integration::ScalableTSDFVolume& v) {
                     return std::string("pipelines::integration::ScalableTSDFVolume ") +
                            (v.color_type_ == integration::TSDFVolumeColorType::NoColor ? "without color." : "with color.");
                 })
            .def("reset", &integration::ScalableTSDFVolume::Reset)
            .def("integrate",
                 [](integration::ScalableTSDFVolume& v, const geometry::RGBDImage& image,
                    const camera::PinholeCameraIntrinsic& intrinsic,
                    const farray& extrinsic) { v.Integrate(image, intrinsic, to_matrix4(extrinsic)); },
                 "image"_a, "intrinsic"_a, "extrinsic"_a)
            .def("extract_point_cloud", &integration::ScalableTSDFVolume::ExtractPointCloud)
            .def("extract_voxel_point_cloud", &integration::ScalableTSDFVolume::ExtractVoxelPointCloud)
            .def("num_volume_units", &integration::ScalableTSDFVolume::NumVolumeUnits)
            .def_readonly("voxel_length", &integration::ScalableTSDFVolume::voxel_length_)
            .def_readonly("sdf_trunc", &integration::ScalableTSDFVolume::sdf_trunc_)
            .def_readonly("color_type", &integration::ScalableTSDFVolume::color_type_)
            .def_readonly("volume_unit_length", &integration::ScalableTSDFVolume::volume_unit_length_)
            .def_readonly("resolution", &integration::ScalableTSDFVolume::resolution_)
            .def_readonly("volume_unit_voxel_num", &integration::ScalableTSDFVolume::volume_unit_voxel_num_)
            .def_readonly("depth_sampling_stride", &integration::ScalableTSDFVolume::depth_sampling_stride_);

    // ---------------------------------------------------------------- imageproc (cupoch_pybind/imageproc/imageproc.cpp)
    py::module mip = m.def_submodule("imageproc");
    py::enum_<imageproc::SGMOption::DisparitySizeType>(mip, "DisparitySizeType")
            .value("DisparitySize64", imageproc::SGMOption::DisparitySize64)
            .value("DisparitySize128", imageproc::SGMOption::DisparitySize128)
            .value("DisparitySize256", imageproc::SGMOption::DisparitySize256)
            .export_values();
    py::enum_<imageproc::SGMOption::PathType>(mip, "PathType")
            .value("ScanPath4", imageproc::SGMOption::ScanPath4)
            .value("ScanPath8", imageproc::SGMOption::ScanPath8)
            .export_values();
    py::class_<imageproc::SGMOption>(mip, "SGMOption", "Parameters for Semi-Global Matching.")
            .def(py::init<>())
            .def(py::init<const imageproc::SGMOption&>())
            .def("__copy__", [](const imageproc::SGMOption& o) { return imageproc::SGMOption(o); })
            .def("__deepcopy__", [](const imageproc::SGMOption& o, py::dict&) { return imageproc::SGMOption(o); })
            .def_readwrite("width", &imageproc::SGMOption::width_)
            .def_readwrite("height", &imageproc::SGMOption::height_)
            .def_readwrite("p1", &imageproc::SGMOption::p1_)
            .def_readwrite("p2", &imageproc::SGMOption::p2_)
            .def_readwrite("uniqueness", &imageproc::SGMOption::uniqueness_)
            .def_readwrite("disp_size", &imageproc::SGMOption::disp_size_)
            .def_readwrite("path_type", &imageproc::SGMOption::path_type_)
            .def_readwrite("min_disp", &imageproc::SGMOption::min_disp_)
            .def_readwrite("lr_max_diff", &imageproc::SGMOption::lr_max_diff_);
    py::class_<imageproc::SemiGlobalMatching>(mip, "SemiGlobalMatching", "This class implements Semi-Global Matching algorithm.")
            .def(py::init([](const imageproc::SGMOption& params) { return new imageproc::SemiGlobalMatching(params); }))
            .def("process_frame", &imageproc::SemiGlobalMatching::ProcessFrame);


    // ---------------------------------------------------------------- registration
    py::module mr = m.def_submodule("registration");
    py::class_<registration::ICPConvergenceCriteria>(mr, "ICPConvergenceCriteria")
            .def(py::init<float, float, int>(), "relative_fitness"_a = 1e-6f, "relative_rmse"_a = 1e-6f,
                 "max_iteration"_a = 30)
            .def_readwrite("relative_fitness", &registration::ICPConvergenceCriteria::relative_fitness_)
            .def_readwrite("relative_rmse", &registration::ICPConvergenceCriteria::relative_rmse_)
            .def_readwrite("max_iteration", &registration::ICPConvergenceCriteria::max_iteration_);

    py::enum_<registration::TransformationEstimationType>(mr, "TransformationEstimationType")
            .value("Unspecified", registration::TransformationEstimationType::Unspecified)
            .value("PointToPoint", registration::TransformationEstimationType::PointToPoint)
            .value("PointToPlane", registration::TransformationEstimationType::PointToPlane)
            .value("SymmetricMethod", registration::TransformationEstimationType::SymmetricMethod)
            .value("ColoredICP", registration::TransformationEstimationType::ColoredICP)
            .value("GeneralizedICP", registration::TransformationEstimationType::GeneralizedICP);

    // the estimators, each behind the trampoline (a Python class may derive from any of them)
    auto set_arg = [](const py::object& o) {  // a Vector2iVector or anything (n, 2)-array-like
        if (py::isinstance<Vector2iVector>(o)) return o.cast<const Vector2iVector&>().data;
        return Vector2iVector(o.cast<py::array_t<int, py::array::c_style | py::array::forcecast>>()).data;
    };
    py::class_<registration::TransformationEstimation, PyTransformationEstimation<>>(mr, "TransformationEstimation")
            .def(py::init<>())
            .def("get_transformation_estimation_type",
                 &registration::TransformationEstimation::GetTransformationEstimationType)
            .def("compute_rmse",
                 [set_arg](const registration::TransformationEstimation& e, const geometry::PointCloud& s,
                           const geometry::PointCloud& t, const py::object& corres) { return e.ComputeRMSE(s, t, set_arg(corres)); },
                 "source"_a, "target"_a, "corres"_a)
            .def("compute_transformation",
                 [set_arg](const registration::TransformationEstimation& e, const geometry::PointCloud& s,
                           const geometry::PointCloud& t, const py::object& corres) {
                     return from_matrix4(e.ComputeTransformation(s, t, set_arg(corres)));
                 },
                 "source"_a, "target"_a, "corres"_a);
    py::class_<registration::TransformationEstimationPointToPoint,
               PyTransformationEstimation<registration::TransformationEstimationPointToPoint>, registration::TransformationEstimation>(
            mr, "TransformationEstimationPointToPoint")
            .def(py::init<>());
    py::class_<registration::TransformationEstimationPointToPlane,
               PyTransformationEstimation<registration::TransformationEstimationPointToPlane>, registration::TransformationEstimation>(
            mr, "TransformationEstimationPointToPlane")
            .def(py::init<float>(), "det_thresh"_a = 1e-6f)
            .def_readwrite("det_thresh", &registration::TransformationEstimationPointToPlane::det_thresh_);
    py::class_<registration::TransformationEstimationSymmetricMethod,
               PyTransformationEstimation<registration::TransformationEstimationSymmetricMethod>, registration::TransformationEstimation>(
            mr, "TransformationEstimationSymmetricMethod")
            .def(py::init<float>(), "det_thresh"_a = 1e-6f)
            .def_readwrite("det_thresh", &registration::TransformationEstimationSymmetricMethod::det_thresh_);
    py::class_<registration::TransformationEstimationForGeneralizedICP,
               PyTransformationEstimation<registration::TransformationEstimationForGeneralizedICP>, registration::TransformationEstimation>(
            mr, "TransformationEstimationForGeneralizedICP")
            .def(py::init<float>(), "epsilon"_a = 1e-3f)
            .def_readwrite("epsilon", &registration::TransformationEstimationForGeneralizedICP::epsilon_);

    py::class_<registration::RegistrationResult>(mr, "RegistrationResult")
            .def(py::init<>())
            .def_property(
                    "transformation",
                    [](const registration::RegistrationResult& r) { return from_matrix4(r.transformation_); },
                    [](registration::RegistrationResult& r, const farray& T) { r.transformation_ = to_matrix4(T); })
            .def_property_readonly("correspondence_set",
                                   [](const registration::RegistrationResult& r) { return corres_to_array(r.correspondence_set_); })
            .def_readwrite("inlier_rmse", &registration::RegistrationResult::inlier_rmse_)
            .def_readwrite("fitness", &registration::RegistrationResult::fitness_)
            .def("__repr__", [](const registration::RegistrationResult& r) {
                return "registration::RegistrationResult with fitness = " + std::to_string(r.fitness_) +
                       ", inlier_rmse = " + std::to_string(r.inlier_rmse_) + ", and correspondence_set size of " +
                       std::to_string(r.correspondence_set_.size());
            });

    mr.def(
            "evaluate_registration",
            [](const geometry::PointCloud& s, const geometry::PointCloud& t, float d, const farray& T) {
                return registration::EvaluateRegistration(s, t, d, to_matrix4(T));
            },
            "source"_a, "target"_a, "max_correspondence_distance"_a, "transformation"_a = identity4());
    mr.def(
            "registration_icp",
            [](const geometry::PointCloud& s, const geometry::PointCloud& t, float d, const farray& init,
               const registration::TransformationEstimation& est, const registration::ICPConvergenceCriteria& crit) {
                return registration::RegistrationICP(s, t, d, to_matrix4(init), est, crit);
            },
            "source"_a, "target"_a, "max_correspondence_distance"_a, "init"_a = identity4(),
            "estimation_method"_a = registration::TransformationEstimationPointToPoint(),
            "criteria"_a = registration::ICPConvergenceCriteria());
    mr.def(
            "registration_generalized_icp",
            [](const geometry::PointCloud& s, const geometry::PointCloud& t, float d, const farray& init,
               const registration::TransformationEstimationForGeneralizedICP& est,
               const registration::ICPConvergenceCriteria& crit) {
                return registration::RegistrationGeneralizedICP(s, t, d, to_matrix4(init), est, crit);
            },
            "source"_a, "target"_a, "max_correspondence_distance"_a, "init"_a = identity4(),
            "estimation"_a = registration::TransformationEstimationForGeneralizedICP(),
            "criteria"_a = registration::ICPConvergenceCriteria());
    mr.def(
            "registration_colored_icp",
            [](const geometry::PointCloud& s, const geometry::PointCloud& t, float d, const farray& init,
               const registration::ICPConvergenceCriteria& crit, float lambda_geometric, float det_thresh) {
                return registration::RegistrationColoredICP(s, t, d, to_matrix4(init), crit, lambda_geometric, det_thresh);
            },
            "source"_a, "target"_a, "max_distance"_a, "init"_a = identity4(),
            "criteria"_a = registration::ICPConvergenceCriteria(), "lambda_geometric"_a = 0.968f, "det_thresh"_a = 1e-6f);

    // FeatureFPFH / FeatureSHOT, FastGlobalRegistrationOption, registration_fast_based_on_feature_matching (both
    // overloads) and correspondences_from_features.  Not bound, as not built: compute_fpfh_feature, compute_shot_feature.
    bind_feature<33>(mr, "FeatureFPFH", "Class to store FPFH features for registration.");
    bind_feature<352>(mr, "FeatureSHOT", "Class to store SHOT features for registration.");
    using FgrOption = registration::FastGlobalRegistrationOption;
    py::class_<FgrOption>(mr, "FastGlobalRegistrationOption", "Options for FastGlobalRegistration.")
            .def(py::init<float, bool, bool, float, int, float, int>(), "division_factor"_a = 1.4f, "use_absolute_scale"_a = false,
                 "decrease_mu"_a = true, "maximum_correspondence_distance"_a = 0.025f, "iteration_number"_a = 64,
                 "tuple_scale"_a = 0.95f, "maximum_tuple_count"_a = 1000)
            .def(py::init<const FgrOption&>())
            .def("__copy__", [](const FgrOption& o) { return FgrOption(o); })
            .def("__deepcopy__", [](const FgrOption& o, py::dict&) { return FgrOption(o); })
            .def_readwrite("division_factor", &FgrOption::division_factor_)
            .def_readwrite("use_absolute_scale", &FgrOption::use_absolute_scale_)
            .def_readwrite("decrease_mu", &FgrOption::decrease_mu_)
            .def_readwrite("maximum_correspondence_distance", &FgrOption::maximum_correspondence_distance_)
            .def_readwrite("iteration_number", &FgrOption::iteration_number_)
            .def_readwrite("tuple_scale", &FgrOption::tuple_scale_)
            .def_readwrite("maximum_tuple_count", &FgrOption::maximum_tuple_count_)
            .def("__repr__", [](const FgrOption& o) {
                return "registration::FastGlobalRegistrationOption class with \ndivision_factor=" + std::to_string(o.division_factor_) +
                       "\nuse_absolute_scale=" + std::to_string(o.use_absolute_scale_) + "\ndecrease_mu=" + std::to_string(o.decrease_mu_) +
                       "\nmaximum_correspondence_distance=" + std::to_string(o.maximum_correspondence_distance_) +
                       "\niteration_number=" + std::to_string(o.iteration_number_) + "\ntuple_scale=" + std::to_string(o.tuple_scale_) +
                       "\nmaximum_tuple_count=" + std::to_string(o.maximum_tuple_count_);
            });
    mr.def("registration_fast_based_on_feature_matching", &registration::FastGlobalRegistration<33>, "source"_a, "target"_a,
           "source_feature"_a, "target_feature"_a, "option"_a = FgrOption(), "seed"_a = (uint64_t)0);
    mr.def("registration_fast_based_on_feature_matching", &registration::FastGlobalRegistration<352>, "source"_a, "target"_a,
           "source_feature"_a, "target_feature"_a, "option"_a = FgrOption(), "seed"_a = (uint64_t)0);
    mr.def(
            "correspondences_from_features",
            [](const registration::Feature<33>& s, const registration::Feature<33>& t, bool mutual_filter, float ratio) {
                return corres_to_array(registration::CorrespondencesFromFeatures<33>(s, t, mutual_filter, ratio));
            },
            "source_features"_a, "target_features"_a, "mutual_filter"_a = false, "mutual_consistency_ratio"_a = 0.1f);
    mr.def(
            "correspondences_from_features",
            [](const registration::Feature<352>& s, const registration::Feature<352>& t, bool mutual_filter, float ratio) {
                return corres_to_array(registration::CorrespondencesFromFeatures<352>(s, t, mutual_filter, ratio));
            },
            "source_features"_a, "target_features"_a, "mutual_filter"_a = false, "mutual_consistency_ratio"_a = 0.1f);

    // ---------------------------------------------------------------- kinfu (cupoch_pybind/kinfu/kinfu.cpp)
    // The reference's names.  Not bound, as not built: extract_triangle_mesh; the pipeline has no copy functions
    // (its volume is not copyable here).
    py::module mkf = m.def_submodule("kinfu");
    py::class_<kinfu::KinfuOption>(mkf, "KinfuOption", "Parameters for Kinect Fusion.")
            .def(py::init<>())
            .def(py::init<const kinfu::KinfuOption&>())
            .def("__copy__", [](const kinfu::KinfuOption& o) { return kinfu::KinfuOption(o); })
            .def("__deepcopy__", [](const kinfu::KinfuOption& o, py::dict&) { return kinfu::KinfuOption(o); })
            .def_readwrite("num_pyramid_levels", &kinfu::KinfuOption::num_pyramid_levels_)
            .def_readwrite("diameter", &kinfu::KinfuOption::diameter_)
            .def_readwrite("sigma_depth", &kinfu::KinfuOption::sigma_depth_)
            .def_readwrite("sigma_space", &kinfu::KinfuOption::sigma_space_)
            .def_readwrite("depth_cutoff", &kinfu::KinfuOption::depth_cutoff_)
            .def_readwrite("tsdf_length", &kinfu::KinfuOption::tsdf_length_)
            .def_readwrite("tsdf_resolution", &kinfu::KinfuOption::tsdf_resolution_)
            .def_readwrite("sdf_trunc", &kinfu::KinfuOption::sdf_trunc_)
            .def_readwrite("tsdf_color_type", &kinfu::KinfuOption::tsdf_color_type_)
            .def_property(
                    "tsdf_origin", [](const kinfu::KinfuOption& o) { return from_vector3(o.tsdf_origin_); },
                    [](kinfu::KinfuOption& o, const farray& v) { o.tsdf_origin_ = to_vector3(v); })
            .def_readwrite("distance_threshold", &kinfu::KinfuOption::distance_threshold_)
            .def_readwrite("icp_iterations", &kinfu::KinfuOption::icp_iterations_)
            .def_readwrite("tf_type", &kinfu::KinfuOption::tf_type_);
    py::class_<kinfu::KinfuPipeline>(mkf, "KinfuPipeline", "KinfuPipeline implements Kinect fusion algorithm.")
            .def(py::init([](const camera::PinholeCameraIntrinsic& intrinsic, const kinfu::KinfuOption& params) {
                return new kinfu::KinfuPipeline(intrinsic, params);
            }))
            .def("reset", &kinfu::KinfuPipeline::Reset)
            .def("process_frame", &kinfu::KinfuPipeline::ProcessFrame)
            .def("extract_point_cloud", &kinfu::KinfuPipeline::ExtractPointCloud)
            .def_property(
                    "cur_pose", [](const kinfu::KinfuPipeline& p) { return from_matrix4(p.cur_pose_); },
                    [](kinfu::KinfuPipeline& p, const farray& T) { p.cur_pose_ = to_matrix4(T); })
            .def_readwrite("model_pyramid", &kinfu::KinfuPipeline::model_pyramid_);
}
