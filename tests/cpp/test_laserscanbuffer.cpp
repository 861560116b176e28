// geometry::LaserScanBuffer through the C++ surface, with the reference's signatures: the reference's three unit tests
// (src/tests/geometry/laserscanbuffer.cpp: Constructor, AddRanges with pop and fill-to-full with intensities,
// RangeFilter), then one conversion each way.  argv[1]: a directory holding scans.f32 ([3][steps] ranges), values.f32
// (their intensities), origins.f32 ([3][16], column-major) and cloud.f32 ([n][3] points); the cloud of the scans goes
// there as points.f32 / colors.f32 and the virtual scan of the cloud as bins.f32.  Prints one JSON line;
// tests/test_gpu_laserscan_cpp.py compiles and runs it and holds the output to tests/laserscan_exact.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static std::vector<float> ReadRaw(const std::string& path) {
    std::vector<float> v;
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(float));
    if (!v.empty() && std::fread((void*)v.data(), sizeof(float), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

static bool WriteRaw(const std::string& path, const void* p, size_t bytes) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static int g_failed = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++g_failed;                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
        }                                                                   \
    } while (0)

static bool Constructor() {
    const int before = g_failed;
    geometry::LaserScanBuffer scan(100);
    EXPECT(geometry::Geometry::GeometryType::LaserScanBuffer == scan.GetGeometryType());
    EXPECT(3 == scan.Dimension());
    EXPECT(0u == scan.ranges_.size());
    EXPECT(0u == scan.intensities_.size());
    EXPECT(scan.IsEmpty());
    EXPECT(!scan.HasIntensities());
    EXPECT(scan.num_max_scans_ == 50 && geometry::DEFAULT_NUM_MAX_SCANS == 50u);
    EXPECT(scan.min_angle_ == (float)-M_PI && scan.max_angle_ == (float)M_PI);
    EXPECT(scan.GetAngleIncrement() == ((float)M_PI - (float)-M_PI) / 99.0f);
    return g_failed == before;
}

static bool AddRanges() {
    const int before = g_failed;
    const unsigned int buffer_size = 10;
    geometry::LaserScanBuffer scan(100, buffer_size);
    EXPECT(scan.num_steps_ == 100 && scan.bottom_ == 0);
    utility::pinned_host_vector<float> hvec(100, 1.0f);
    scan.AddRanges(hvec);
    EXPECT(scan.bottom_ == 1 && scan.GetNumScans() == 1);
    EXPECT(scan.GetRanges().size() == (size_t)scan.num_steps_ * (size_t)scan.GetNumScans());
    scan.AddRanges(hvec);
    EXPECT(scan.bottom_ == 2 && scan.GetNumScans() == 2);
    EXPECT(scan.GetRanges().size() == (size_t)scan.num_steps_ * (size_t)scan.GetNumScans());
    auto oldest = scan.PopOneScan();
    EXPECT(oldest && oldest->num_steps_ == 100 && oldest->GetNumScans() == 1);
    EXPECT(scan.GetNumScans() == 1);
    scan.Clear();
    EXPECT(scan.IsEmpty() && scan.ranges_.size() == 0u);
    for (unsigned int i = 0; i < buffer_size; ++i) {
        EXPECT(!scan.IsFull());
        scan.AddRanges(hvec, Eigen::Matrix4f::Identity(), hvec);
        EXPECT(scan.GetRanges().size() == (size_t)scan.num_steps_ * (size_t)scan.GetNumScans());
        EXPECT(scan.GetIntensities().size() == (size_t)scan.num_steps_ * (size_t)scan.GetNumScans());
        EXPECT(scan.GetNumScans() == (int)i + 1);
    }
    EXPECT(scan.IsFull() && scan.HasIntensities());
    std::vector<float> two(100, 2.0f);                       // a full ring: the oldest scan goes
    scan.AddRanges(two.data(), Eigen::Matrix4f::Identity(), two.data());
    EXPECT(scan.IsFull() && scan.top_ == 1 && scan.bottom_ == 11);
    const std::vector<float> live = scan.GetRanges();
    EXPECT(live.size() == 1000u && live[0] == 1.0f && live[899] == 1.0f && live[900] == 2.0f && live[999] == 2.0f);
    scan.AddRanges(std::vector<float>(3, 1.0f));             // refused, logged
    EXPECT(scan.bottom_ == 11);
    auto host = scan.PopHostOneScan();
    EXPECT(host.first->size() == 100u && host.second->size() == 100u && (*host.first)[0] == 1.0f && scan.GetNumScans() == 9);
    geometry::LaserScanBuffer other(100, buffer_size);
    other.AddRanges(utility::device_vector<float>(two), Eigen::Matrix4f::Identity(), utility::device_vector<float>(two));
    scan.Merge(other);
    EXPECT(scan.IsFull() && scan.GetRanges()[999] == 2.0f);
    scan.Merge(other);                                       // refused: full
    EXPECT(scan.GetNumScans() == 10);
    return g_failed == before;
}

static bool RangeFilter() {
    const int before = g_failed;
    geometry::LaserScanBuffer scan(5);
    utility::pinned_host_vector<float> hvec = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f};
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    pose(0, 3) = 2.5f;
    scan.AddRanges(hvec, pose, hvec);
    auto out = scan.RangeFilter(1.5, 3.5);
    auto h = out->GetRanges();
    EXPECT(h.size() == 5u && std::isnan(h[0]) && h[1] == 2.0f && h[2] == 3.0f && std::isnan(h[3]) && std::isnan(h[4]));
    EXPECT(out->HasIntensities() && out->GetIntensities() == std::vector<float>(hvec) && out->origins_[0] == pose);   // kept
    EXPECT(scan.GetRanges() == std::vector<float>(hvec));
    EXPECT(scan.GetMinBound() == Eigen::Vector3f::Zero());   // logs "not supported"
    return g_failed == before;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const bool constructor = Constructor(), add = AddRanges(), filter = RangeFilter();

    const std::vector<float> scans = ReadRaw(dir + "/scans.f32"), values = ReadRaw(dir + "/values.f32");
    const std::vector<float> origins = ReadRaw(dir + "/origins.f32"), cloud = ReadRaw(dir + "/cloud.f32");
    if (scans.empty() || scans.size() % 3 || values.size() != scans.size() || origins.size() != 48 || cloud.empty()) return 3;
    const int steps = (int)(scans.size() / 3);
    geometry::LaserScanBuffer scan(steps, 2, -2.1f, 2.3f);    // two slots: the first scan is overwritten
    for (int k = 0; k < 3; ++k) {
        Eigen::Matrix4f o;
        std::memcpy(o.data(), origins.data() + k * 16, 16 * sizeof(float));
        scan.AddRanges(scans.data() + (size_t)k * steps, o, values.data() + (size_t)k * steps);
    }
    auto pc = geometry::PointCloud::CreateFromLaserScanBuffer(scan, 0.5f, 20.0f);
    const std::vector<Eigen::Vector3f> pts = pc->points_.to_host(), cols = pc->colors_.to_host();
    bool written = WriteRaw(dir + "/points.f32", pts.data(), pts.size() * sizeof(Eigen::Vector3f)) &&
                   WriteRaw(dir + "/colors.f32", cols.data(), cols.size() * sizeof(Eigen::Vector3f));
    auto none = geometry::PointCloud::CreateFromLaserScanBuffer(scan, 2.0f, 2.0f);   // logged, empty

    geometry::PointCloud in;
    in.points_.resize(cloud.size() / 3);
    utility::copy_h2d(in.points_.data(), cloud.data(), cloud.size() * sizeof(float));
    auto virt = geometry::LaserScanBuffer::CreateFromPointCloud(in, 0.02f, 0.0f, 2.0f, 3, 0.2f, 9.0f, -1.5f, 1.5f);
    auto bad = geometry::LaserScanBuffer::CreateFromPointCloud(in, 0.0f, 0.0f, 2.0f);   // logged, null
    std::vector<float> bins;
    if (virt) bins = virt->GetRanges();
    written = written && WriteRaw(dir + "/bins.f32", bins.data(), bins.size() * sizeof(float));
    std::printf("{\"constructor\": %s, \"add_ranges\": %s, \"range_filter\": %s, \"written\": %s, \"points\": %zu, \"colors\": %zu, "
                "\"empty\": %zu, \"bad_is_null\": %s, \"virt_steps\": %d, \"virt_scans\": %d, \"virt_slots\": %d, \"origin_z1\": %.9g}\n",
                constructor ? "true" : "false", add ? "true" : "false", filter ? "true" : "false", written ? "true" : "false",
                pts.size(), cols.size(), none->points_.size(), bad ? "false" : "true", virt ? virt->num_steps_ : -1,
                virt ? virt->GetNumScans() : -1, virt ? virt->num_max_scans_ : -1, virt ? (double)virt->origins_[1](2, 3) : 0.0);
    return g_failed ? 1 : 0;
}
