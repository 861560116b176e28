// registration::Feature, knn::BruteForceNN, CorrespondencesFromFeatures and FastGlobalRegistration through the C++
// surface.  argv[1]: a folder with src<Dim>.f32 / tgt<Dim>.f32 ([n][3]) and sfeat<Dim>.f32 / tfeat<Dim>.f32 ([n][Dim]) for Dim =
// 33 and 352, written by tests/test_gpu_fgr_cpp.py, which also compares what this program writes back (T<Dim>.bin,
// corr<Dim>.bin, nn33.bin, cff33.bin, cffm33.bin) with the restatement and the other surfaces.  Prints one JSON line.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cupoch/cupoch.h"

using namespace cupoch;

static int failed = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++failed;                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
        }                                                                 \
    } while (0)

template <class T>
static std::vector<T> ReadAll(const std::string& path) {
    std::vector<T> out;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        out.resize((size_t)bytes / sizeof(T));
        if (std::fread((void*)out.data(), sizeof(T), out.size(), f) != out.size()) out.clear();
        std::fclose(f);
    }
    return out;
}

static void WriteAll(const std::string& path, const void* p, size_t bytes) {
    if (FILE* f = std::fopen(path.c_str(), "wb")) {
        std::fwrite(p, 1, bytes, f);
        std::fclose(f);
    }
}

template <int Dim>
static void Run(const std::string& dir) {
    const std::string d = std::to_string(Dim);
    geometry::PointCloud src, tgt;
    src.points_ = ReadAll<Eigen::Vector3f>(dir + "/src" + d + ".f32");
    tgt.points_ = ReadAll<Eigen::Vector3f>(dir + "/tgt" + d + ".f32");
    EXPECT(src.points_.size() == 360 && tgt.points_.size() == 380);
    registration::Feature<Dim> fs, ft;
    fs.SetData(ReadAll<Eigen::Matrix<float, Dim, 1>>(dir + "/sfeat" + d + ".f32"));
    ft.SetData(ReadAll<Eigen::Matrix<float, Dim, 1>>(dir + "/tfeat" + d + ".f32"));
    EXPECT(fs.Num() == src.points_.size() && ft.Num() == tgt.points_.size() && fs.Dimension() == (size_t)Dim && !fs.IsEmpty());
    EXPECT(fs.GetData().size() == fs.Num());
    const auto a = registration::FastGlobalRegistration<Dim>(src, tgt, fs, ft);
    const auto b = registration::FastGlobalRegistration<Dim>(src, tgt, fs, ft, registration::FastGlobalRegistrationOption(), 0);
    EXPECT(a.transformation_ == b.transformation_ && a.fitness_ == b.fitness_);
    const auto ev = registration::EvaluateRegistration(src, tgt, 0.025f, a.transformation_);
    EXPECT(ev.fitness_ == a.fitness_ && ev.inlier_rmse_ == a.inlier_rmse_ && ev.GetCorrespondenceSet() == a.GetCorrespondenceSet());
    EXPECT(a.fitness_ > 0.8f && a.correspondence_set_.size() >= 300);
    const auto other = registration::FastGlobalRegistration<Dim>(src, tgt, fs, ft, registration::FastGlobalRegistrationOption(), 9);
    EXPECT(other.fitness_ == a.fitness_);  // (another draw, the same answer to within rounding)
    WriteAll(dir + "/T" + d + ".bin", a.transformation_.data(), sizeof(float) * 16);
    const auto cor = a.GetCorrespondenceSet();
    WriteAll(dir + "/corr" + d + ".bin", cor.data(), cor.size() * sizeof(Eigen::Vector2i));
    // empty inputs: a default result and an error log
    const auto none = registration::FastGlobalRegistration<Dim>(src, tgt, registration::Feature<Dim>(), ft);
    EXPECT(none.transformation_ == Eigen::Matrix4f::Identity() && none.fitness_ == 0.0f && none.correspondence_set_.empty());
    const auto none2 = registration::FastGlobalRegistration<Dim>(geometry::PointCloud(), tgt, fs, ft);
    EXPECT(none2.fitness_ == 0.0f && none2.correspondence_set_.empty());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const registration::FastGlobalRegistrationOption o;
    EXPECT(o.division_factor_ == 1.4f && !o.use_absolute_scale_ && o.decrease_mu_ && o.maximum_correspondence_distance_ == 0.025f &&
           o.iteration_number_ == 64 && o.tuple_scale_ == 0.95f && o.maximum_tuple_count_ == 1000);
    registration::Feature<33> f;
    EXPECT(f.IsEmpty() && f.Num() == 0 && f.Dimension() == 33);
    f.Resize(7);
    EXPECT(f.Num() == 7 && f.GetData().size() == 7 && registration::Feature<352>().Dimension() == 352);

    Run<33>(dir);
    Run<352>(dir);

    registration::Feature<33> fs, ft;
    fs.SetData(ReadAll<Eigen::Matrix<float, 33, 1>>(dir + "/sfeat33.f32"));
    ft.SetData(ReadAll<Eigen::Matrix<float, 33, 1>>(dir + "/tfeat33.f32"));
    utility::device_vector<int> idx;
    utility::device_vector<float> dist;
    knn::BruteForceNN<33>(ft.data_, fs.data_, idx, dist);
    EXPECT(idx.size() == 360 && dist.size() == 360);
    const std::vector<int> nn = idx.to_host();
    WriteAll(dir + "/nn33.bin", nn.data(), nn.size() * sizeof(int));
    const auto rows = registration::CorrespondencesFromFeatures(fs, ft).to_host();
    const auto mutual = registration::CorrespondencesFromFeatures(fs, ft, true).to_host();
    const auto fallback = registration::CorrespondencesFromFeatures(fs, ft, true, 0.9f).to_host();
    EXPECT(rows.size() == 360 && mutual.size() < rows.size() && fallback == rows);
    for (size_t i = 0; i < rows.size(); ++i) EXPECT(rows[i](0) == (int)i && rows[i](1) == nn[i]);
    EXPECT(registration::CorrespondencesFromFeatures(registration::Feature<33>(), ft).empty());
    WriteAll(dir + "/cff33.bin", rows.data(), rows.size() * sizeof(Eigen::Vector2i));
    WriteAll(dir + "/cffm33.bin", mutual.data(), mutual.size() * sizeof(Eigen::Vector2i));
    std::printf("{\"failed\": %d}\n", failed);
    return failed ? 1 : 0;
}
