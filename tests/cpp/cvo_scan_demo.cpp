// cvo_scan_demo.cpp -- registration::pose_scan of include/cvo.hpp: the two clouds of one pair through a cvo::cvo and a
// list of candidate poses scored in one call, printed bit for bit.
// Input: a binary file written by the test: int32 n_frames (2), then per frame int32 n, n*3 float32 positions,
// n*5 float32 features (row-major); then int32 count, count*9 float32 rotations, count*3 float32 translations and one
// float32 length scale.
// Output (stdout): "count <n>", "best <k>", the summary's integers, its doubles as C99 hex ("%a"), then one line per pose:
// "pose <k> <nnz> <inner> <cos_angle> <mean_d2>", the doubles as hex.
// Build: g++ -std=c++17 -I include cvo_scan_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "cvo.hpp"

struct Frame { std::vector<float> xyz, feat; int n; };

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: demo scan.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    int32_t nf = 0;
    in.read(reinterpret_cast<char *>(&nf), 4);
    if (nf != 2) { std::fprintf(stderr, "two frames expected\n"); return 2; }
    std::vector<Frame> frames((size_t)nf);
    for (auto &f : frames) {
        int32_t n = 0;
        in.read(reinterpret_cast<char *>(&n), 4);
        f.n = n;
        f.xyz.resize((size_t)n * 3);
        f.feat.resize((size_t)n * 5);
        in.read(reinterpret_cast<char *>(f.xyz.data()), (std::streamsize)f.xyz.size() * 4);
        in.read(reinterpret_cast<char *>(f.feat.data()), (std::streamsize)f.feat.size() * 4);
    }
    int32_t count = 0;
    in.read(reinterpret_cast<char *>(&count), 4);
    if (!in || count < 0 || count > (1 << 20)) { std::fprintf(stderr, "bad pose count\n"); return 2; }
    std::vector<float> R9((size_t)count * 9), T3((size_t)count * 3);
    float ell = 0.0f;
    in.read(reinterpret_cast<char *>(R9.data()), (std::streamsize)R9.size() * 4);
    in.read(reinterpret_cast<char *>(T3.data()), (std::streamsize)T3.size() * 4);
    in.read(reinterpret_cast<char *>(&ell), 4);
    if (!in) { std::fprintf(stderr, "short read\n"); return 2; }
    try {
        cvo::cvo reg;
        for (const Frame &f : frames) reg.set_pcd(cvo_hip::point_cloud_view{f.n, f.xyz.data(), f.feat.data(), CVO_HIP_FEAT_ROWMAJOR});
        std::vector<cvo_hip_pose_scan_entry> out((size_t)count + 1);
        cvo_hip_pose_scan_t s;
        reg.pose_scan(R9.data(), T3.data(), count, ell, out.data(), &s);
        std::printf("count %d\nbest %d\nnnz_fixed %lld\nnnz_moving %lld\nn_fixed %d\nn_moving %d\n", s.count, s.best,
                    (long long)s.nnz_fixed, (long long)s.nnz_moving, s.n_fixed, s.n_moving);
        std::printf("self_fixed %a\nself_moving %a\nell %a\n", s.self_fixed, s.self_moving, (double)s.ell);
        for (int k = 0; k < count; ++k)
            std::printf("pose %d %lld %a %a %a\n", k, (long long)out[(size_t)k].nnz, out[(size_t)k].inner, out[(size_t)k].cos_angle,
                        out[(size_t)k].mean_d2);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
