// cvo_score_demo.cpp -- registration::align(cvo_hip_pose_score_t *, float, cvo_hip_pose_hessian_t *) of include/cvo.hpp:
// one pair through a cvo::cvo, scored at the final pose (ell_init) and printed bit for bit.
// Input: a binary file written by the test: int32 n_frames (2), then per frame int32 n, n*3 float32 positions,
// n*5 float32 features (row-major).
// Output (stdout): "n_iter <k>", the integer fields, then every double of the score as C99 hex ("%a"), and "hess_f":
// the f of the pose Hessian the same call evaluated (at the final length scale).
// Build: g++ -std=c++17 -I include cvo_score_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "cvo.hpp"

struct Frame { std::vector<float> xyz, feat; int n; };

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: demo frames.bin\n"); return 2; }
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
    if (!in) { std::fprintf(stderr, "short read\n"); return 2; }
    try {
        cvo::cvo reg;
        for (const Frame &f : frames) reg.set_pcd(cvo_hip::point_cloud_view{f.n, f.xyz.data(), f.feat.data(), CVO_HIP_FEAT_ROWMAJOR});
        cvo_hip_pose_score_t s;
        cvo_hip_pose_hessian_t h;
        reg.align(&s, 0.0f, &h);
        std::printf("n_iter %d\nnnz %lld\nnnz_fixed %lld\nnnz_moving %lld\nfixed_matched %d\nmoving_matched %d\n",
                    reg.num_iterations(), (long long)s.nnz, (long long)s.nnz_fixed, (long long)s.nnz_moving,
                    s.fixed_matched, s.moving_matched);
        std::printf("inner %a\nself_fixed %a\nself_moving %a\ncos_angle %a\nmean_d2 %a\nell %a\nhess_f %a\n", s.inner,
                    s.self_fixed, s.self_moving, s.cos_angle, s.mean_d2, (double)s.ell, h.f);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
