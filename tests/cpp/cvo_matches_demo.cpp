// cvo_matches_demo.cpp -- registration::pose_matches of include/cvo.hpp: two clouds handed to a cvo::cvo, then which
// points matched at a given pose, printed bit for bit.
// Input: a binary file written by the test: int32 n_frames (2), then per frame int32 n, n*3 float32 positions,
// n*5 float32 features (row-major); then 9 float32 R, 3 float32 T, 1 float32 ell.
// Output (stdout): the integer fields of the summary, "inner" and "ell" as C99 hex ("%a"), and per side and array
// "<side>_<array> <fnv1a64 of its bytes, hex>".
// Build: g++ -std=c++17 -I include cvo_matches_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "cvo.hpp"

struct Frame { std::vector<float> xyz, feat; int n; };

static unsigned long long fnv1a(const void *p, size_t bytes)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t k = 0; k < bytes; ++k) { h ^= b[k]; h *= 0x100000001b3ull; }
    return h;
}

struct Side {
    std::vector<double> support;
    std::vector<int32_t> count, best;
    std::vector<float> best_w;
    explicit Side(int n) : support((size_t)n), count((size_t)n), best((size_t)n), best_w((size_t)n) {}
    cvo_hip_point_matches view() { return cvo_hip_point_matches{support.data(), count.data(), best.data(), best_w.data()}; }
    void print(const char *name) const
    {
        std::printf("%s_support %llx\n%s_count %llx\n%s_best %llx\n%s_best_w %llx\n", name, fnv1a(support.data(), support.size() * 8),
                    name, fnv1a(count.data(), count.size() * 4), name, fnv1a(best.data(), best.size() * 4), name,
                    fnv1a(best_w.data(), best_w.size() * 4));
    }
};

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
    float pose[13];
    in.read(reinterpret_cast<char *>(pose), sizeof(pose));
    if (!in) { std::fprintf(stderr, "short read\n"); return 2; }
    try {
        cvo::cvo reg;
        for (const Frame &f : frames) reg.set_pcd(cvo_hip::point_cloud_view{f.n, f.xyz.data(), f.feat.data(), CVO_HIP_FEAT_ROWMAJOR});
        Side fixed(frames[0].n), moving(frames[1].n);
        const cvo_hip_point_matches vf = fixed.view(), vm = moving.view();
        cvo_hip_pose_matches_t s;
        reg.pose_matches(pose, pose + 9, pose[12], &vf, &vm, &s);
        std::printf("nnz %lld\nn_fixed %d\nn_moving %d\nfixed_matched %d\nmoving_matched %d\nexact %d\n", (long long)s.nnz,
                    s.n_fixed, s.n_moving, s.fixed_matched, s.moving_matched, s.exact);
        std::printf("inner %a\nell %a\n", s.inner, (double)s.ell);
        fixed.print("fixed");
        moving.print("moving");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
