// fe_demo_common.hpp -- what the demos of the image form of run_cvo() share (cvo_image_demo.cpp,
// cvo_camera_demo.cpp, cvo_depth_camera_demo.cpp, cvo_depth_gate_demo.cpp): the input file, the registration
// object of the mode asked for, the lines a frame prints, and the frame of main().
// Input: int32 n_frames, width, height; whatever settings the demo reads behind them; per frame 32 bytes of
// name (zero padded), height*width*3 bytes (B,G,R as cv::imread decodes) and the depth image as uint16 --
// height*width of them, or behind its own int32 width and height (next_frame(true)).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo.hpp"

namespace fe_demo {

// digest of `rows` rows of `k` 32-bit words, modulo 2^64, whatever the order of the rows:
// h(row) = sum of word j * (j + 1); digest = sum of h * h
inline uint64_t digest(const float *p, size_t rows, size_t k)
{
    uint64_t acc = 0;
    for (size_t i = 0; i < rows; ++i) {
        uint64_t h = 0;
        for (size_t j = 0; j < k; ++j) {
            uint32_t u;
            std::memcpy(&u, p + i * k + j, 4);
            h += (uint64_t)u * (uint64_t)(j + 1);
        }
        acc += h * h;
    }
    return acc;
}

struct Demo {
    std::ifstream in;
    int nf = 0, w = 0, h = 0;
    std::unique_ptr<cvo_hip::registration> reg;
    std::ostringstream lines;   // what the demo prints once every frame is through
    // the frame read last
    char name[33] = {0};
    std::vector<uint8_t> rgb;
    std::vector<uint16_t> dep;
    int dw = 0, dh = 0;

    template <class T> void read(T *to, size_t count)
    {
        in.read(reinterpret_cast<char *>(to), (std::streamsize)(count * sizeof(T)));
        if (!in) throw std::runtime_error("short read");
    }

    void next_frame(bool depth_sizes = false)
    {
        std::memset(name, 0, sizeof(name));
        read(name, 32);
        rgb.resize((size_t)w * h * 3);
        read(rgb.data(), rgb.size());
        int32_t dsz[2] = {w, h};
        if (depth_sizes) read(dsz, 2);
        if (dsz[0] < 1 || dsz[1] < 1 || dsz[0] > 8192 || dsz[1] > 8192) throw std::runtime_error("bad depth size");
        dw = dsz[0]; dh = dsz[1];
        dep.resize((size_t)dw * dh);
        read(dep.data(), dep.size());
    }

    cvo_hip::image_view rgb_view() const { return cvo_hip::image_view{rgb.data(), h, w, (size_t)w * 3}; }
    cvo_hip::image_view dep_view() const { return cvo_hip::image_view{dep.data(), dh, dw, (size_t)dw * 2}; }

    // "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the registration holds for the
    // frame: the fixed one (first frame: handed over as fixed; later: swapped after align), its live rows
    void cloud_line()
    {
        int rows = 0, points = 0;
        if (cvo_hip_get_device_cloud(reg->context(), 0, nullptr, nullptr, nullptr, &rows, &points) != CVO_HIP_OK)
            throw std::runtime_error("cvo_hip_get_device_cloud");
        std::vector<float> pos4((size_t)rows * 4, 0.0f), feat8((size_t)rows * 8, 0.0f);
        if (cvo_hip_get_device_cloud(reg->context(), 0, pos4.data(), feat8.data(), nullptr, &rows, &points) != CVO_HIP_OK)
            throw std::runtime_error("cvo_hip_get_device_cloud");
        lines << "cloud " << name << " " << points << " " << digest(pos4.data(), (size_t)points, 4) << " "
              << digest(feat8.data(), (size_t)points, 8) << "\n";
    }

    // the pose line of the reference's drivers (ref src/cvo_main.cpp:58-65), default ostream precision
    void pose_line()
    {
        float q[4];
        reg->accum_transform.quaternion(q);
        lines << name << " " << reg->accum_transform.matrix()(0, 3) << " " << reg->accum_transform.matrix()(1, 3) << " "
              << reg->accum_transform.matrix()(2, 3) << " " << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << "\n";
    }
};

// main() of a demo: `demo frames.bin cvo|acvo ...`; body(demo) reads its settings and runs the frames, then
// the lines go out, and "points_last_frame <n> iterations <k>" behind them
template <class Body> int run(int argc, char **argv, int nargs, const char *usage, Body body)
{
    if (argc < nargs) { std::fprintf(stderr, "usage: %s\n", usage); return 2; }
    Demo d;
    d.in.open(argv[1], std::ios::binary);
    int32_t hdr[3] = {0, 0, 0};
    d.in.read(reinterpret_cast<char *>(hdr), 12);
    d.nf = hdr[0]; d.w = hdr[1]; d.h = hdr[2];
    if (!d.in || d.nf < 1 || d.w < 1 || d.h < 1 || d.w > 8192 || d.h > 8192) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::ostringstream quiet;
    std::streambuf *old = std::cout.rdbuf(quiet.rdbuf());   // run_cvo prints like the reference does
    try {
        if (std::string(argv[2]) == "acvo") d.reg.reset(new acvo::acvo());
        else d.reg.reset(new cvo::cvo());
        body(d);
        std::cout.rdbuf(old);
        std::cout << d.lines.str();
        std::cout << "points_last_frame " << d.reg->num_points_last_frame() << " iterations " << d.reg->num_iterations() << "\n";
    } catch (const std::exception &e) {
        std::cout.rdbuf(old);
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

}   // namespace fe_demo
