// cvo_depth_gate_demo.cpp -- registration::set_depth_gate / clear_depth_gate / set_mask / clear_mask of
// include/cvo.hpp: the image form of run_cvo() with a gate on the depth values and a caller's mask
// (pixels out of range, on or beside a depth jump, or masked give no point; cvo_frontend.h).
// Frames 0 and 1 run with gate and mask (both set BEFORE the first image, i.e. before the front end
// exists; the mask as an image_view), frame 2 after clear_depth_gate() and clear_mask(), frame 3 after
// both are set again (the front end exists: they go to it at once; the mask as pointer and stride).
// A gate with grow = 4 is refused, before and after the front end exists, and so is the mask without
// a size before the first image.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input: int32 n_frames, width, height; cvo_fe_depth_gate; height*width bytes of mask; per frame 32 bytes
// of name, height*width*3 bytes (B,G,R) and height*width uint16 of depth.
// Build: g++ -std=c++17 -I include cvo_depth_gate_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
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

// digest of `rows` rows of `k` 32-bit words, modulo 2^64, whatever the order of the rows:
// h(row) = sum of word j * (j + 1); digest = sum of h * h
static uint64_t digest(const float *p, size_t rows, size_t k)
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

static void try_bad_gate(cvo_hip::registration &reg, cvo_fe_depth_gate gate, std::ostream &lines)
{
    gate.grow = 4;
    try {
        reg.set_depth_gate(gate);
        lines << "accepted a bad gate\n";
    } catch (const std::exception &) {
        lines << "refused a bad gate\n";
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: demo frames.bin cvo|acvo\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    int32_t hdr[3] = {0, 0, 0};
    in.read(reinterpret_cast<char *>(hdr), 12);
    cvo_fe_depth_gate gate;
    in.read(reinterpret_cast<char *>(&gate), sizeof(gate));
    const int nf = hdr[0], w = hdr[1], h = hdr[2];
    if (!in || nf < 1 || w < 1 || h < 1 || w > 8192 || h > 8192) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<uint8_t> mask((size_t)w * h);
    in.read(reinterpret_cast<char *>(mask.data()), (std::streamsize)mask.size());
    const bool adaptive = std::string(argv[2]) == "acvo";
    std::ostringstream lines, quiet;
    std::streambuf *old = std::cout.rdbuf(quiet.rdbuf());   // run_cvo prints like the reference does
    try {
        std::unique_ptr<cvo_hip::registration> reg;
        if (adaptive) reg.reset(new acvo::acvo());
        else reg.reset(new cvo::cvo());
        try_bad_gate(*reg, gate, lines);
        reg->set_depth_gate(gate);
        try {
            reg->set_mask(mask.data(), (size_t)w);
            lines << "accepted a mask without a size\n";
        } catch (const std::exception &) {
            lines << "refused a mask without a size\n";
        }
        reg->set_mask(cvo_hip::image_view{mask.data(), h, w, (size_t)w});
        std::vector<uint8_t> rgb((size_t)w * h * 3);
        std::vector<uint16_t> dep((size_t)w * h);
        std::vector<float> pos4, feat8;
        for (int i = 0; i < nf; ++i) {
            char name[33] = {0};
            in.read(name, 32);
            in.read(reinterpret_cast<char *>(rgb.data()), (std::streamsize)rgb.size());
            in.read(reinterpret_cast<char *>(dep.data()), (std::streamsize)dep.size() * 2);
            if (!in) { std::fprintf(stderr, "short read\n"); return 2; }
            if (i == 2) {
                reg->clear_depth_gate();
                reg->clear_mask();
            }
            if (i == 3) {
                try_bad_gate(*reg, gate, lines);
                reg->set_depth_gate(gate);
                reg->set_mask(mask.data(), (size_t)w);
            }
            const cvo_hip::image_view RGB_img{rgb.data(), h, w, (size_t)w * 3};
            const cvo_hip::image_view dep_img{dep.data(), h, w, (size_t)w * 2};
            reg->run_cvo(/*dataset_seq*/ 1, RGB_img, dep_img);
            // the frame's cloud is the fixed one now (first frame: handed over as fixed; later: swapped after align)
            int rows = 0, points = 0;
            if (cvo_hip_get_device_cloud(reg->context(), 0, nullptr, nullptr, nullptr, &rows, &points) != CVO_HIP_OK)
                throw std::runtime_error("cvo_hip_get_device_cloud");
            pos4.assign((size_t)rows * 4, 0.0f);
            feat8.assign((size_t)rows * 8, 0.0f);
            if (cvo_hip_get_device_cloud(reg->context(), 0, pos4.data(), feat8.data(), nullptr, &rows, &points) != CVO_HIP_OK)
                throw std::runtime_error("cvo_hip_get_device_cloud");
            lines << "cloud " << name << " " << points << " " << digest(pos4.data(), (size_t)points, 4) << " "
                  << digest(feat8.data(), (size_t)points, 8) << "\n";
            float q[4];
            reg->accum_transform.quaternion(q);
            lines << name << " " << reg->accum_transform.matrix()(0, 3) << " " << reg->accum_transform.matrix()(1, 3) << " "
                  << reg->accum_transform.matrix()(2, 3) << " " << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << "\n";
        }
        std::cout.rdbuf(old);
        std::cout << lines.str();
        std::cout << "points_last_frame " << reg->num_points_last_frame() << " iterations " << reg->num_iterations() << "\n";
    } catch (const std::exception &e) {
        std::cout.rdbuf(old);
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
