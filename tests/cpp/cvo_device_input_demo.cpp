// cvo_device_input_demo.cpp -- registration::run_cvo_on_device and set_depth_format of include/cvo.hpp: the image form of
// run_cvo() for images that lie in device memory already (the device-input contract of cvo_frontend.h), and depth as
// float32 metres (the depth-format contract).
// Every frame is copied into pitched device images of the demo's own (hipMalloc, rows 48 bytes further apart than their
// bytes; hipMemcpy2D returns when the copy is done, so the images are complete before the call) and goes through
// run_cvo_on_device: nothing of a frame is handed over in host memory.  Frames 0 and 1 carry uint16 depth; from frame 2
// on the depth format is CVO_FE_DEPTH_F32 with unit 1 and the demo hands over (float)d / 5000.0f, metres of a TUM
// depth image.  Depth format 3 is refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the registration
// holds for that frame and, once initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): nothing behind the header.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I include -I <rocm>/include cvo_device_input_demo.cpp
//        -L cvo-rgbd_amd/csrc -lcvo_hip -L <rocm>/lib -lamdhip64
#include <hip/hip_runtime_api.h>

#include "fe_demo_common.hpp"

namespace {

constexpr size_t PAD = 48;   // bytes between the end of a row and the next row

// a pitched image in device memory
struct DeviceImage {
    void *p = nullptr;
    size_t pitch = 0;
    DeviceImage(size_t row, int rows) : pitch(row + PAD)
    {
        if (hipMalloc(&p, pitch * (size_t)rows) != hipSuccess) throw std::runtime_error("hipMalloc");
    }
    ~DeviceImage() { (void)hipFree(p); }
    DeviceImage(const DeviceImage &) = delete;
    DeviceImage &operator=(const DeviceImage &) = delete;
    void fill(const void *src, size_t row, int rows)
    {
        if (hipMemcpy2D(p, pitch, src, row, row, (size_t)rows, hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("hipMemcpy2D");
    }
};

void try_bad_format(cvo_hip::registration &reg, std::ostream &lines)
{
    try {
        reg.set_depth_format(3);
        lines << "accepted a bad depth format\n";
    } catch (const std::exception &) {
        lines << "refused a bad depth format\n";
    }
}

}   // namespace

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        try_bad_format(*d.reg, d.lines);
        const size_t np = (size_t)d.w * d.h;
        DeviceImage img((size_t)d.w * 3, d.h), dep16((size_t)d.w * 2, d.h), dep32((size_t)d.w * 4, d.h);
        std::vector<float> metres(np);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) {
                try_bad_format(*d.reg, d.lines);
                d.reg->set_depth_format(CVO_FE_DEPTH_F32, 1.0f);
            }
            img.fill(d.rgb.data(), (size_t)d.w * 3, d.h);
            const cvo_hip::image_view colour{img.p, d.h, d.w, img.pitch};
            if (i < 2) {
                dep16.fill(d.dep.data(), (size_t)d.w * 2, d.h);
                d.reg->run_cvo_on_device(/*dataset_seq*/ 1, colour, cvo_hip::image_view{dep16.p, d.h, d.w, dep16.pitch});
            } else {
                for (size_t q = 0; q < np; ++q) metres[q] = (float)d.dep[q] / 5000.0f;
                dep32.fill(metres.data(), (size_t)d.w * 4, d.h);
                d.reg->run_cvo_on_device(/*dataset_seq*/ 1, colour, cvo_hip::image_view{dep32.p, d.h, d.w, dep32.pitch});
            }
            d.cloud_line();
            d.pose_line();
        }
    });
}
