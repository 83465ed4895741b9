// cvo_pixel_format_demo.cpp -- registration::set_pixel_format of include/cvo.hpp: the image form of run_cvo() with the
// colour image handed over in the sensor's own pixel format and unpacked on the device (the unpack contract of
// cvo_frontend.h).
// Frames 0 and 1 run under the format (set BEFORE the first image, i.e. before the front end exists), frame 2 after
// set_pixel_format(CVO_FE_PIXEL_BGR8), frame 3 after the format is set again (the front end exists: it goes to it at
// once).  Format 12 is refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the format as int32; the colour image of frames 0, 1 and 3 is the
// packed one, rows * row_bytes bytes of cvo_fe_pixel_layout, that of frame 2 height*width*3 bytes.
// Build: g++ -std=c++17 -I include cvo_pixel_format_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_format(cvo_hip::registration &reg, std::ostream &lines)
{
    try {
        reg.set_pixel_format(12);
        lines << "accepted a bad format\n";
    } catch (const std::exception &) {
        lines << "refused a bad format\n";
    }
}

// next_frame() of fe_demo_common.hpp for a colour image of `rows` rows of `row` bytes
static void next_packed_frame(fe_demo::Demo &d, size_t row, int rows)
{
    std::memset(d.name, 0, sizeof(d.name));
    d.read(d.name, 32);
    d.rgb.resize(row * (size_t)rows);
    d.read(d.rgb.data(), d.rgb.size());
    d.dw = d.w; d.dh = d.h;
    d.dep.resize((size_t)d.w * d.h);
    d.read(d.dep.data(), d.dep.size());
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        int32_t format = 0;
        d.read(&format, 1);
        size_t row = 0;
        int rows = 0;
        if (cvo_fe_pixel_layout(format, d.w, d.h, &row, &rows) != CVO_HIP_OK) throw std::runtime_error("bad format");
        try_bad_format(*d.reg, d.lines);
        d.reg->set_pixel_format(format);
        for (int i = 0; i < d.nf; ++i) {
            if (i == 2) d.reg->set_pixel_format(CVO_FE_PIXEL_BGR8);
            if (i == 3) {
                try_bad_format(*d.reg, d.lines);
                d.reg->set_pixel_format(format);
            }
            if (i == 2) next_packed_frame(d, (size_t)d.w * 3, d.h);
            else next_packed_frame(d, row, rows);
            // (rows and cols are the picture's; the step is the pitch of the packed rows)
            const cvo_hip::image_view img{d.rgb.data(), d.h, d.w, i == 2 ? (size_t)d.w * 3 : row};
            d.reg->run_cvo(/*dataset_seq*/ 1, img, d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
