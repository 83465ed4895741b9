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
// Input (fe_demo_common.hpp): behind the header the cvo_fe_depth_gate and height*width bytes of mask.
// Build: g++ -std=c++17 -I include cvo_depth_gate_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

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
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_depth_gate gate;
        d.read(&gate, 1);
        std::vector<uint8_t> mask((size_t)d.w * d.h);
        d.read(mask.data(), mask.size());
        try_bad_gate(*d.reg, gate, d.lines);
        d.reg->set_depth_gate(gate);
        try {
            d.reg->set_mask(mask.data(), (size_t)d.w);
            d.lines << "accepted a mask without a size\n";
        } catch (const std::exception &) {
            d.lines << "refused a mask without a size\n";
        }
        d.reg->set_mask(cvo_hip::image_view{mask.data(), d.h, d.w, (size_t)d.w});
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) {
                d.reg->clear_depth_gate();
                d.reg->clear_mask();
            }
            if (i == 3) {
                try_bad_gate(*d.reg, gate, d.lines);
                d.reg->set_depth_gate(gate);
                d.reg->set_mask(mask.data(), (size_t)d.w);
            }
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
