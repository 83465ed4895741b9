// cvo_depth_infill_demo.cpp -- registration::set_depth_infill / clear_depth_infill of include/cvo.hpp: the image form
// of run_cvo() with the infill stage on the depth plane (a short run of pixels without depth between two depths of
// one surface is bridged linearly in inverse depth; the infill contract of cvo_frontend.h).
// Frames 0 and 1 run with the stage (set BEFORE the first image, i.e. before the front end exists), frame 2 after
// clear_depth_infill(), frame 3 after it is set again (the front end exists: it goes to it at once).
// Settings with gap_x 16 are refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_depth_infill.
// Build: g++ -std=c++17 -I include cvo_depth_infill_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_infill(cvo_hip::registration &reg, cvo_fe_depth_infill infill, std::ostream &lines)
{
    infill.gap_x = 16;
    try {
        reg.set_depth_infill(infill);
        lines << "accepted bad settings\n";
    } catch (const std::exception &) {
        lines << "refused bad settings\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_depth_infill infill;
        d.read(&infill, 1);
        try_bad_infill(*d.reg, infill, d.lines);
        d.reg->set_depth_infill(infill);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) d.reg->clear_depth_infill();
            if (i == 3) {
                try_bad_infill(*d.reg, infill, d.lines);
                d.reg->set_depth_infill(infill);
            }
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
