// cvo_select_mode_demo.cpp -- registration::set_select_mode of include/cvo.hpp: the image form of run_cvo() with
// the selector among the pixels that have a depth (the selection contract: cvo_frontend.h).
// Frames 0 and 1 run with CVO_FE_SELECT_DEPTH (set BEFORE the first image, i.e. before the front end exists),
// frame 2 after set_select_mode(CVO_FE_SELECT_IMAGE), frame 3 after CVO_FE_SELECT_DEPTH is set again (the front
// end exists: the mode goes to it at once).  A mode of 2 is refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the
// registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once initialised, the pose line
// of the reference's drivers.
// Input (fe_demo_common.hpp): nothing behind the header.
// Build: g++ -std=c++17 -I include cvo_select_mode_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_mode(cvo_hip::registration &reg, std::ostream &lines)
{
    try {
        reg.set_select_mode(2);
        lines << "accepted a bad mode\n";
    } catch (const std::exception &) {
        lines << "refused a bad mode\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        try_bad_mode(*d.reg, d.lines);
        d.reg->set_select_mode(CVO_FE_SELECT_DEPTH);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) d.reg->set_select_mode(CVO_FE_SELECT_IMAGE);
            if (i == 3) {
                try_bad_mode(*d.reg, d.lines);
                d.reg->set_select_mode(CVO_FE_SELECT_DEPTH);
            }
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
