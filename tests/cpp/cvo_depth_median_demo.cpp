// cvo_depth_median_demo.cpp -- registration::set_depth_median / clear_depth_median of include/cvo.hpp: the image form
// of run_cvo() with the median stage on the depth plane (a pixel with a depth takes the lower median of its window,
// a small hole is filled; the median contract of cvo_frontend.h).
// Frames 0 and 1 run with the filter (set BEFORE the first image, i.e. before the front end exists), frame 2 after
// clear_depth_median(), frame 3 after it is set again (the front end exists: it goes to it at once).
// Settings with radius 3 are refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_depth_median.
// Build: g++ -std=c++17 -I include cvo_depth_median_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_median(cvo_hip::registration &reg, cvo_fe_depth_median median, std::ostream &lines)
{
    median.radius = 3;
    try {
        reg.set_depth_median(median);
        lines << "accepted bad settings\n";
    } catch (const std::exception &) {
        lines << "refused bad settings\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_depth_median median;
        d.read(&median, 1);
        try_bad_median(*d.reg, median, d.lines);
        d.reg->set_depth_median(median);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) d.reg->clear_depth_median();
            if (i == 3) {
                try_bad_median(*d.reg, median, d.lines);
                d.reg->set_depth_median(median);
            }
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
