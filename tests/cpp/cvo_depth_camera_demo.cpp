// cvo_depth_camera_demo.cpp -- registration::set_depth_camera / clear_depth_camera of
// include/cvo.hpp: the image form of run_cvo() with a depth camera of its own (another size,
// pinhole and lens, mounted beside the colour camera; the depth image is registered to
// colour on the device, cvo_frontend.h).
// Frames 0 and 1 run with the rig (set BEFORE the first image, i.e. before the front end
// exists), frame 2 after clear_depth_camera() with a depth image of the colour size, frame 3
// after set_depth_camera() again (the front end exists: the rig goes to it at once).  A rig
// whose R is a reflection is refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_depth_camera; every depth image behind its size.
// Build: g++ -std=c++17 -I include cvo_depth_camera_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_reflection(cvo_hip::registration &reg, cvo_fe_depth_camera rig, std::ostream &lines)
{
    rig.R[8] = -rig.R[8]; rig.R[2] = -rig.R[2]; rig.R[5] = -rig.R[5];   // (the third column negated)
    try {
        reg.set_depth_camera(rig);
        lines << "accepted a reflection\n";
    } catch (const std::exception &) {
        lines << "refused a reflection\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_depth_camera rig;
        d.read(&rig, 1);
        try_reflection(*d.reg, rig, d.lines);
        d.reg->set_depth_camera(rig);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(/*depth_sizes*/ true);
            if (i == 2) d.reg->clear_depth_camera();
            if (i == 3) {
                try_reflection(*d.reg, rig, d.lines);
                d.reg->set_depth_camera(rig);
            }
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
