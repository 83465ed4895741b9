// cvo_camera_demo.cpp -- registration::set_camera / clear_camera of include/cvo.hpp: the
// image form of run_cvo() with a camera model of the caller's (lens distortion removed on
// the device, cvo_frontend.h) in place of the table row of dataset_seq.
// Frames 0 and 1 run with the model (set BEFORE the first image, i.e. before the front end
// exists), frame 2 after clear_camera() with dataset_seq 1, frame 3 after set_camera() again
// (the front end exists: the model goes to it at once).  A model with fx = 0 is refused.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header 10 floats (cvo_fe_camera_model).
// Build: g++ -std=c++17 -I include cvo_camera_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_camera_model model;
        d.read(&model, 1);
        cvo_fe_camera_model bad = model;
        bad.fx = 0.0f;
        try {
            d.reg->set_camera(bad);
            d.lines << "accepted fx = 0\n";
        } catch (const std::exception &) {
            d.lines << "refused fx = 0\n";
        }
        d.reg->set_camera(model);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            if (i == 2) d.reg->clear_camera();
            if (i == 3) d.reg->set_camera(model);
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
