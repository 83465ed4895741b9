// cvo_stereo_rig_demo.cpp -- registration::set_stereo_rig / clear_stereo_rig of include/cvo.hpp: run_cvo_stereo()
// on RAW stereo pairs, both images rectified on the device by the rig in front of the matcher (the rig contract of
// cvo_frontend.h).
// Frames 0 and 1 run with the settings and the rig read from the file, both set BEFORE the first image, i.e. before
// the front end exists; in front of frame 2 the rig is cleared and set again (the front end exists: both go to it at
// once).  Refused, and said so: a rig before any stereo settings, a rig whose baseline is 0 (before and after the
// front end exists), and, under a rig, a camera model and clear_stereo().
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the
// registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once initialised, the pose line of
// the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_stereo and the cvo_fe_stereo_rig; a frame's second image
// is the right colour image, height rows of width*3 bytes, stored as a "depth image" of width*3/2 x height uint16
// behind its own size (the width is even).
// Build: g++ -std=c++17 -I include cvo_stereo_rig_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

template <class Call> static void expect_refusal(std::ostream &lines, const char *what, Call call)
{
    try {
        call();
        lines << "accepted " << what << "\n";
    } catch (const std::exception &) {
        lines << "refused " << what << "\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_stereo st;
        cvo_fe_stereo_rig rig;
        d.read(&st, 1);
        d.read(&rig, 1);
        cvo_fe_stereo_rig flat = rig;
        flat.baseline = 0.0f;
        const cvo_fe_camera_model pinhole{rig.depth_scale, rig.fx, rig.fy, rig.cx, rig.cy, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw * 2 != d.w * 3 || d.dh != d.h) throw std::runtime_error("the right image must have the left one's size");
            const cvo_hip::image_view left = d.rgb_view(), right{d.dep.data(), d.h, d.w, (size_t)d.w * 3};
            if (i == 0) {
                expect_refusal(d.lines, "a rig without settings", [&] { d.reg->set_stereo_rig(rig); });
                d.reg->set_stereo(st);
                expect_refusal(d.lines, "a bad rig", [&] { d.reg->set_stereo_rig(flat); });
                d.reg->set_stereo_rig(rig);
            }
            if (i == 2) {
                expect_refusal(d.lines, "a bad rig", [&] { d.reg->set_stereo_rig(flat); });
                expect_refusal(d.lines, "a camera model under a rig", [&] { d.reg->set_camera(pinhole); });
                expect_refusal(d.lines, "clear_stereo under a rig", [&] { d.reg->clear_stereo(); });
                d.reg->clear_stereo_rig();
                d.reg->set_stereo_rig(rig);
            }
            d.reg->run_cvo_stereo(/*dataset_seq*/ 4, left, right);
            d.cloud_line();
            d.pose_line();
        }
    });
}
