// cvo_stereo_demo.cpp -- registration::set_stereo / set_pcd_stereo / run_cvo_stereo of include/cvo.hpp: the
// image form of run_cvo() for two colour views of a rectified stereo pair, the depth matched on the device
// (the stereo contract of cvo_frontend.h).
// Frames 0 and 1 run with the settings read from the file (set BEFORE the first image, i.e. before the front
// end exists), frame 2 with the left-right test switched off (the front end exists: the settings go to it at
// once), frame 3 with the first settings again.  Settings with max_disp = 20 are refused, before and after the
// front end exists; the depth form of run_cvo() is refused while stereo is set, and run_cvo_stereo() before
// any settings.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the
// registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once initialised, the pose
// line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_stereo; a frame's second image is the right colour
// image, height rows of width*3 bytes, stored as a "depth image" of width*3/2 x height uint16 behind its own
// size (the width is even).
// Build: g++ -std=c++17 -I include cvo_stereo_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_settings(cvo_hip::registration &reg, cvo_fe_stereo st, std::ostream &lines)
{
    st.max_disp = 20;
    try {
        reg.set_stereo(st);
        lines << "accepted bad settings\n";
    } catch (const std::exception &) {
        lines << "refused bad settings\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_stereo st;
        d.read(&st, 1);
        cvo_fe_stereo no_lr = st;
        no_lr.lr_max = -1;
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw * 2 != d.w * 3 || d.dh != d.h) throw std::runtime_error("the right image must have the left one's size");
            const cvo_hip::image_view left = d.rgb_view(), right{d.dep.data(), d.h, d.w, (size_t)d.w * 3};
            if (i == 0) {
                try {
                    d.reg->run_cvo_stereo(/*dataset_seq*/ 4, left, right);
                    d.lines << "accepted a pair without settings\n";
                } catch (const std::exception &) {
                    d.lines << "refused a pair without settings\n";
                }
                try_bad_settings(*d.reg, st, d.lines);
                d.reg->set_stereo(st);
            }
            if (i == 2) d.reg->set_stereo(no_lr);
            if (i == 3) {
                try_bad_settings(*d.reg, st, d.lines);
                d.reg->set_stereo(st);
                try {
                    d.reg->run_cvo(4, left, right);
                    d.lines << "accepted a depth frame under stereo\n";
                } catch (const std::exception &) {
                    d.lines << "refused a depth frame under stereo\n";
                }
            }
            d.reg->run_cvo_stereo(/*dataset_seq*/ 4, left, right);
            d.cloud_line();
            d.pose_line();
        }
    });
}
