// cvo_stereo_speckle_demo.cpp -- registration::set_stereo_speckle of include/cvo.hpp: the speckle filter of the stereo
// matcher (the speckle contract of cvo_frontend.h) beside set_stereo() / run_cvo_stereo().
// Frames 0 and 1 run with the settings read from the file (set BEFORE the first image and before set_stereo(), i.e.
// before the front end exists; kept across frames), frame 2 without a filter (clear_stereo_speckle(): the front end
// exists, the call goes to it at once), frame 3 with the first settings again.  max_size 0 and max_diff 65536 are
// refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the
// registration holds for that frame and, once initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_stereo and the cvo_fe_speckle; a frame's second image is
// the right colour image, stored as cvo_stereo_demo.cpp's.
// Build: g++ -std=c++17 -I include cvo_stereo_speckle_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_speckle(cvo_hip::registration &reg, int32_t max_size, int32_t max_diff, std::ostream &lines)
{
    try {
        reg.set_stereo_speckle(cvo_fe_speckle{max_size, max_diff});
        lines << "accepted bad settings\n";
    } catch (const std::exception &) {
        lines << "refused bad settings\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_stereo st;
        cvo_fe_speckle sp;
        d.read(&st, 1);
        d.read(&sp, 1);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw * 2 != d.w * 3 || d.dh != d.h) throw std::runtime_error("the right image must have the left one's size");
            const cvo_hip::image_view left = d.rgb_view(), right{d.dep.data(), d.h, d.w, (size_t)d.w * 3};
            if (i == 0) {
                try_bad_speckle(*d.reg, 0, sp.max_diff, d.lines);
                d.reg->set_stereo_speckle(sp);
                d.reg->set_stereo(st);
            }
            if (i == 2) d.reg->clear_stereo_speckle();
            if (i == 3) {
                try_bad_speckle(*d.reg, sp.max_size, 65536, d.lines);
                d.reg->set_stereo_speckle(sp);
            }
            d.reg->run_cvo_stereo(/*dataset_seq*/ 4, left, right);
            d.cloud_line();
            d.pose_line();
        }
    });
}
