// cvo_stereo_paths_demo.cpp -- registration::set_stereo_paths of include/cvo.hpp: the path mask of the stereo
// matcher (step 4 of the stereo contract of cvo_frontend.h) beside set_stereo() / run_cvo_stereo().
// Frames 0 and 1 run with the mask read from the file (set BEFORE the first image and before set_stereo(), i.e.
// before the front end exists), frame 2 with CVO_FE_PATHS_4 (the front end exists: the mask goes to it at once),
// frame 3 with the first mask again.  The masks 0 and 0x100 are refused, before and after the front end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the cloud the
// registration holds for that frame and, once initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_stereo and the mask (uint32); a frame's second image is
// the right colour image, stored as cvo_stereo_demo.cpp's.
// Build: g++ -std=c++17 -I include cvo_stereo_paths_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_mask(cvo_hip::registration &reg, unsigned mask, std::ostream &lines)
{
    try {
        reg.set_stereo_paths(mask);
        lines << "accepted a bad mask\n";
    } catch (const std::exception &) {
        lines << "refused a bad mask\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_stereo st;
        uint32_t mask;
        d.read(&st, 1);
        d.read(&mask, 1);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw * 2 != d.w * 3 || d.dh != d.h) throw std::runtime_error("the right image must have the left one's size");
            const cvo_hip::image_view left = d.rgb_view(), right{d.dep.data(), d.h, d.w, (size_t)d.w * 3};
            if (i == 0) {
                try_bad_mask(*d.reg, 0u, d.lines);
                d.reg->set_stereo_paths(mask);
                d.reg->set_stereo(st);
            }
            if (i == 2) d.reg->set_stereo_paths(CVO_FE_PATHS_4);
            if (i == 3) {
                try_bad_mask(*d.reg, 0x100u, d.lines);
                d.reg->set_stereo_paths(mask);
            }
            d.reg->run_cvo_stereo(/*dataset_seq*/ 4, left, right);
            d.cloud_line();
            d.pose_line();
        }
    });
}
