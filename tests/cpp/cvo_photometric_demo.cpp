// cvo_photometric_demo.cpp -- registration::set_photometric of include/cvo.hpp: the image form of run_cvo() with the
// colour image corrected on the device by a response table, a vignette and a gain per frame (the photometric contract
// of cvo_frontend.h).
// Frames 0 and 1 run under the stage (set BEFORE the first image, i.e. before the front end exists) with the gains
// of their own, frame 2 after clear_photometric(), frame 3 after the stage is set again (the front end exists: it goes
// to it at once).  Settings with both CVO_FE_PHOTO_GAIN and CVO_FE_PHOTO_AUTO are refused, before and after the front
// end exists.
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the settings (cvo_fe_photometric), the response table (3 x 256 uint16),
// the vignette (height x width uint16) and one gain (B G R, float32) per frame.
// Build: g++ -std=c++17 -I include cvo_photometric_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

static void try_bad_photometric(cvo_hip::registration &reg, cvo_fe_photometric bad, std::ostream &lines)
{
    bad.flags = CVO_FE_PHOTO_GAIN | CVO_FE_PHOTO_AUTO;
    try {
        reg.set_photometric(bad);
        lines << "accepted a bad photometric\n";
    } catch (const std::exception &) {
        lines << "refused a bad photometric\n";
    }
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_photometric set{};
        d.read(&set, 1);
        std::vector<uint16_t> response(768), vignette((size_t)d.w * d.h);
        d.read(response.data(), response.size());
        d.read(vignette.data(), vignette.size());
        std::vector<float> gains((size_t)3 * d.nf);
        d.read(gains.data(), gains.size());
        auto on = [&]() { d.reg->set_photometric(set, response.data(), vignette.data(), d.h, d.w, (size_t)d.w * 2); };
        try_bad_photometric(*d.reg, set, d.lines);
        on();
        for (int i = 0; i < d.nf; ++i) {
            if (i == 2) d.reg->clear_photometric();
            if (i == 3) {
                try_bad_photometric(*d.reg, set, d.lines);
                on();
            }
            if (i != 2) d.reg->set_photometric_gain(&gains[(size_t)3 * i]);
            d.next_frame();
            d.reg->run_cvo(/*dataset_seq*/ 1, d.rgb_view(), d.dep_view());
            d.cloud_line();
            d.pose_line();
        }
    });
}
