// cvo_lidar_sweep_demo.cpp -- registration::set_lidar_sweep / clear_lidar_sweep / set_lidar_motion of include/cvo.hpp:
// motion compensation of a spinning scan in the image form of run_cvo_lidar() (the sweep contract of cvo_frontend.h).
// The scan source, the sweep and the first twist are given BEFORE the first image, i.e. before the front end exists; a
// sweep without a scan source, a sweep with mode 0 and a twist over the cap are refused, before and after the front end
// exists; every frame runs under a twist of its own; after frame 1 the sweep is cleared and set again (the twist is
// zero after that until it is given), and after frame 2 the scan source is cleared, which takes the sweep with it.
// Per frame the cloud line and the pose line of the other demos.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_lidar, the cvo_fe_lidar_sweep and six floats of twist per
// frame; a frame's "depth image" of 128 x (n / 16) uint16 holds its scan, n records of four float32 (x y z and the
// time word), behind its own sizes.
// Build: g++ -std=c++17 -I include cvo_lidar_sweep_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

template <class Call> static void expect_throw(std::ostream &lines, const char *what, Call call)
{
    try {
        call();
        lines << "accepted " << what << "\n";
    } catch (const std::exception &) {
        lines << "refused " << what << "\n";
    }
}

static void try_bad(fe_demo::Demo &d, cvo_fe_lidar_sweep sweep)
{
    sweep.mode = 0;
    expect_throw(d.lines, "bad sweep", [&] { d.reg->set_lidar_sweep(sweep); });
    const float fast[6] = {0.0f, 1.5f, 0.0f, 0.0f, 0.0f, 0.0f};
    expect_throw(d.lines, "twist over the cap", [&] { d.reg->set_lidar_motion(fast); });
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_lidar lidar;
        cvo_fe_lidar_sweep sweep;
        d.read(&lidar, 1);
        d.read(&sweep, 1);
        std::vector<float> twists((size_t)6 * d.nf);
        d.read(twists.data(), twists.size());
        expect_throw(d.lines, "sweep without a scan source", [&] { d.reg->set_lidar_sweep(sweep); });
        expect_throw(d.lines, "twist without a sweep", [&] { d.reg->set_lidar_motion(twists.data()); });
        d.reg->set_lidar(lidar);
        d.reg->set_lidar_sweep(sweep);
        try_bad(d, sweep);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw != 128) throw std::runtime_error("a scan comes as rows of 16 records");
            if (i == 2) {
                try_bad(d, sweep);
                d.reg->clear_lidar_sweep();
                expect_throw(d.lines, "twist without a sweep", [&] { d.reg->set_lidar_motion(twists.data()); });
                d.reg->set_lidar_sweep(sweep);
            }
            if (i == 3) {
                d.reg->clear_lidar();
                expect_throw(d.lines, "twist without a sweep", [&] { d.reg->set_lidar_motion(twists.data()); });
                d.reg->set_lidar(lidar);   // (no sweep now: this frame is projected as it was measured)
            } else
                d.reg->set_lidar_motion(twists.data() + 6 * i);
            d.reg->run_cvo_lidar(/*dataset_seq*/ 1, d.rgb_view(), d.dep.data(), 16, 16 * d.dh);
            d.cloud_line();
            d.pose_line();
        }
    });
}
