// cvo_lidar_demo.cpp -- registration::set_lidar / clear_lidar / run_cvo_lidar of include/cvo.hpp: the image form of
// run_cvo() with a LiDAR scan in place of the depth image (projected into the colour camera on the device; the LiDAR
// contract of cvo_frontend.h).
// The settings are given BEFORE the first image, i.e. before the front end exists; settings with splat 4 are refused,
// before and after the front end exists; while they are set run_cvo() with a depth image, set_stereo() and
// set_depth_camera() throw; after frame 1 they are cleared and set again (the front end exists: both go to it at once).
// Per frame one line "cloud <name> <points> <digest of positions> <digest of features>" of the
// cloud the registration holds for that frame (cvo_hip_get_device_cloud, live rows) and, once
// initialised, the pose line of the reference's drivers.
// Input (fe_demo_common.hpp): behind the header the cvo_fe_lidar; a frame's "depth image" of 128 x (n / 16) uint16 holds
// its scan, n records of four float32 (x y z and one more), behind its own sizes.
// Build: g++ -std=c++17 -I include cvo_lidar_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
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

static void try_others(fe_demo::Demo &d, cvo_fe_lidar lidar)
{
    lidar.splat = 4;
    expect_throw(d.lines, "bad settings", [&] { d.reg->set_lidar(lidar); });
    cvo_fe_stereo stereo = {0.54f, 64, 1, 8, 32, 10, 1, 0};
    expect_throw(d.lines, "stereo", [&] { d.reg->set_stereo(stereo); });
    cvo_fe_depth_camera rig = {};
    rig.width = d.w; rig.height = d.h; rig.depth_scale = 5000.0f; rig.fx = rig.fy = 500.0f;
    rig.R[0] = rig.R[4] = rig.R[8] = 1.0f;
    expect_throw(d.lines, "depth camera", [&] { d.reg->set_depth_camera(rig); });
}

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 3, "demo frames.bin cvo|acvo", [](fe_demo::Demo &d) {
        cvo_fe_lidar lidar;
        d.read(&lidar, 1);
        d.reg->set_lidar(lidar);
        try_others(d, lidar);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame(true);
            if (d.dw != 128) throw std::runtime_error("a scan comes as rows of 16 records");
            if (i == 2) {
                try_others(d, lidar);
                expect_throw(d.lines, "depth image", [&] { d.reg->run_cvo(1, d.rgb_view(), d.rgb_view()); });
                d.reg->clear_lidar();
                expect_throw(d.lines, "scan", [&] { d.reg->run_cvo_lidar(1, d.rgb_view(), d.dep.data(), 16, 16 * d.dh); });
                d.reg->set_lidar(lidar);
            }
            d.reg->run_cvo_lidar(/*dataset_seq*/ 1, d.rgb_view(), d.dep.data(), 16, 16 * d.dh);
            d.cloud_line();
            d.pose_line();
        }
    });
}
