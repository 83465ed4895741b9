// cvo_image_demo.cpp -- the reference's driver loop (ref src/cvo_main.cpp:17-66,
// adaptive_cvo_main.cpp) on the C++ mirror objects with IMAGES as input: every
// frame goes through run_cvo(dataset_seq, RGB_img, dep_img), which runs the GPU
// front end and the registration; a pose line per frame goes to stdout in the
// reference's format (default ostream precision).
// Input (fe_demo_common.hpp): a binary file written by the test, nothing behind the header.  (PNG decoding is
// the caller's: the reference uses cv::imread, ref src/cvo_main.cpp:100-106.)
// Build: g++ -std=c++17 -I include cvo_image_demo.cpp -L cvo-rgbd_amd/csrc -lcvo_hip
#include "fe_demo_common.hpp"

int main(int argc, char **argv)
{
    return fe_demo::run(argc, argv, 4, "demo frames.bin cvo|acvo dataset_seq", [argv](fe_demo::Demo &d) {
        const int dataset_seq = std::stoi(argv[3]);
        for (int i = 0; i < d.nf; ++i) {
            d.next_frame();
            d.reg->run_cvo(dataset_seq, d.rgb_view(), d.dep_view(), "unused.pcd", "unused.pcd");
            if (d.reg->init) d.pose_line();   // ref src/cvo_main.cpp:58-65
        }
    });
}
