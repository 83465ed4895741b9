// Stand-in for <opencv2/opencv.hpp>: the reference's frame type only names cv::Mat.
#ifndef CVO_REF_SHIM_OPENCV
#define CVO_REF_SHIM_OPENCV
namespace cv { struct Mat {}; }
#endif
