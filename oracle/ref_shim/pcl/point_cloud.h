// Stand-in for <pcl/point_cloud.h>: the reference's cloud type only names the container.
#ifndef CVO_REF_SHIM_PCL_POINT_CLOUD
#define CVO_REF_SHIM_PCL_POINT_CLOUD
namespace pcl { template <typename P> struct PointCloud {}; }
#endif
