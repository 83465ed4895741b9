// Stand-in for <pcl/point_types.h>: the reference's cloud type only names the point.
#ifndef CVO_REF_SHIM_PCL_POINT_TYPES
#define CVO_REF_SHIM_PCL_POINT_TYPES
namespace pcl { struct PointXYZRGBA {}; }
#endif
