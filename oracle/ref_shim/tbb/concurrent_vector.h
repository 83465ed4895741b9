// Stand-in for <tbb/concurrent_vector.h>: included by the reference's data types, never used by the selector.
#ifndef CVO_REF_SHIM_TBB
#define CVO_REF_SHIM_TBB
namespace tbb { template <typename T> class concurrent_vector {}; }
#endif
