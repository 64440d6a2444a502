// reg_core.hip -- C ABI (include/o3dslam_reg.h) + HIP kernels of the MI355X registration path.
// gfx950 only.  The product never falls back to a CPU path: every entry point that needs the
// device returns REG_DEVICE_ERROR when HIP fails.
#include "../../include/o3dslam_reg.h"
#include "../../include/o3dslam_reg_debug.h"
#include "host_math.hpp"
#include "reg_kernels.hpp"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

using namespace o3dreg;

// minimum waves per SIMD the search kernels are compiled for (2nd __launch_bounds__ argument): caps their VGPRs
#ifndef O3D_MATCH_WAVES
#define O3D_MATCH_WAVES 1
#endif
#ifndef O3D_SEARCH_WAVES
#define O3D_SEARCH_WAVES O3D_MATCH_WAVES
#endif

#include "reg_state.hpp"
#include "kernels_build.hpp"
#include "kernels_reading.hpp"
#include "kernels_match.hpp"
#include "kernels_fused.hpp"
#include "kernels_cloud64.hpp"
#include "kernels_mapprep.hpp"
#include "kernels_xicp.hpp"
#include "kernels_update.hpp"
#include "kernels_tail.hpp"
#include "kernels_neighbours.hpp"
#include "kernels_normals.hpp"
#include "kernels_pmextras.hpp"
#include "kernels_xicp_ternary.hpp"
#include "kernels_pmchain.hpp"
#include "kernels_pmoutliers.hpp"
#include "kernels_filters.hpp"
#include "kernels_octree.hpp"
#include "kernels_overlap.hpp"
#include "kernels_fpfh.hpp"
#include "kernels_ransac.hpp"
#include "kernels_scanprep.hpp"
#include "kernels_densemap.hpp"
#include "kernels_mapcloud.hpp"
#include "kernels_submaps.hpp"
#include "kernels_odometry.hpp"
#include "kernels_posegraph.hpp"

// host side: one handle = one non-re-entrant registration context (include/o3dslam_reg.h)
#include "host_mem.hpp"
#include "host_handle.hpp"
#include "host_prims.hpp"
#include "host_target.hpp"
#include "host_launch.hpp"
#include "host_loop.hpp"
#include "host_pm.hpp"
#include "host_dist.hpp"
#include "host_rccl.hpp"
#include "host_filters.hpp"
#include "host_octree.hpp"
#include "host_cloud_filters.hpp"
#include "host_overlap.hpp"
#include "host_fpfh.hpp"
#include "host_ransac.hpp"
#include "host_scanprep.hpp"
#include "host_densemap.hpp"
#include "host_mapcloud.hpp"
#include "host_odometry.hpp"
#include "host_posegraph.hpp"
#include "host_submaps.hpp"

#if O3D_SEARCH_STATS
// diagnostic builds only: read (and clear) the search counters of reg_kernels.hpp
extern "C" __attribute__((visibility("default"))) int o3d_debug_search_stats(unsigned long long out[96], int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(o3dreg::g_search_stats), 768) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[96] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(o3dreg::g_search_stats), z, 768) != hipSuccess) return -1;
    }
    return 0;
}
#endif
