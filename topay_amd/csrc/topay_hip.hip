// libtopay_hip.so — kernels + host side of the C-ABI declared in include/topay.h.
// gfx950 (MI355X) only; built by `hipcc --offload-arch=gfx950 -shared -fPIC`.  No torch types, no CPU fallback:
// every entry point fails with TOPAY_ERR_NO_DEVICE when no HIP device is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <mutex>
#include <thread>
#include <string>
#include <vector>
#include <dlfcn.h>

#include "topay_solve.h"
#include "topay_feas.h"
#include "topay_edt.h"
#include "topay_front.h"
#include "topay_mcrrt.h"
#include "topay_jps.h"
#include "topay_topo.h"
#include "topay_plan.h"
#include "topay_track.h"
#include "topay_ee.h"
#include "topay_yaml.h"

#include "topay_kernels.h"
#include "topay_world.h"
#include "topay_sense.h"
#include "topay_mpc.h"

// host side, in this order: each header uses what the ones before it define
#include "topay_host_ctx.h"
#include "topay_host_maps.h"
#include "topay_host_batch.h"
#include "topay_host_results.h"
#include "topay_host_front.h"
#include "topay_host_dist.h"
#include "topay_host_plan.h"
#include "topay_host_world.h"
#include "topay_host_track.h"
#include "topay_host_ee.h"
#include "topay_host_sense.h"
#include "topay_host_mpc.h"
