// What the host-only planning units share with the device headers: the host / device function qualifier and the layout of a
// pose's constants.  Plain C++ under g++, HIP under hipcc.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RSBA_HD __host__ __device__ __forceinline__
#else
#define RSBA_HD inline
#endif

namespace rsba {

// Per-camera constants, 32 doubles (256 B) per camera.
enum {
  CC_R = 0,      // 9: rotation matrix, row-major (I + [w]x in the small-angle branch)
  CC_K = 9,      // 9: left Jacobian Jl(w) (identity in the small-angle branch)
  CC_T = 18,     // 3: translation
  CC_FX = 21, CC_FY = 22, CC_PPX = 23, CC_PPY = 24,
  CC_SMALL = 25, // 1.0 when theta^2 <= DBL_EPSILON
  CC_STRIDE = 32
};

}  // namespace rsba
