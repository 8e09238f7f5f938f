// vy_support.h — what every host translation unit of libvyolo.so shares: the error channel behind vy_last_error() and the
// two macros that end a function on the first error.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vyolo.h"

// records the message for vy_last_error() (per thread) and returns `code` (defined in net.hip)
int vy_fail(int code, const char* fmt, ...);
#define fail vy_fail

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(VY_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// a step's error ends the sequence it is part of
#define VY_TRY(expr)                 \
  do {                               \
    if (int rc_ = (expr)) return rc_; \
  } while (0)
