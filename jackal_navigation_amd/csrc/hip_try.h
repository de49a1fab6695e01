// hip_try.h — how the library reports a failed HIP call.  Product code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../../include/jn_stereo.h"

// Returns JN_ERR_NO_DEVICE from the calling function when a HIP call fails.  It prints its argument: keep the names of public constants
// out of it (tests/test_abi.py counts the library's strings).
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess) {                                                                \
      fprintf(stderr, "libjn_stereo: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
      return JN_ERR_NO_DEVICE;                                                              \
    }                                                                                       \
  } while (0)
