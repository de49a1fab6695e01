// jn_api.cpp — the entry points of libjn_stereo.so (include/jn_stereo.h) that belong to no module: the version, the hash the tests compare
// maps by, the device count and the plain device-memory helpers.  Product code.
//
// Every module keeps its C entry points beside its kernels or its handle:
//   the ELAS handle      elas_api.cpp (create, submit, wait ...), elas_batch.cpp (a slot's worker), elas_handle.h (what the two share)
//   the ELAS stage seams elas_seams.cpp (jn_host_stage, jn_host_triangulate*, jn_host_arrangement, jn_device_arrangement / _triangulate / _support_filters)
//   the node side        scan.hip (jn_disparity_to_u8, jn_build_valid_disp_lut, the scans, jn_point_cloud, the rectification maps and remap)
//   the other matchers and the navigation tails: sgm.hip, bm.hip, costmap.hip, subpix.hip, localmap.hip, plan.hip, route.hip, postfilter.hip,
//   ground.hip, jpeg.hip
#include "../../include/jn_stereo.h"
#include "hip_try.h"

extern "C" {

const char* jn_version(void) { return "jn_stereo 0.4 (gfx950)"; }

uint64_t jn_fnv1a64_u32(const uint32_t* words, int64_t n) {
  uint64_t h = 1469598103934665603ull;
  for (int64_t i = 0; i < n; i++) h = (h ^ words[i]) * 1099511628211ull;
  return h;
}

jn_status jn_device_count(int32_t* count) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) { *count = 0; return JN_ERR_NO_DEVICE; }
  *count = c;
  return c > 0 ? JN_OK : JN_ERR_NO_DEVICE;
}

// ---- device helpers -------------------------------------------------------------------------------
jn_status jn_device_malloc(int32_t device, int64_t bytes, void** out) {
  if (!out || bytes < 0) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(out, (size_t)bytes));
  return JN_OK;
}
jn_status jn_device_free(int32_t device, void* p) { HIP_TRY(hipSetDevice(device)); HIP_TRY(hipFree(p)); return JN_OK; }
jn_status jn_memcpy_h2d(int32_t device, void* dst, const void* src, int64_t bytes) {
  HIP_TRY(hipSetDevice(device)); HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice)); return JN_OK;
}
jn_status jn_memcpy_d2h(int32_t device, void* dst, const void* src, int64_t bytes) {
  HIP_TRY(hipSetDevice(device)); HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost)); return JN_OK;
}
jn_status jn_device_synchronize(int32_t device) { HIP_TRY(hipSetDevice(device)); HIP_TRY(hipDeviceSynchronize()); return JN_OK; }

}  // extern "C"
