// TEST-ONLY: the device buffers of one harness call (device_harness.hip, device_harness_points.hip): allocate, copy, launch, synchronise,
// free; the first HIP error sticks and every later step is skipped.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct DevBufs {
  void* p[8] = {};
  int k = 0;
  hipError_t err = hipSuccess;
  void* get(size_t bytes) {
    void* q = nullptr;
    if (err == hipSuccess) err = hipMalloc(&q, bytes ? bytes : 1);
    if (err == hipSuccess) p[k++] = q;
    return q;
  }
  void up(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && bytes) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  }
  void sync() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  int done() {
    for (int j = 0; j < k; ++j) (void)hipFree(p[j]);
    return err == hipSuccess ? 0 : -(int)err;
  }
};

}  // namespace
