// Per-utterance lengths of an exact-lengths call (FaCodec decode, PVA flow, prior decode): the caller's host ints travel
// as kernel arguments (copied at launch, so the caller's array may go at once) into a handle-owned device array, written
// in stream order ahead of the kernels (or the graph replay) that read it.  A captured graph therefore holds no length,
// only the array's address.  (Where a sequence ends on the device: seqend.hpp.)
#pragma once
#include "common.hpp"

namespace fl {

constexpr int kLensChunk = 64;
struct LensChunk { int v[kLensChunk]; };
static __global__ __launch_bounds__(kLensChunk) void lens_put_kernel(LensChunk a, int cnt, int* __restrict__ dst) {
  const int i = threadIdx.x;
  if (i < cnt) dst[i] = a.v[i];
}

struct DevLens {
  int* d = nullptr;
  int cap = 0;
  void release() {
    if (d) (void)hipFree(d);
    d = nullptr;
    cap = 0;
  }
  // *moved: the array was reallocated (a graph keyed on its address is stale)
  int put(const int* lens, int B, hipStream_t st, bool* moved) {
    *moved = false;
    if (B > cap) {
      if (d) FL_HIP(hipFree(d));  // (waits for the work that may still read it)
      d = nullptr;
      cap = 0;
      const int n = (B + kLensChunk - 1) / kLensChunk * kLensChunk;
      FL_HIP(hipMalloc(&d, sizeof(int) * n));
      cap = n;
      *moved = true;
    }
    for (int b0 = 0; b0 < B; b0 += kLensChunk) {
      LensChunk a;
      const int cnt = B - b0 < kLensChunk ? B - b0 : kLensChunk;
      for (int i = 0; i < kLensChunk; ++i) a.v[i] = i < cnt ? lens[b0 + i] : 0;
      hipLaunchKernelGGL(lens_put_kernel, dim3(1), dim3(kLensChunk), 0, st, a, cnt, d + b0);
      FL_LAUNCH_CHECK();
    }
    return kOk;
  }
};

}  // namespace fl
