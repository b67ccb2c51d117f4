// Keyed noise (DESIGN.md "Keyed noise"): Philox4x32-10 keyed by an utterance's 64-bit seed and counted by the
// element's index inside its own utterance, Box-Muller normals in fp32, and the solve's initial state
// x = cond + temperature * n in the same pass.  Element (t, c) of an utterance is the same number whatever batch it
// sits in and whatever it is padded to.  Stateless: no handle, no allocation, no synchronisation; the seeds and the
// lengths travel as by-value kernel arguments (as in lens.hpp), at most 64 utterances per launch.
#include "common.hpp"
#include "flamed_diag.h"

namespace fl {

constexpr int kNoiseChunk = 64;
struct NoiseChunk {
  unsigned long long seed[kNoiseChunk];
  int len[kNoiseChunk];
};

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four 32-bit words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  w[0] = c0;
  w[1] = c1;
  w[2] = c2;
  w[3] = c3;
}

__device__ __forceinline__ void philox_block(unsigned long long seed, unsigned long long block, int stream_id, uint32_t w[4]) {
  philox4x32_10((uint32_t)block, (uint32_t)(block >> 32), (uint32_t)stream_id, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// Box-Muller on one word pair: u in (0, 1] and the turn fraction are 24-bit and exact in fp32; precise logf / sqrtf /
// sincosf (no fast intrinsics), and no multiply-add pattern a compiler could contract.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float* n0, float* n1) {
  const float u = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float th = 6.283185307179586f * ((float)(wb >> 8) * 0x1p-24f);
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincosf(th, &s, &c);
  *n0 = r * c;
  *n1 = r * s;
}

__device__ __forceinline__ void normal_block(unsigned long long seed, unsigned long long block, int stream_id, float n[4]) {
  uint32_t w[4];
  philox_block(seed, block, stream_id, w);
  box_muller(w[0], w[1], &n[0], &n[1]);
  box_muller(w[2], w[3], &n[2], &n[3]);
}

// One thread per Philox block = four consecutive elements of utterance blockIdx.y.  per: elements per utterance (T C);
// elements at or behind len * C are written 0.  VEC: per % 4 == 0 and 16-byte aligned cond / x, one 16-byte load and
// store per thread; otherwise scalar accesses with the same values.  x may alias cond (a thread reads its own four
// elements before it writes them), hence no __restrict__.
template <bool VEC>
__global__ __launch_bounds__(256) void noise_state_kernel(NoiseChunk a, const float* cond, int stream_id, float temperature,
                                                          long long per, int C, float* x) {
  const int u = blockIdx.y;
  const unsigned long long seed = a.seed[u];
  const long long valid = (long long)a.len[u] * C;
  const long long nblk = (per + 3) >> 2;
  const float* cu = cond ? cond + (size_t)u * per : nullptr;
  float* xu = x + (size_t)u * per;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nblk; j += (long long)gridDim.x * 256) {
    const long long e0 = j << 2;
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e0 < valid) {
      float n[4];
      normal_block(seed, (unsigned long long)j, stream_id, n);
      float cv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (cu) {
        if constexpr (VEC) {
          const float4 v = *reinterpret_cast<const float4*>(cu + e0);
          cv[0] = v.x, cv[1] = v.y, cv[2] = v.z, cv[3] = v.w;
        } else {
#pragma unroll
          for (int l = 0; l < 4; ++l)
            if (e0 + l < valid) cv[l] = cu[e0 + l];
        }
      }
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (e0 + l < valid) o[l] = cu ? fmaf(temperature, n[l], cv[l]) : temperature * n[l];
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(xu + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (e0 + l < per) xu[e0 + l] = o[l];
    }
  }
}

// (diagnostic) the raw Philox word of elements first .. first + n - 1 of one utterance
__global__ __launch_bounds__(256) void noise_bits_kernel(unsigned long long seed, int stream_id, unsigned long long first, int n,
                                                         uint32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long e = first + (unsigned long long)i;
  uint32_t w[4];
  philox_block(seed, e >> 2, stream_id, w);
  out[i] = w[e & 3];
}

}  // namespace fl

using namespace fl;

extern "C" {

FLAMED_API int flamed_noise_state(const float* cond, const unsigned long long* seeds, const int* lens, int stream_id,
                                  float temperature, int B, int T, int C, float* x, hipStream_t st) {
  FL_REQUIRE(x && seeds, "flamed_noise_state: null x or seeds");
  FL_REQUIRE(B >= 1 && T >= 1 && C >= 1, "flamed_noise_state: B, T, C must be >= 1 (got %d, %d, %d)", B, T, C);
  FL_REQUIRE(stream_id >= 0, "flamed_noise_state: stream_id must be >= 0 (got %d)", stream_id);
  if (lens)
    for (int u = 0; u < B; ++u)
      FL_REQUIRE(lens[u] >= 1 && lens[u] <= T, "flamed_noise_state: lens[%d] = %d outside 1..%d", u, lens[u], T);
  int dv = -1;
  (void)device_of(x, &dv);
  FL_ON_DEVICE(dv);
  const long long per = (long long)T * C;
  const long long nblk = (per + 3) >> 2;
  const bool vec = per % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(cond) & 15) == 0;
  const long long want = (nblk + 255) / 256;
  const unsigned gx = (unsigned)(want < 4096 ? want : 4096);  // grid-stride behind 4096 x 256 blocks per utterance
  for (int b0 = 0; b0 < B; b0 += kNoiseChunk) {
    NoiseChunk a;
    const int cnt = B - b0 < kNoiseChunk ? B - b0 : kNoiseChunk;
    for (int i = 0; i < kNoiseChunk; ++i) {
      a.seed[i] = i < cnt ? seeds[b0 + i] : 0ull;
      a.len[i] = i < cnt ? (lens ? lens[b0 + i] : T) : 0;
    }
    const float* cb = cond ? cond + (size_t)b0 * per : nullptr;
    float* xb = x + (size_t)b0 * per;
    if (vec)
      hipLaunchKernelGGL(noise_state_kernel<true>, dim3(gx, cnt), dim3(256), 0, st, a, cb, stream_id, temperature, per, C, xb);
    else
      hipLaunchKernelGGL(noise_state_kernel<false>, dim3(gx, cnt), dim3(256), 0, st, a, cb, stream_id, temperature, per, C, xb);
    FL_LAUNCH_CHECK();
  }
  return kOk;
}

FLAMED_API int flamed_noise_bits(unsigned long long seed, int stream_id, unsigned long long first_element, int n,
                                 unsigned int* out, hipStream_t st) {
  FL_REQUIRE(out && n >= 1 && stream_id >= 0, "flamed_noise_bits: bad args");
  int dv = -1;
  (void)device_of(out, &dv);
  FL_ON_DEVICE(dv);
  hipLaunchKernelGGL(noise_bits_kernel, dim3((n + 255) / 256), dim3(256), 0, st, seed, stream_id, first_element, n, out);
  FL_LAUNCH_CHECK();
  return kOk;
}

}  // extern "C"
