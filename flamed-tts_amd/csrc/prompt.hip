// Prompt-side FaCodec quantizers + timbre encoder on gfx950 (the part after the
// encoder conv stack): FACodecDecoder.forward(vq=True) (reference facodec.py:470-533).
//   * the three residual VQs (prosody, content on x; residual on x - (prosody + content)), each layer a
//     FactorizedVectorQuantize (quantize/fvq.py:35-116): weight-norm in_proj (C -> codebook_dim), L2
//     normalise, nearest normalised code by |e|^2 - 2 e.c + |c|^2 (first index on ties, as max(1)),
//     raw code row, straight-through z_e + (z_q - z_e), weight-norm out_proj, residual update
//     (quantize/rvq.py:27-73) -> one workgroup per frame runs all layers of all groups;
//   * the timbre TransformerEncoder (facodec/transformer.py:154-234; pre-LN layers :86-151, FFN
//     Conv1d(k) -> ReLU -> Linear :54-83), `x + pe[:B]` (the batch index selects the position vector,
//     :49-51), last LayerNorm, mean over time (facodec.py:530-532).
// Exact fp32 (codes must match the reference's argmax; f32 MFMA GEMMs are fp32 FMA chains).
// flamed_vq_encode_lens runs the same launches on a padded ragged batch, every utterance over its own frames and with
// position vector pe[0], as if alone (run_vq<true>).
#include "flamed_hip.h"
#include "flamed_diag.h"
#include "gemm.hpp"
#include "lens.hpp"
#include "seqend.hpp"
#include "xfmr.hpp"

#include <mutex>
#include <vector>

namespace fl {

// torch._weight_norm(v, g, dim=0) of a Linear weight: w[o][i] = v[o][i] * (g[o] / ||v[o]||_2).
__global__ void wn_rows_kernel(const float* __restrict__ g, const float* __restrict__ v, float* __restrict__ w, int rows,
                               int cols) {
  int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= rows) return;
  const float* vr = v + (size_t)o * cols;
  float s = 0.f;
  for (int i = 0; i < cols; ++i) s += vr[i] * vr[i];
  const float f = g[o] / sqrtf(s);
  for (int i = 0; i < cols; ++i) w[(size_t)o * cols + i] = vr[i] * f;
}

// F.normalize(codebook) (fvq.py:106) and the row sums of squares of the normalised codes (:110-112).
__global__ void cb_norm_kernel(const float* __restrict__ cb, float* __restrict__ cbn, float* __restrict__ cbsq, int K, int cd) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const float* r = cb + (size_t)k * cd;
  float s = 0.f;
  for (int j = 0; j < cd; ++j) s += r[j] * r[j];
  const float den = fmaxf(sqrtf(s), 1e-12f);
  float q = 0.f;
  for (int j = 0; j < cd; ++j) {
    float e = r[j] / den;
    cbn[(size_t)k * cd + j] = e;
    q += e * e;
  }
  cbsq[k] = q;
}

struct VqLayer {
  const float *win, *bin, *wout, *bout, *cb, *cbn, *cbsq;
  int K;
};
constexpr int kMaxVqLayers = 16;
struct VqParams {
  VqLayer l[kMaxVqLayers];
  int G;
  int nl[4];
};

// Exact lengths (flamed_vq_encode_lens): utterance b of the padded batch holds lens[b] frames.  The kernels below take
// that end through SeqEnd (seqend.hpp); the dense instantiation is the code it was.  PadCode is what a frame behind an
// end gets as its codes (empty in the dense form).
template <class End> struct PadCode {};
template <> struct PadCode<SeqEnd<true>> { int64_t v; };

// One workgroup (C = 256 threads, thread c = channel c) per frame (b, t); CD = codebook_dim.  A frame at or past its
// utterance's end reads nothing and writes pad.v to its codes and 0 to outs / qbuf (the buffers are reused).
template <int CD, class End = SeqEnd<false>>
__global__ __launch_bounds__(256) void rvq_kernel(VqParams P, const float* __restrict__ x, int B, int T,
                                                  float* __restrict__ outs, int64_t* __restrict__ codes,
                                                  float* __restrict__ qbuf, End end, PadCode<End> pad) {
  constexpr int C = 256;
  __shared__ float red[4][CD];
  __shared__ float ze_s[CD];
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int c = threadIdx.x, lane = c & 63, w = c >> 6;
  const int b = blockIdx.x / T, t = blockIdx.x - b * T;
  const size_t at = ((size_t)b * C + c) * T + t;  // (B, C, T) layouts
  if constexpr (End::kExact) {
    if (t >= end.end(b, T)) {  // blockIdx-uniform
      int nl = 0;
      for (int g = 0; g < P.G; ++g) {
        nl += P.nl[g];
        qbuf[(size_t)g * B * C * T + at] = 0.f;
      }
      for (int li = c; li < nl; li += C) codes[((size_t)li * B + b) * T + t] = pad.v;
      outs[at] = 0.f;
      return;
    }
  }
  const float xv = x[at];
  float gsum[4] = {0.f, 0.f, 0.f, 0.f};  // per-group quantized sums (qbuf)
  int li = 0;
  for (int g = 0; g < P.G; ++g) {
    float r = g < 2 ? xv : xv - (gsum[0] + gsum[1]);  // facodec.py:495-497
    for (int l = 0; l < P.nl[g]; ++l, ++li) {
      const VqLayer& L = P.l[li];
      // z_e = in_proj(r)
      float p[CD];
#pragma unroll
      for (int j = 0; j < CD; ++j) p[j] = wave_sum64(L.win[(size_t)j * C + c] * r);
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < CD; ++j) red[w][j] = p[j];
      }
      __syncthreads();
      if (c < CD) ze_s[c] = ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) + L.bin[c];
      __syncthreads();
      float ze[CD], nrm = 0.f;
#pragma unroll
      for (int j = 0; j < CD; ++j) {
        ze[j] = ze_s[j];
        nrm += ze[j] * ze[j];
      }
      const float den = fmaxf(sqrtf(nrm), 1e-12f);
      float enc[CD], esq = 0.f;
#pragma unroll
      for (int j = 0; j < CD; ++j) {
        enc[j] = ze[j] / den;
        esq += enc[j] * enc[j];
      }
      // nearest normalised code: max of -dist, lowest index on ties
      float best = -INFINITY;
      int bidx = 0x7fffffff;
      for (int k = c; k < L.K; k += C) {
        const float* cr = L.cbn + (size_t)k * CD;
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < CD; ++j) dot = fmaf(enc[j], cr[j], dot);
        const float nd = -((esq - 2.f * dot) + L.cbsq[k]);
        if (nd > best) { best = nd; bidx = k; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        float ov = __shfl_xor(best, o);
        int oi = __shfl_xor(bidx, o);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
      }
      if (lane == 0) { bv[w] = best; bi[w] = bidx; }
      __syncthreads();
      best = bv[0]; bidx = bi[0];
#pragma unroll
      for (int u = 1; u < 4; ++u)
        if (bv[u] > best || (bv[u] == best && bi[u] < bidx)) { best = bv[u]; bidx = bi[u]; }
      // straight-through value z_e + (z_q - z_e) (fvq.py:76-77), then out_proj for channel c
      const float* zq = L.cb + (size_t)bidx * CD;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < CD; ++j) q = fmaf(L.wout[(size_t)c * CD + j], ze[j] + (zq[j] - ze[j]), q);
      q += L.bout[c];
      r = r - q;                                     // rvq.py:60
      gsum[g] = l == 0 ? q : gsum[g] + q;            // rvq.py:62 (0.0 + q is q)
      if (c == 0) codes[((size_t)li * B + b) * T + t] = bidx;
      __syncthreads();  // red / ze_s / bv reuse by the next layer
    }
    qbuf[(size_t)g * B * C * T + at] = gsum[g];
  }
  float o = gsum[0];
  for (int g = 1; g < P.G; ++g) o = o + gsum[g];  // facodec.py:503 outs accumulation
  outs[at] = o;
}

// Timbre encoder input: x (B, C, T) -> rows (B*T, C) + pe[b] (transformer.py:49-51: pe[:x.size(0)]).
// Exact lengths: every utterance gets pe[0], the row it gets alone, and the rows from its end on are written as 0 and
// x is not read there, so every later row of the workspace is a finite function of finite data (a masked key's V row
// is multiplied by a zero weight: 0 x NaN would be NaN).
template <class End = SeqEnd<false>>
__global__ void timbre_in_kernel(const float* __restrict__ x, const float* __restrict__ pe, int B, int C, int T,
                                 float* __restrict__ X, End end) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C * T) return;
  int t = i % T;
  int bc = i / T;
  int c = bc % C, b = bc / C;
  if constexpr (End::kExact) {
    X[((size_t)b * T + t) * C + c] = t < end.end(b, T) ? x[i] + pe[c] : 0.f;
  } else {
    X[((size_t)b * T + t) * C + c] = x[i] + pe[(size_t)b * C + c];
  }
}

// The (B, T) key mask of an exact-lengths call (1 = behind the utterance's end) from the device lengths: what ln_mask
// (which zeroes the masked rows, the FFN conv's zero pad at the utterance's own end) and attention take.
__global__ void vq_mask_kernel(const int* __restrict__ lens, int B, int T, uint8_t* __restrict__ mask) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * T) return;
  int b = i / T, t = i - b * T;
  mask[i] = t >= lens[b];
}

// mean over time of the last-LayerNorm rows (facodec.py:531-532): spk[b][c] = sum_t Y[b][t][c] / T.  One workgroup
// per (64 channels, utterance); wave w sums the frames t = w (mod 8) and wave 0 adds the eight partials in wave
// order.  The sums are held in fp64: one fp32 running sum over T frames drifts by about sqrt(T / 3) roundings, which
// from a few hundred frames on is several times the error of the reference's pairwise fp32 mean.
// Exact lengths: the sum and the divisor end at the utterance's own end Te (the same frames in the same waves as alone).
constexpr int kMeanWaves = 8;
template <class End = SeqEnd<false>>
__global__ __launch_bounds__(64 * kMeanWaves) void mean_t_kernel(const float* __restrict__ Y, int T, int C,
                                                                 float* __restrict__ spk, End end) {
  __shared__ double part[kMeanWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane, b = blockIdx.y;
  const int Te = end.end(b, T);
  double s = 0.0;
  if (c < C)
    for (int t = w; t < Te; t += kMeanWaves) s += (double)Y[((size_t)b * T + t) * C + c];
  part[w][lane] = s;
  __syncthreads();
  if (w != 0 || c >= C) return;
  for (int u = 1; u < kMeanWaves; ++u) s += part[u][lane];
  spk[(size_t)b * C + c] = (float)(s / (double)Te);
}

__global__ void vq_taps_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int Cin, int KT) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * Cin * KT;
  if (i >= total) return;
  int k = i % KT;
  size_t t = i / KT;
  int c = t % Cin;
  int n = t / Cin;
  dst[((size_t)n * KT + k) * Cin + c] = src[i];
}

struct TimbreLayer {
  const float *g1, *b1, *wqkv, *bqkv, *wo, *bo, *g2, *b2, *w1, *c1b, *w2, *c2b;
};

struct PromptVq {
  int C = 0, cd = 0, G = 0, nl[4] = {0, 0, 0, 0}, K[4] = {0, 0, 0, 0};
  int d = 0, heads = 0, F = 0, k = 0, pe_len = 0;
  int device = -1;
  std::mutex mu;
  char* dev = nullptr;
  VqParams vp;
  const float* pe = nullptr;
  std::vector<TimbreLayer> tl;
  const float *lg = nullptr, *lb = nullptr;
  // exact lengths: a graph of its own whose kernels read this call's lengths from dlens and the key mask built from
  // them (dmask: B*T bytes, handle-owned so that the workspace is the dense call's)
  CapGraph graph, graph_l;
  DevLens dlens;
  uint8_t* dmask = nullptr;
  size_t mask_cap = 0;
  void release_graphs() {
    graph.release();
    graph_l.release();
    dlens.release();
    if (dmask) (void)hipFree(dmask);
    dmask = nullptr;
    mask_cap = 0;
  }
  int n_vq_layers() const { int s = 0; for (int g = 0; g < G; ++g) s += nl[g]; return s; }
};

static size_t a256p(size_t x) { return (x + 255) & ~(size_t)255; }

struct VqWs {
  float *X, *R, *H, *QKV, *O, *Hf;
};
static size_t vq_ws_layout(const PromptVq* p, int B, int T, void* base, VqWs* w) {
  const size_t M = (size_t)B * T;
  size_t sizes[6] = {4 * M * p->d, 4 * M * p->d, 4 * M * p->d, 12 * M * p->d, 4 * M * p->d, 4 * M * p->F};
  size_t off = 0;
  float* q[6];
  for (int i = 0; i < 6; ++i) {
    q[i] = base ? (float*)((char*)base + off) : nullptr;
    off += a256p(sizes[i]);
  }
  if (w) *w = VqWs{q[0], q[1], q[2], q[3], q[4], q[5]};
  return off;
}

// RAG: the exact-lengths form -- the same launches; `lens` (B device ints) ends every utterance through SeqEnd<true>,
// `mask` is the (B, T) key mask built from it.  RAG = false is the call as it always was (lens, mask null).
template <bool RAG>
static int run_vq(PromptVq* p, const float* x, int B, int T, float* outs, int64_t* codes, float* qbuf, float* spk,
                  const VqWs& w, hipStream_t st, const int* lens, uint8_t* mask, int64_t pad_code) {
  using End = SeqEnd<RAG>;
  const End end = End::make(lens, 1);
  PadCode<End> pad{};
  if constexpr (RAG) pad.v = pad_code;
  hipLaunchKernelGGL((rvq_kernel<8, End>), dim3(B * T), dim3(256), 0, st, p->vp, x, B, T, outs, codes, qbuf, end, pad);
  FL_LAUNCH_CHECK();
  const int M = B * T, d = p->d, F = p->F;
  hipLaunchKernelGGL(timbre_in_kernel<End>, dim3((B * d * T + 255) / 256), dim3(256), 0, st, x, p->pe, B, d, T, w.X, end);
  FL_LAUNCH_CHECK();
  if constexpr (RAG) {
    hipLaunchKernelGGL(vq_mask_kernel, dim3((M + 255) / 256), dim3(256), 0, st, lens, B, T, mask);
    FL_LAUNCH_CHECK();
  }
  float* X = w.X;
  float* R = w.R;
  int rc;
  for (const TimbreLayer& L : p->tl) {  // pre-LN layer, transformer.py:122-151
    if ((rc = ln_mask(d, X, L.g1, L.b1, mask, w.H, M, T, nullptr, 0, 0, 0, 0, st))) return rc;
    if ((rc = xf_gemm(LoadF32<float>{w.H, d}, L.wqkv, d, EpiBiasAct<float, 0>{L.bqkv, w.QKV, 3 * d}, M, 3 * d, d, st))) return rc;
    if ((rc = attention(d / p->heads, w.QKV, mask, B, T, d, p->heads, w.O, st))) return rc;
    if ((rc = xf_gemm(LoadF32<float>{w.O, d}, L.wo, d, EpiBiasRes{L.bo, X, R, d}, M, d, d, st))) return rc;
    std::swap(X, R);
    // the masked rows of H are 0: the k-tap FFN conv finds its zero pad at each utterance's own end
    if ((rc = ln_mask(d, X, L.g2, L.b2, mask, w.H, M, T, nullptr, 0, 0, 0, 0, st))) return rc;
    if ((rc = xf_gemm(LoadConvRows<float, false>{w.H, d, T, p->k, 1, nullptr, 0, 0, 0.f, nullptr, nullptr}, L.w1,
                                 p->k * d, EpiBiasAct<float, 3>{L.c1b, w.Hf, F}, M, F, p->k * d, st)))
      return rc;
    if ((rc = xf_gemm(LoadF32<float>{w.Hf, F}, L.w2, F, EpiBiasRes{L.c2b, X, R, d}, M, d, F, st))) return rc;
    std::swap(X, R);
  }
  if ((rc = ln_mask(d, X, p->lg, p->lb, mask, w.H, M, T, nullptr, 0, 0, 0, 0, st))) return rc;
  hipLaunchKernelGGL(mean_t_kernel<End>, dim3((d + 63) / 64, B), dim3(64 * kMeanWaves), 0, st, w.H, T, d, spk, end);
  FL_LAUNCH_CHECK();
  return kOk;
}

}  // namespace fl

using namespace fl;

extern "C" {

FLAMED_API int flamed_vq_create(const int* d, int nd, flamed_vq_t* out) {
  FL_REQUIRE(out && d && nd >= 3, "flamed_vq_create: bad dims");
  const int G = d[2];
  FL_REQUIRE(G >= 1 && G <= 4 && nd == 3 + 2 * G + 6, "flamed_vq_create: expected %d dims", 3 + 2 * G + 6);
  PromptVq* p = new PromptVq();
  p->C = d[0]; p->cd = d[1]; p->G = G;
  for (int g = 0; g < G; ++g) { p->nl[g] = d[3 + g]; p->K[g] = d[3 + G + g]; }
  const int* t = d + 3 + 2 * G;
  p->d = t[0]; p->heads = t[1]; p->F = t[2]; p->k = t[3]; p->pe_len = t[5];
  p->tl.resize(t[4] > 0 ? t[4] : 0);
  bool ok = p->C == 256 && p->cd == 8 && p->d == p->C && p->heads > 0 && p->d % p->heads == 0 &&
            (p->d / p->heads == 32 || p->d / p->heads == 48 || p->d / p->heads == 64) && p->F % 64 == 0 && (p->k & 1) &&
            p->pe_len > 0 && p->n_vq_layers() <= kMaxVqLayers && t[4] >= 0;
  for (int g = 0; g < G; ++g) ok = ok && p->nl[g] >= 1 && p->K[g] >= 1;
  if (!ok) {
    delete p;
    FL_REQUIRE(false, "flamed_vq_create: unsupported dims (C=256, codebook_dim=8, timbre hidden = C, head width 32/48/64)");
  }
  p->vp.G = G;
  for (int g = 0; g < G; ++g) p->vp.nl[g] = p->nl[g];
  *out = reinterpret_cast<flamed_vq_t>(p);
  return kOk;
}

FLAMED_API int flamed_vq_destroy(flamed_vq_t h) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  if (!p) return kOk;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    DeviceGuard dg(p->device);
    p->release_graphs();
    if (p->dev) (void)hipFree(p->dev);
  }
  delete p;
  return kOk;
}

FLAMED_API int flamed_vq_num_weights(flamed_vq_t h) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  return p ? 7 * p->n_vq_layers() + 1 + 12 * (int)p->tl.size() + 2 : -1;
}

FLAMED_API int flamed_vq_load(flamed_vq_t h, const float* const* w, int nw, hipStream_t st) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  FL_REQUIRE(p && w, "flamed_vq_load: null handle / weights");
  FL_REQUIRE(nw == flamed_vq_num_weights(h), "flamed_vq_load: expected %d weights, got %d", flamed_vq_num_weights(h), nw);
  for (int i = 0; i < nw; ++i) FL_REQUIRE(w[i], "flamed_vq_load: weight %d is null", i);
  int wdev = -1;
  FL_REQUIRE(device_of(w[0], &wdev) == kOk, "flamed_vq_load: weights must be device memory");
  for (int i = 1; i < nw; ++i) FL_REQUIRE_ON(w[i], wdev, "flamed_vq_load");
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->device >= 0 && p->device != wdev) {
    DeviceGuard og(p->device);
    p->release_graphs();
    if (p->dev) { (void)hipFree(p->dev); p->dev = nullptr; }
  }
  p->device = wdev;
  FL_ON_DEVICE(wdev);
  p->graph.release();
  p->graph_l.release();
  if (p->dev) { FL_HIP(hipFree(p->dev)); p->dev = nullptr; }
  const int C = p->C, cd = p->cd, d = p->d, F = p->F, k = p->k;
  // packed region: per VQ layer folded in/out weights, normalised codebook, code norms; per timbre layer
  // the tap-major conv weight
  size_t off = 0;
  std::vector<size_t> o_win, o_wout, o_cbn, o_cbsq, o_w1;
  for (int g = 0, li = 0; g < p->G; ++g)
    for (int l = 0; l < p->nl[g]; ++l, ++li) {
      o_win.push_back(off); off += a256p(4ull * cd * C);
      o_wout.push_back(off); off += a256p(4ull * C * cd);
      o_cbn.push_back(off); off += a256p(4ull * p->K[g] * cd);
      o_cbsq.push_back(off); off += a256p(4ull * p->K[g]);
    }
  for (size_t i = 0; i < p->tl.size(); ++i) { o_w1.push_back(off); off += a256p(4ull * F * k * d); }
  VecCopies vc;
  int i = 0;
  for (int g = 0, li = 0; g < p->G; ++g)
    for (int l = 0; l < p->nl[g]; ++l, ++li) {
      VqLayer& L = p->vp.l[li];
      L.K = p->K[g];
      vc.add(w[i + 2], cd, &L.bin);
      vc.add(w[i + 5], C, &L.bout);
      vc.add(w[i + 6], (size_t)p->K[g] * cd, &L.cb);
      i += 7;
    }
  vc.add(w[i++], (size_t)p->pe_len * d, &p->pe);
  for (TimbreLayer& L : p->tl) {
    vc.add(w[i + 0], d, &L.g1); vc.add(w[i + 1], d, &L.b1);
    vc.add(w[i + 2], 3ull * d * d, &L.wqkv); vc.add(w[i + 3], 3ull * d, &L.bqkv);
    vc.add(w[i + 4], (size_t)d * d, &L.wo); vc.add(w[i + 5], d, &L.bo);
    vc.add(w[i + 6], d, &L.g2); vc.add(w[i + 7], d, &L.b2);
    vc.add(w[i + 9], F, &L.c1b);
    vc.add(w[i + 10], (size_t)d * F, &L.w2); vc.add(w[i + 11], d, &L.c2b);
    i += 12;
  }
  vc.add(w[i], d, &p->lg);
  vc.add(w[i + 1], d, &p->lb);
  FL_HIP(hipMalloc(&p->dev, a256p(off) + a256p(vc.bytes)));
  char* base = p->dev;
  i = 0;
  for (int g = 0, li = 0; g < p->G; ++g)
    for (int l = 0; l < p->nl[g]; ++l, ++li) {
      VqLayer& L = p->vp.l[li];
      float* win = (float*)(base + o_win[li]);
      float* wout = (float*)(base + o_wout[li]);
      float* cbn = (float*)(base + o_cbn[li]);
      float* cbsq = (float*)(base + o_cbsq[li]);
      hipLaunchKernelGGL(wn_rows_kernel, dim3(1), dim3(64), 0, st, w[i + 0], w[i + 1], win, cd, C);
      hipLaunchKernelGGL(wn_rows_kernel, dim3((C + 63) / 64), dim3(64), 0, st, w[i + 3], w[i + 4], wout, C, cd);
      hipLaunchKernelGGL(cb_norm_kernel, dim3((p->K[g] + 255) / 256), dim3(256), 0, st, w[i + 6], cbn, cbsq, p->K[g], cd);
      FL_LAUNCH_CHECK();
      L.win = win; L.wout = wout; L.cbn = cbn; L.cbsq = cbsq;
      i += 7;
    }
  i += 1;
  for (size_t li = 0; li < p->tl.size(); ++li) {
    float* w1 = (float*)(base + o_w1[li]);
    const size_t n = (size_t)F * d * k;
    hipLaunchKernelGGL(vq_taps_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w[i + 8], w1, F, d, k);
    FL_LAUNCH_CHECK();
    p->tl[li].w1 = w1;
    i += 12;
  }
  return vc.commit(base + a256p(off), st);
}

FLAMED_API size_t flamed_vq_workspace_size(flamed_vq_t h, int B, int T) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  return p ? vq_ws_layout(p, B, T, nullptr, nullptr) : 0;
}

// Diagnostic (include/flamed_diag.h): byte offsets of the flamed_vq_encode workspace's buffers X, R, H, QKV, O, Hf
// (vq_ws_layout).  After an encode H holds the last-LayerNorm rows (B*T, d) that mean_t_kernel averages.
FLAMED_API int flamed_vq_ws_offsets(flamed_vq_t h, int B, int T, size_t* off) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  FL_REQUIRE(p && off && B > 0 && T > 0, "flamed_vq_ws_offsets: bad args");
  char* const base = reinterpret_cast<char*>(4096);  // any non-null base: offsets are relative to it
  VqWs w;
  vq_ws_layout(p, B, T, base, &w);
  const float* q[6] = {w.X, w.R, w.H, w.QKV, w.O, w.Hf};
  for (int i = 0; i < 6; ++i) off[i] = (size_t)((const char*)q[i] - base);
  return kOk;
}

// The call behind flamed_vq_encode (hlens null) and flamed_vq_encode_lens (hlens: B host lengths in frames, already
// checked).  `who` names the entry point in error messages.
static int vq_encode_call(PromptVq* p, const char* who, const float* x, int B, int T, const int* hlens, int64_t pad_code,
                          float* outs, int64_t* codes, float* qbuf, float* spk, void* ws, size_t ws_bytes, int use_graph,
                          hipStream_t st) {
  std::lock_guard<std::mutex> lk(p->mu);
  FL_ON_DEVICE(p->device);
  FL_REQUIRE_ON(x, p->device, who);
  const Tune tsnap = tune_snapshot(nullptr);
  TuneScope ts_(&tsnap);
  if (ws_bytes < vq_ws_layout(p, B, T, nullptr, nullptr)) {
    set_error("%s: workspace too small", who);
    return kNoWorkspace;
  }
  VqWs w;
  vq_ws_layout(p, B, T, ws, &w);
  std::vector<const void*> key = {x, outs, codes, qbuf, spk, ws, (const void*)(intptr_t)B, (const void*)(intptr_t)T, p->dev};
  if (!hlens)
    return with_graph(p->graph, key, use_graph != 0, st, [&](hipStream_t s) {
      return run_vq<false>(p, x, B, T, outs, codes, qbuf, spk, w, s, nullptr, nullptr, 0);
    });
  // lengths and key mask: handle-owned, the lengths written in stream order ahead of the kernels / the replay
  bool moved = false;
  const int rc = p->dlens.put(hlens, B, st, &moved);
  if (rc) return rc;
  const size_t need = (size_t)B * T;
  if (need > p->mask_cap) {
    if (p->dmask) FL_HIP(hipFree(p->dmask));  // (waits for the work that may still read it)
    p->dmask = nullptr;
    p->mask_cap = 0;
    FL_HIP(hipMalloc(&p->dmask, a256p(need)));
    p->mask_cap = a256p(need);
    moved = true;
  }
  if (moved) p->graph_l.retire();
  // the graph holds no length; the pad code is a kernel argument, so it is part of the key
  key.push_back(p->dlens.d);
  key.push_back(p->dmask);
  key.push_back((const void*)(intptr_t)pad_code);
  const int* dl = p->dlens.d;
  uint8_t* dm = p->dmask;
  return with_graph(p->graph_l, key, use_graph != 0, st, [&](hipStream_t s) {
    return run_vq<true>(p, x, B, T, outs, codes, qbuf, spk, w, s, dl, dm, pad_code);
  });
}

FLAMED_API int flamed_vq_encode(flamed_vq_t h, const float* x, int B, int T, float* outs, int64_t* codes, float* qbuf,
                                float* spk, void* ws, size_t ws_bytes, int use_graph, hipStream_t st) {
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  FL_REQUIRE(p && p->dev, "flamed_vq_encode: handle not loaded");
  FL_REQUIRE(x && outs && codes && qbuf && spk && ws && B > 0 && T > 0, "flamed_vq_encode: bad args");
  FL_REQUIRE(B <= p->pe_len, "flamed_vq_encode: B=%d exceeds the position table (%d rows)", B, p->pe_len);
  return vq_encode_call(p, "flamed_vq_encode", x, B, T, nullptr, 0, outs, codes, qbuf, spk, ws, ws_bytes, use_graph, st);
}

FLAMED_API int flamed_vq_encode_lens(flamed_vq_t h, const float* x, int B, int T, const int* lens, int64_t pad_code,
                                     float* outs, int64_t* codes, float* qbuf, float* spk, void* ws, size_t ws_bytes,
                                     int use_graph, hipStream_t st) {
  // every check of the arguments comes before any pointer is touched
  FL_REQUIRE(h && x && lens && outs && codes && qbuf && spk && ws,
             "flamed_vq_encode_lens: null handle, input, lengths, outs, codes, qbuf, spk or workspace");
  FL_REQUIRE(B > 0 && T > 0, "flamed_vq_encode_lens: bad dims B=%d T=%d", B, T);
  for (int u = 0; u < B; ++u)
    FL_REQUIRE(lens[u] >= 1 && lens[u] <= T, "flamed_vq_encode_lens: utterance %d has length %d (1..T = %d)", u, lens[u], T);
  // one full-length utterance: the dense call itself (pe[0] is pe[b] there).  B > 1 never is: the dense call adds pe[b]
  if (B == 1 && lens[0] == T) return flamed_vq_encode(h, x, B, T, outs, codes, qbuf, spk, ws, ws_bytes, use_graph, st);
  PromptVq* p = reinterpret_cast<PromptVq*>(h);
  FL_REQUIRE(p->dev, "flamed_vq_encode_lens: handle not loaded");
  return vq_encode_call(p, "flamed_vq_encode_lens", x, B, T, lens, pad_code, outs, codes, qbuf, spk, ws, ws_bytes, use_graph, st);
}

}  // extern "C"
