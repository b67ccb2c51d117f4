// Persistent B = 1 Euler solve: every step of ProbGenerator.sample's ODE loop (reference
// flamed/models/synthesizer/prob_generator.py:434-447; one SimpleMLPAdaLN.forward :349-365 per step)
// in ONE launch of 256 workgroups (one per CU), the phases of a step chained by in-launch hand-offs
// instead of 25 kernel boundaries.
//
// Work split (speed only; correctness never depends on placement).  Workgroup b is (group g, slot s); with the
// default persist_opt bit 8 the XCDs form a 2 x 4 grid: the round-robin dispatch puts b on XCD x = b % 8, which
// holds row groups 4 (x / 4) .. + 3 and slots 8 (x % 4) .. + 7 (so each weight panel is read by 2 XCDs and each
// group's hand-off rows by 4; without bit 8, g = b % 8 and s = b / 8: one group per XCD, every panel on all 8).
// Group g owns a contiguous range of <= 512 frames (equal shares of the utterance), processed as chunks of 64
// (four 16-row MFMA tiles, one per wave; NTW chunks: a kernel variant per chunk count); slot s owns hidden
// columns [32 s, 32 s + 32) and latent channels [8 s, 8 s + 8).  What stays on chip across phases:
//   * the residual stream X of the workgroup's (frames x 32 columns) tile, in registers;
//   * the Euler state x of its (frames x 8 channels), in registers across ALL steps (fp32);
//   * each GEMM phase's weight panel (32 output columns x K, bf16), LDS-DMA'd into one of two LDS
//     buffers by the previous GEMM phase, so a phase only waits for its activations.
// GEMM A operands (bf16 x_t, GroupNorm output, conv_2 / mlp.0 outputs, x * alpha) are handed over
// fragment-major (persist_opt 64, default): group g's rows as [16-row tile][32-wide K-step][lane][8 bf16],
// the exact register image of a v_mfma_f32_16x16x32_bf16 A operand, so each consumer wave's load of one
// K-step is one contiguous 1 KB (8 full lines) instead of 16 rows x 64 B (16 half-lines): the per-XCD L2
// request rate, not bytes, was what the A fetch waited on (2.4 -> 1.2 us per GEMM phase, 26.4 -> 22.8 ms).
// Every activation handed to another workgroup through a counter (bf16 GEMM operands, LayerNorm row partials,
// halo rows) is stored write-through (sc1), drained by every storing
// wave, then one lane adds to a counter; consumers poll with sc1 loads and read the data with sc1
// loads only (cdna_hip_programming.md §6 Guideline 16, table row 1: no release / acquire fences).
//   group counters  after each group phase (GEMM operands, partials) each of the 32 slots of g adds 1 to its shard's
//                           word: four words per group, eight adds each per hand-off (one word and 32 adds under
//                           persist_opt kOptOneWord and in the variants of one_word_variant; "counters" below)
//   GroupNorm       gn[s]:  the 8 groups' slot-s workgroups add 1 after publishing their partials (the counter form,
//                           persist_opt without 512)
// Two exchanges need no drain and no counter: their data is the flag.  Each value travels as an 8-byte {tag, fp32}
// granule (one relaxed agent-scope atomic store; readers re-read with atomic loads until every tag is the expected
// one), and the launch's reset prologue zeroes every tag, so none of an earlier launch matches:
//   GroupNorm partials gnp (persist_opt 512, default): tag = the number of the GroupNorm hand-off
//   conv_out boundary rows yb: Y0 of a workgroup's last row and Y2 of its first, 8 channels each, read only by the
//                           same-slot workgroups of the two neighbouring groups; tag = the launch's evaluation number.
//                           conv_out therefore signals nothing: the Euler update waits for 16 granules, not the grid.
// Per step: proj_in, 4 x (dwconv+GroupNorm, conv_2, conv_3, mlp.0, mlp.2), FinalLayer (dwconv+
// GroupNorm, conv_2, conv_3, conv_out), Euler update.  Numerics follow the bf16 launch path (bf16
// operands, fp32 accumulation / residual / statistics / state, the LayerNorm fold of mlp.0 and
// conv_out); GroupNorm statistics are exact per group (two passes) and Chan-combined across the 8
// groups in a fixed order (deterministic).  The grid is launched cooperatively (hipLaunchCooperativeKernel:
// all 256 workgroups co-resident, or the launch fails up front), so no wait depends on a workgroup that
// is not running.  Every spin is still bounded: a timeout sets the error word, every workgroup leaves and
// writes NaN into its part of x (a failed solve is loud, never silently wrong), and the first to set the
// word adds one to a sticky failure count the host reads after the fact (no host sync on the call path).
#pragma once
#include "common.hpp"

namespace fl {
namespace pk {

constexpr int kGroups = 8, kSlots = 32, kWGs = kGroups * kSlots, kThreads = 256;
constexpr int kH = 1024, kC = 256, kCols = kH / kSlots, kCh = kC / kSlots;
// A row group holds up to kMaxNTW chunks of kChunk = 64 frames (chunk i = 16-row tiles 4 i .. 4 i + 3, wave w owning
// tile 4 i + w): B x T <= 8 x 512 = 4096 frames (one 30 s utterance at 80 Hz is 2400; the reference's metadata
// batch of 4 at T = 1024).
constexpr int kChunk = 64, kMaxNTW = 8, kMaxRows = kChunk * kMaxNTW, kHalo = 15, kTaps = 31, kWin = kChunk + 2 * kHalo;
constexpr int kMaxNB = 8, kMaxT = kGroups * kMaxRows;
// LDS carve (bytes): two weight panels, the dwconv window (aliased by the epilogue staging tile), row
// statistics of the window, GroupNorm reduction scratch, poll flag
constexpr int kWPanel = kCols * kH * 2;
// dwconv window rows are padded to 36 floats: the transposed epilogue layout writes a lane's row as float4 pieces, and
// with a 32-float stride the 16 rows of one write would share 2 bank groups; at 36 they hit 16 distinct ones (and the
// depthwise conv's two rows per wave, 8 apart, fall in opposite bank halves)
constexpr int kHsLd = kCols + 4;
constexpr int L_HS = 2 * kWPanel;
constexpr int L_ST = L_HS + kWin * kHsLd * 4;
constexpr int L_RED = L_ST + (kMaxRows + 2 * kHalo) * 8;  // row statistics of the whole group window
constexpr int L_GNV = L_RED + 8 * kCols * 4;
constexpr int L_FLAG = L_GNV + kCols * 16;
constexpr int kLds = (L_FLAG + 16 + 15) / 16 * 16;
static_assert(kLds <= 160 * 1024, "persistent solve LDS");
// counters (ints); zeroed by the launch itself (its reset prologue)
//   [CT_GRP, CT_GN)   one word per row group, 64 B apart: the one-word image (32 adds per hand-off)
//   [CT_GN, CT_ERR)   GroupNorm, one word per slot, 64 B apart
//   CT_ERR            the error word, alone on its 128-B line        -- up to here the block every variant has had
//   [CT_SHD, kCtrInts) group arrivals, sharded: kShards words per row group, each on a 128-B line of its own.  Shard k
//                     takes the arrivals of slots 8 k .. 8 k + 7 (under the 2 x 4 XCD grid the group's eight workgroups
//                     on one XCD; under the other placements the same fixed partition), so a word sees 8 adds per
//                     hand-off instead of 32 and a consumer polls 4 words (the depthwise phase: all 32), each up to
//                     8 x the hand-off number
// A sharded variant zeroes all kCtrInts words (kResetInts per workgroup); a one-word variant only ever touches the
// first kCtrOneInts and zeroes those, 4 per workgroup, as before.
constexpr int kLineInts = 32, kShards = 4, kShardSlots = kSlots / kShards;
constexpr int CT_GRP = 0, CT_GN = 16 * kGroups, CT_ERR = CT_GN + 16 * kSlots, kCtrOneInts = CT_ERR + 16;
constexpr int CT_SHD = (kCtrOneInts + kLineInts - 1) / kLineInts * kLineInts;
constexpr int kCtrInts = CT_SHD + kGroups * kShards * kLineInts, kResetInts = 8;
static_assert(kCtrInts <= kWGs * kResetInts && kCtrOneInts <= kWGs * 4, "the reset prologue covers the block");
static_assert(CT_GN % kLineInts == 0 && CT_ERR % kLineInts == 0 && CT_ERR + kLineInts <= CT_SHD,
              "group words, GroupNorm words and the error word share no line");
constexpr int kOptOneWord = 1 << 22;
// Kernel variants <KH, NTW, RK2, RAG> that keep the one-word image at compile time (persist_opt kOptOneWord has nothing
// to select there): for them the hand-off code is the single-word code unchanged, registers and scratch included.  They
// are the variants whose sharded build needed more scratch than the single-word one
// (profiles/arrive_shard_resources.txt), the five-chunk Euler variant among them, which also measured slower sharded.
__host__ __device__ constexpr bool one_word_variant(bool KH, int NTW, bool RK2, bool RAG) {
  if (KH) return false;
  if (!RAG) return !RK2 ? (NTW == 4 || NTW == 5) : (NTW == 5 || NTW == 8);
  return !RK2 ? ((NTW >= 3 && NTW <= 5) || NTW == 7) : (NTW <= 3 || NTW == 5);
}
// Group hand-off image of a workgroup (group g, slot s) under persist_opt `opt`, worked out once before the step loop
// (host-callable for the CPU unit test, flamed_persist_ctr_layout): the word it signals (`sig`), the first word a wait
// for group g polls (`base`), and `sh`, from which the rest follows by shifts -- a group wait polls 1 << sh words, the
// all-group wait kGroups << sh from abase(), `stride()` ints apart, and every polled word must reach
// (kSlots x the hand-off number) >> sh.  sh = 2: the four shard words; sh = 0: the one word.
struct ArriveImage {
  int sig, base, sh;
  __host__ __device__ int n() const { return 1 << sh; }
  __host__ __device__ int an() const { return kGroups << sh; }
  __host__ __device__ int abase() const { return sh ? CT_SHD : CT_GRP; }
  __host__ __device__ int stride() const { return 16 << (sh >> 1); }
  __host__ __device__ int target(int L) const { return (kSlots * L) >> sh; }
};
static_assert((1 << 2) == kShards && (16 << 1) == kLineInts && (kSlots >> 2) == kShardSlots, "ArriveImage shifts");
__host__ __device__ inline ArriveImage arrive_image(int opt, int g, int s) {
  if (opt & kOptOneWord) return {CT_GRP + 16 * g, CT_GRP + 16 * g, 0};
  const int w = CT_SHD + g * kShards * kLineInts;
  return {w + (s / kShardSlots) * kLineInts, w, 2};
}
// sticky words (never reset; zeroed once at allocation): failed launches, and the two monotonic arrival
// counters of the reset prologue, each on a 128-B line of its own
constexpr int SY_FAILS = 0, SY_ARRIVE0 = 32, SY_ARRIVE1 = 64, SY_PFAIL = 96, kStickyInts = 128;

// Reset-prologue arrival tickets, wrap-safe: every launch adds exactly kWGs to each arrival counter (unsigned),
// and 2^32 is a multiple of kWGs, so the launch a ticket belongs to starts at ticket - ticket % kWGs on either
// side of the 32-bit wrap; its arrivals are complete once the counter has moved kWGs past that base, compared
// by signed difference.  (Host-callable for the CPU unit test: flamed_persist_ticket.)
__host__ __device__ inline unsigned arrive_target(unsigned ticket) {
  return ticket - ticket % (unsigned)kWGs + (unsigned)kWGs;
}
__host__ __device__ inline bool arrive_reached(unsigned cur, unsigned target) { return (int)(cur - target) >= 0; }

// LayerNorm row partials (Params::xpart), tile-major: [group][16-row tile of the group][slot][row in tile] float2, so
// the 16 rows a wave stores for one (tile, slot) are one 128-B line with a single writer (row-major, a row's 32 slots
// share two lines written 8 B at a time by 16 workgroups on 4 XCDs each).  A row is addressed as the fragment images
// are, by its group and its index in the group (group_rows); byte offset of (group g, row lrow of it, slot s):
constexpr int kGroupTiles = kMaxRows / 16;
constexpr unsigned kXpartBytes = (unsigned)kGroups * kGroupTiles * kSlots * 128u;
// (the row-major image, kMaxT rows of kSlots cells, fits the same buffer: the persistent layout allocates kXpartBytes)
static_assert(kXpartBytes >= (unsigned)kMaxT * kSlots * 8u, "row partial buffers");
__host__ __device__ inline unsigned xpart_off(int g, int lrow, int s) {
  return (unsigned)((((g * kGroupTiles + (lrow >> 4)) * kSlots + s) * 16 + (lrow & 15)) * 8);
}
// The group that owns frame i < Lu of an utterance (gi of its gpu = 8 / B groups) and the frame's index in that group:
// the inverse of group_rows (persist.hip), for a reader of another group's rows (the depthwise halo).  opt bit 2:
// whole 16-row tiles, group gi holding tiles [gi MT / gpu, (gi + 1) MT / gpu) -- the last gi with gi MT / gpu <= i / 16.
__host__ __device__ inline void row_owner(int i, int Lu, int gpu, int opt, int& gi, int& lrow) {
  if (opt & 2) {
    const int MT = (Lu + 15) >> 4;
    gi = (((i >> 4) + 1) * gpu - 1) / MT;
    lrow = i - 16 * (gi * MT / gpu);
    return;
  }
  const int R = (Lu + gpu - 1) / gpu;
  gi = i / R;
  lrow = i - gi * R;
}

struct BlockW {
  const bf16 *w2, *w3, *m0, *m2;
  const float *b2, *b3, *mb0, *mb2, *lnw, *lnb, *lnmw, *lnmb, *dww, *dwb, *gnw, *gnb;  // dww: tap-major (31, H)
};

struct Params {
  int T, NB, s0, s1;
  int B = 1;               // utterances (1, 2, 4 or 8), each T frames: utterance u owns row groups u 8/B .. + 8/B - 1
  int Bx = 0;              // > 0: only utterances < Bx carry data (a batch of 3 or 5..7 run as B = 4 / 8): the others
                           // compute on zeros, never read or write xt, and take modulation row Bx - 1 (mods hold
                           // nfe x Bx rows)
  float dt;
  const float* mods;
  int MS, MS0;
  const bf16* win;
  const float* bin;
  BlockW blk[kMaxNB + 1];  // [NB] = FinalLayer (w2, w3, b2, b3, dww, dwb, gnw, gnb)
  const bf16* wout;        // conv_out taps stacked (3 C) x H
  const float* bout;
  float* xt;               // Euler state (T x C), read at launch start, written at the end
  float2* xpart[2];        // LayerNorm row partials (mean, M2) over each slot's 32 columns, tile-major (xpart_off;
                           // persist_opt 2097152: row-major, T x 32); [0]
                           // from proj_in / mlp.2 (read by the next dwconv phase of EVERY group: halo
                           // rows), [1] from conv_3 (read by mlp.0 / conv_out of the same group) -- two
                           // buffers, so a group's conv_3 never overwrites what a slower neighbour's
                           // dwconv phase is still reading
  float* ximg;             // X rows (fp32) near the group edges: dwconv halo of the neighbouring groups
  bf16* a2;                // GroupNorm output = conv_2 operand, T x H
  bf16* u;                 // conv_2 / mlp.0 output = conv_3 / mlp.2 operand, T x H
  bf16* xa;                // x * alpha (LayerNorm fold) = mlp.0 / conv_out operand, T x H
  bf16* xs;                // bf16(x) = proj_in operand, T x C
  float4* gnp;             // GroupNorm partials (n, mean, M2) per (group, channel): 8 x H
  unsigned long long* yb;  // conv_out boundary rows per workgroup as {tag, fp32} granules: Y0 of its last row [0, 8),
                           // Y2 of its first [8, 16); tag = the launch's evaluation number (from 1), zeroed per launch
  int* ctr;
  int* seal;               // persist_opt 16384: per (group, slot) the number of its last group hand-off (16 B each)
  int* sticky;             // kStickyInts words never reset between launches: [SY_FAILS] failed launches so far
                           // (the host reads it after the fact), [SY_ARRIVE0/1] the reset prologue's arrivals
                           // (unsigned tickets), [SY_PFAIL] the last launch whose prologue failed (counted once)
  int inject_step = -1;    // diagnostic (flamed_tune persist_inject): every workgroup fails at this step
  int seal_skip = -1;      // diagnostic (flamed_tune persist_seal_skip): workgroup 5 does not store its seals in this step
  long long tmo;           // poll timeout, s_memrealtime ticks (100 MHz)
  int ntw = 1;             // row chunks (64 frames each) per group: the kernel variant (rows per group <= 64 ntw)
  int opt = 0;                        // experiment bits (flamed_tune persist_opt)
  unsigned long long* pst = nullptr;  // FL_STAMPS builds: timeline of step pst_step (persist_timeline.py)
  int pst_step = -1;
  float* gnd = nullptr;               // FL_STAMPS builds: GroupNorm exchange dump of step gnd_step (rowpart_probe.py)
  int gnd_step = -1;
  // two-stage second-order solver (the RK2 kernel variants; the Euler variants never read these): [s0, s1) then
  // counts velocity evaluations, two per step with s0 even, evaluation k reads modulation row block k;
  //   even k: y = x + adt v(x)        odd k: x = x + c1 (y - x) + c2dt v(y)
  int rk2 = 0;
  float adt = 0.f, c1 = 0.f, c2dt = 0.f;
  float* xbase = nullptr;  // the step's base x of the variants with >= 3 chunks per group (B T x C, thread-private
                           // elements: each thread stores and reloads its own)
  // The depthwise taps of block i once more, channel-major: (H, 32) fp32 with tap 31 zero, which a thread reads as
  // eight 16-B loads (the kernel variants up to four chunks per group; the others read blk[i].dww).  Behind every
  // older field: the variants that do not read it see the kernel arguments they always had.
  const float* dwc[kMaxNB + 1] = {};
  // Exact lengths (the ragged kernel variants only; appended, so every field above keeps its offset): utterance u
  // holds lens[u] <= T frames at rows u T .. u T + lens[u] - 1 and is solved over those alone -- its row groups split
  // lens[u], its GroupNorm divides by it, its zero padding sits at its own end, and rows u T + lens[u] .. (u + 1) T - 1
  // of xt and of every scratch image are neither read nor written.  Idle utterances (Bx) carry T.
  int lens[kGroups] = {};
};

// Host side (persist.hip): whether this device runs the 256-workgroup grid fully resident, and the launch.
bool persist_device_ok(int device);
// Row chunks per group for B utterances of T frames (group_rows' largest share; opt bit 2: whole 16-row tiles).
inline int persist_ntw(int B, int T, int opt) {
  const int gpu = kGroups / B;
  int R = (T + gpu - 1) / gpu;
  if (opt & 2) R = ((T + 15) / 16 + gpu - 1) / gpu * 16;
  return (R + kChunk - 1) / kChunk;
}
// ragged: the exact-lengths variants (Params::lens; several utterances only).
int persist_launch(const Params& P, hipStream_t st, bool cooperative = true, bool ragged = false);

}  // namespace pk
}  // namespace fl
