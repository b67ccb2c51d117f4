"""Frame and row error profiles for the prompt stage (csrc/prompt.hip): the six-layer residual VQ and the timbre
encoder behind FACodecDecoder.forward(vq=True).

The stage's one test (test_vq_timbre_vs_oracle) judged the timbre encoder through the speaker embedding, a mean over
time, by a global rel-L2 of 1e-4: a query that loses a key moves its own row by 1e-3 of the row RMS and the embedding
by 1e-5.  The profile looks at every row the mean averages and at every frame of the quantizers' outputs:

  refs(sd, sd64, x)            the fp64 and fp32 oracle of one input: orc.timbre_encoder (rows), orc.decoder_vq (codes,
                               spk, the fp32 top-2 gaps), orc.rvq_quantize per group (outs, qbuf) on a float64 copy of
                               the state dict and input, and the same in fp32
  emulated_timbre              orc.timbre_encoder restated with a `mutate(site, value, ctx)` hook; mutate = None is
                               the oracle bitwise (tests/test_promptprofile_cpu.py)
  row_err / spk_err            e[r] = ||out[r] - ref64[r]|| / sqrt(mean_r ||ref64[r]||^2) (tests/_xfmrprofile.py
                               row_errors) over the last-LayerNorm rows (B, T, 256); the speaker embedding (B, 256) on
                               the same scale (the RMS row norm of the rows it averages)
  frame_err                    the same over the channel axis of `outs` and each `qbuf[g]` (B, 256, T), each against
                               its own RMS frame norm, over the frames of `keep` only
  tied_state_dicts(sd)         three copies of the weights whose VQ codebooks hold exact duplicate rows:
                               "thread" cb[i + 512] = cb[i] (rvq_kernel's thread c walks k = c, c + 256, ...: one
                               thread sees both), "lane" cb[2m + 1] = cb[2m] (neighbouring lanes of one wave: the
                               shuffle butterfly), "wave" cb[1023 - i] = cb[i], i < 512 (wave w and wave 3 - w: the LDS
                               merge)
  gap_excluding_copies         the oracle's distance gap between the winner and the best code whose codebook row is
                               not a copy of the winner's (the plain top-2 gap is 0 on a tied codebook)
  bar_of(floor)                min(FACTOR_F32 x floor, F32_ROW_BAR): tests/_xfmrprofile.py's 4.0 and 1e-5

`mutate(site, value, ctx)` sites (CPU calibration only); ctx always holds layer (0..3; -1 after the last), B, T:
  "att"    logits (B, heads, T, T) before the softmax; ctx: qq, kk, vv (B, heads, T, hd), and `leak`, a list to which
           the hook may append (b, q, b2, key): query q of utterance b then also attends key `key` of utterance b2 in
           every head (logit, softmax and value of that row recomputed over T + 1 keys)
  "conv"   ffn_1 output (B, F, T) before the ReLU; ctx: x (its input (B, d, T)), w ((F, d, k))
  "rows"   the last-LayerNorm rows (B, T, d) before the mean; ctx: x (the encoder's input (B, T, d)), sd
  "spk"    the mean over time (B, d); ctx: rows

Inputs: torch.randn(B, 256, T) from Generator().manual_seed(1000 * B + T + 7919 * s), s = 0, 1 (case_input).

Floors (fp32 oracle against fp64 oracle, seeded decoder weights, this file's SHAPES, two seeds; max over the rows /
frames of a case, then the range over the 26 cases; tests/test_promptprofile_cpu.py prints the table; the fp32 oracle
is the CPU's BLAS, so another host moves single cases by up to 1.3 x, e.g. (1, 1) rows 1.9e-7 / 2.6e-7):

  rows   max 1.9e-7 .. 4.9e-7, median 1.9e-7 .. 4.5e-7; spk 5.3e-8 .. 3.2e-7 (falling with T: T <= 7 1.9 .. 3.2e-7,
         T 63 .. 193 0.7 .. 1.2e-7, T >= 481 5.3 .. 6.4e-8 -- the rows' errors average out in the mean)
  outs   frame max 1.07e-7 .. 1.67e-7    qbuf[0] (prosody, 1 layer)   7.4e-8 .. 2.2e-7
                                         qbuf[1] (content, 2 layers)  8.8e-8 .. 1.7e-7
                                         qbuf[2] (residual, 3 layers) 1.0e-7 .. 1.9e-7
  The fp32 oracle's codes equal the fp64 oracle's on every cell of every case (so the reference excludes no frame).
  Cells (layer, frame) whose fp32 top-2 gap is below 1e-5: 0 for every T <= 481; (1, 673): 1 / 0 of 4,038 (s = 0 / 1);
  (1, 2049): 2 / 3 of 12,294.

Planted bugs at (B, T) = (3, 161), seed 0, each on top of the fp32 oracle (test_planted_bugs_against_the_bars; row
floor 4.1e-7, bar 1.7e-6; spk floor 8.6e-8, bar 3.4e-7; "old" = the spk rel-L2 that test_vq_timbre_vs_oracle bounds
by 1e-4, the stage's only figure before):

  bug                                                       row max  x floor    x bar   spk err  x spk bar  old figure
  query 80 of utt 1 loses its last key, head 2, layer 0     1.07e-3   2.6e3     640     1.71e-5      50     1.3e-5 passed
  the same in layer 3                                       5.86e-4   1.4e3     350     3.82e-6      11     2.8e-6 passed
  queries 0..63 of utt 1 lose key 64, all heads, layer 0    8.81e-3   2.1e4    5300     2.11e-3    6200     1.6e-3 failed
  query 80 of utt 1 attends key 0 of utt 2, layer 0         1.52e-3   3.7e3     920     1.98e-5      58     1.5e-5 passed
  frame 0 of utt 1 reads utt 0's last frame, tap -1, l. 0   1.77e-1   4.3e5   1.1e5     2.08e-3    6100     1.6e-3 failed
  frame T-3 of utt 1 loses tap +2 (the last frame), l. 0    1.54e-1   3.7e5   9.3e4     1.82e-3    5300     1.4e-3 failed
  frame T-1 of utt 1 loses tap -2, layer 0                  1.64e-1   4.0e5   9.9e4     2.31e-3    6800     1.7e-3 failed
  the mean divides by T + 1                                 (floor)      1     0.25     4.81e-3   14000     6.2e-3 failed
  utterance 1 is encoded with pe[0]                         2.27e-1   5.5e5   1.4e5     1.76e-1   5.1e5     1.3e-1 failed
  Tap +2 of an utterance's LAST frame reads the reference's zero padding (test_last_frame_tap_plus_2_reads_padding):
  nothing is there to lose.  The two conv rows above are that bug's real neighbours: the frame that reaches the last
  frame through tap +2, and the last frame's farthest real tap.
  Every bug stands >= 350 x above the row bar (the mean bug: 14,000 x above the spk bar; needed: 1.5 x).  The old
  figure alone passed the three single-query attention bugs.  Judged by spk alone, the layer-3 bug would stand 11 x
  above the spk bar at this length and shrinks with T: the rows are what sees it.

Measured HIP / floor ratios on the MI355X (tests/test_prompt_profile_gpu.py, the 13 SHAPES, seed 0):
  rows, attn_mfma 1   1.37 .. 2.28   (row max 4.6e-7 .. 7.8e-7, median 4.6e-7 .. 6.6e-7)
  rows, attn_mfma 0   1.48 .. 2.29
  spk                 0.82 .. 1.83   (both kernels; T >= 193: 0.82 .. 1.27)
  outs                0.89 .. 1.04   qbuf[0] 0.84 .. 1.09, qbuf[1] 0.93 .. 1.06, qbuf[2] 0.90 .. 1.04
  codes               equal to the fp32 oracle's on every cell of every case, the five near-tie cells included; no
                      frame excluded; the three tied codebooks: 0 of 5,814 cells differ
  Finding: with mean_t_kernel's single fp32 running sum over T frames spk stood 1.5 .. 2.6 x its floor up to T = 193
  and 4.31 x at (1, 481) (2.4e-7 against a floor of 5.6e-8: the floor falls as 1 / sqrt(T), the running sum's drift
  grows as sqrt(T / 3) roundings; the rows themselves were at 2.1 x).  The kernel now sums in fp64, split over eight
  waves; the ratios above are with it.
"""
import math

import torch
import torch.nn.functional as F

from _common import orc
from _xfmrprofile import FACTOR_F32, F32_ROW_BAR, row_errors, to64, memo  # noqa: F401  (re-exported)
from _codecprofile import frame_errors  # noqa: F401

NEAR_TIE = 1e-5
N_Q = (1, 2, 3)
HEADS = 4

# (B, T): the smallest shapes that reach each edge of csrc/prompt.hip and csrc/xfmr.hpp on this handle (d = 256,
# 4 heads of 64, F = 1024, k = 5; attn_mfma_kernel<64, 4>: 64-query tiles, 2 key groups taking alternate 64-key chunks)
SHAPES = [
    (1, 1), (1, 2),              # T below the k = 5 halo; a single key; a single row in a 4-row LayerNorm block
    (3, 5),                      # an utterance edge every 5 rows; pe[b] for b > 0
    (9, 7),                      # M = 63; nine position vectors
    (2, 63), (1, 64), (2, 65),   # one full 64-query tile, then one extra; key group 1 empty, then holding one key
    (1, 129),                    # the third chunk, back on group 0, holding one key
    (1, 193),                    # a short last query tile
    (3, 161),                    # M = 483: past the conv GEMM's 32 x 32 tiles (M <= 480 at N = 1024); edges off the 32-row grid
    (1, 481), (1, 673),          # the conv switch point and the qkv switch point (M <= 672 at N = 768)
    (1, 2049),                   # past xf_gemm's M < 2048
]


def case_input(B, T, s=0):
    return torch.randn(B, 256, T, generator=torch.Generator().manual_seed(1000 * B + T + 7919 * s))


def decoder_sd():
    """The seeded FACodecDecoder weights (tests/_flamed_common.py build_flamed loads the same)."""
    from _common import seeded
    return memo("prompt_sd", lambda: seeded("facodec_decoder"))


def bar_of(floor):
    return min(FACTOR_F32 * floor, F32_ROW_BAR)


# ------------------------------------------------------------------------------------------------------------
# the oracle's timbre encoder restated with hooks (oracle/flamed_oracle.py timbre_encoder: the same torch calls on
# the same operands in the same order)
# ------------------------------------------------------------------------------------------------------------

def emulated_timbre(sd, x, mutate=None, p="timbre_encoder", n_layers=4, heads=HEADS):
    """x (B, T, d) -> the last-LayerNorm rows (B, T, d)."""
    B, T, d = x.shape
    x_in = x
    x = x + sd[p + ".position_emb.pe"][:B]
    hd = d // heads
    for i in range(n_layers):
        q = f"{p}.layers.{i}"
        h = F.layer_norm(x, (d,), sd[q + ".ln_1.weight"], sd[q + ".ln_1.bias"], 1e-5)
        qkv = F.linear(h, sd[q + ".self_attn.in_proj_weight"], sd[q + ".self_attn.in_proj_bias"])
        qq, kk, vv = (t.reshape(B, T, heads, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        logits = (qq / math.sqrt(hd)) @ kk.transpose(-1, -2)
        leak = []
        if mutate is not None:
            logits = mutate("att", logits, {"layer": i, "B": B, "T": T, "qq": qq, "kk": kk, "vv": vv, "leak": leak})
        a = torch.softmax(logits, dim=-1) @ vv
        for (b, qi, b2, key) in leak:
            extra = ((qq[b, :, qi] / math.sqrt(hd)) * kk[b2, :, key]).sum(-1, keepdim=True)      # (heads, 1)
            pr = torch.softmax(torch.cat([logits[b, :, qi], extra], dim=-1), dim=-1)              # (heads, T + 1)
            a = a.clone()
            a[b, :, qi] = (pr.unsqueeze(1) @ torch.cat([vv[b], vv[b2, :, key:key + 1]], dim=1)).squeeze(1)
        a = a.transpose(1, 2).reshape(B, T, d)
        x = x + F.linear(a, sd[q + ".self_attn.out_proj.weight"], sd[q + ".self_attn.out_proj.bias"])
        h = F.layer_norm(x, (d,), sd[q + ".ln_2.weight"], sd[q + ".ln_2.bias"], 1e-5)
        w = sd[q + ".ffn.ffn_1.weight"]
        hin = h.transpose(1, 2)
        h = F.conv1d(hin, w, sd[q + ".ffn.ffn_1.bias"], padding=w.shape[-1] // 2)
        if mutate is not None:
            h = mutate("conv", h, {"layer": i, "B": B, "T": T, "x": hin, "w": w})
        h = h.transpose(1, 2)
        x = x + F.linear(F.relu(h), sd[q + ".ffn.ffn_2.weight"], sd[q + ".ffn.ffn_2.bias"])
    rows = F.layer_norm(x, (d,), sd[p + ".last_ln.weight"], sd[p + ".last_ln.bias"], 1e-5)
    if mutate is not None:
        rows = mutate("rows", rows, {"layer": -1, "B": B, "T": T, "x": x_in, "sd": sd})
    return rows


def spk_of(rows, mutate=None):
    """The mean over time as orc.decoder_vq takes it: rows (B, T, d) -> (B, d)."""
    spk = rows.transpose(1, 2).mean(dim=2)
    if mutate is not None:
        spk = mutate("spk", spk, {"layer": -1, "B": rows.shape[0], "T": rows.shape[1], "rows": rows})
    return spk


# ------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------

def _side(sd, x, gaps=None):
    """One precision's oracle of x (B, 256, T): rows, spk, codes, outs, qbuf (list of G)."""
    rows = orc.timbre_encoder(sd, x.transpose(1, 2))
    codes, spk = orc.decoder_vq(sd, x, N_Q, gaps=gaps)
    op, _, qp = orc.rvq_quantize(sd, "quantizer.0", x, N_Q[0])
    oc, _, qc = orc.rvq_quantize(sd, "quantizer.1", x, N_Q[1])
    o_r, _, qr = orc.rvq_quantize(sd, "quantizer.2", x - (qp.sum(0) + qc.sum(0)), N_Q[2])
    return {"rows": rows, "spk": spk, "codes": codes, "outs": op + oc + o_r, "qbuf": [qp.sum(0), qc.sum(0), qr.sum(0)]}


def refs(sd, sd64, x):
    """{"r64": fp64 oracle, "r32": fp32 oracle (+ "gaps": (n_q, B, T) top-2 distance gaps)} of one input."""
    with torch.inference_mode():
        gaps = []
        r32 = _side(sd, x, gaps)
        r32["gaps"] = torch.stack(gaps)
        return {"r64": _side(sd64, x.double()), "r32": r32}


def case(B, T, s=0, sd=None, tag="seeded"):
    """(x, refs) of one seeded input, computed once per run and shared."""
    sd = decoder_sd() if sd is None else sd
    sd64 = memo(("prompt_sd64", tag), lambda: to64(sd))

    def make():
        x = case_input(B, T, s)
        return x, refs(sd, sd64, x)
    return memo(("prompt_case", tag, B, T, s), make)


# ------------------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------------------

def row_err(rows, rows64):
    """(B, T, d) x 2 -> (B * T,) float64."""
    return row_errors(rows, rows64)


def spk_err(spk, spk64, rows64):
    """(B, d) x 2 -> (B,) float64 on the scale of the rows the embedding averages."""
    r = torch.as_tensor(rows64, dtype=torch.float64)
    rms = torch.sqrt(r.reshape(-1, r.shape[-1]).pow(2).sum(1).mean())
    d = torch.as_tensor(spk, dtype=torch.float64) - torch.as_tensor(spk64, dtype=torch.float64)
    return torch.linalg.vector_norm(d, dim=1) / rms


def frame_err(out, ref64, keep=None):
    """(B, 256, T) x 2 [, keep (B, T) bool] -> (B * T,) float64: frame_errors over the kept frames (others report 0
    and stay out of the RMS)."""
    o, r = torch.as_tensor(out).transpose(1, 2), torch.as_tensor(ref64).transpose(1, 2)
    return row_errors(o, r, keep)


def floors(r):
    """The fp32 oracle's own distance to fp64: {"rows", "rows_median", "spk", "outs", "qbuf": [G]} (max over the case)."""
    r32, r64 = r["r32"], r["r64"]
    e = row_err(r32["rows"], r64["rows"])
    keep = (r32["codes"] == r64["codes"]).all(0)
    return {"rows": float(e.max()), "rows_median": float(e.median()),
            "spk": float(spk_err(r32["spk"], r64["spk"], r64["rows"]).max()),
            "outs": float(frame_err(r32["outs"], r64["outs"], keep).max()),
            "qbuf": [float(frame_err(a, b, keep).max()) for a, b in zip(r32["qbuf"], r64["qbuf"])]}


# ------------------------------------------------------------------------------------------------------------
# exact ties
# ------------------------------------------------------------------------------------------------------------
TIE_KINDS = ("thread", "lane", "wave")


def tied_state_dicts(sd):
    """{"thread" | "lane" | "wave": a copy of sd whose every VQ codebook (1024 rows) holds exact duplicates}; the
    lower index of every pair keeps its row."""
    out = {}
    keys = [k for k in sd if k.startswith("quantizer.") and k.endswith("._codebook.weight")]
    assert len(keys) == sum(N_Q)
    for kind in TIE_KINDS:
        t = dict(sd)
        for k in keys:
            cb = sd[k].clone()
            assert cb.shape[0] == 1024, cb.shape
            if kind == "thread":
                cb[512:] = cb[:512]
            elif kind == "lane":
                cb[1::2] = cb[0::2]
            else:
                cb[512:] = cb[:512].flip(0)  # cb[1023 - i] = cb[i]
            t[k] = cb
        out[kind] = t
    return out


def higher_of_pair(kind, idx):
    """Whether a code index is the higher one of its duplicate pair."""
    return (idx % 2 == 1) if kind == "lane" else (idx >= 512)


def _neg_dist(sd, p, z):
    """-dist (B * T, K) exactly as orc.fvq_quantize forms it."""
    B, D, T = z.shape
    z_e = orc._wn_linear(sd, p + ".in_proj", z.transpose(1, 2))
    e = F.normalize(z_e.reshape(B * T, -1))
    cb = F.normalize(sd[p + "._codebook.weight"])
    return -(e.pow(2).sum(1, keepdim=True) - 2 * e @ cb.t() + cb.pow(2).sum(1, keepdim=True).t())


def gap_excluding_copies(sd, x, n_q=N_Q):
    """(sum n_q, B, T): the oracle's -dist of the winner minus the best -dist among the codes whose codebook row
    differs from the winner's, along the oracle's own residual chain."""
    B, _, T = x.shape
    gaps = []

    def group(p, inp, n):
        res, qs = inp, []
        for i in range(n):
            lp = f"{p}.layers.{i}"
            q, idx = orc.fvq_quantize(sd, lp, res)
            nd = _neg_dist(sd, lp, res)
            cb = sd[lp + "._codebook.weight"]
            win = idx.reshape(-1)
            assert torch.equal(nd.max(1)[1], win)
            copies = (cb[win].unsqueeze(1) == cb.unsqueeze(0)).all(-1)
            best = nd.gather(1, win[:, None])[:, 0]
            gaps.append((best - nd.masked_fill(copies, -math.inf).max(1).values).reshape(B, T))
            res = res - q
            qs.append(q)
        return torch.stack(qs).sum(0)
    with torch.inference_mode():
        qp = group("quantizer.0", x, n_q[0])
        qc = group("quantizer.1", x, n_q[1])
        group("quantizer.2", x - (qp + qc), n_q[2])
    return torch.stack(gaps)
