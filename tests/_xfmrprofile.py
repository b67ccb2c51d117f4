"""Per-row error profiles for the prior transformer stack (csrc/prior.hip, csrc/xfmr.hpp).

A global rel-L2 divides an error confined to one row by sqrt(rows): one target row that is 30 % wrong in an
8 x 580-row batch adds 4.4e-3 to the bf16 decoders' global figure (floor 5-6e-3, bar 1e-2) and passes.  The
profile looks at every unpadded row, as tests/_rowprofile.py does for the denoiser:

  row_errors(out, ref, valid)  e[r] = ||out[r] - ref[r]|| / sqrt(mean_r' ||ref[r']||^2) in float64 over the unpadded
                               rows (padded rows report 0 and do not enter the RMS)
  to64, encode / decode_refs   the fp64 reference: the oracle's own functions (orc.fft_block, prior_encoder,
                               prior_decode) on a float64 copy of the state dict and inputs (a rebuilt sinusoid table
                               holds float32 values and is promoted)
  emulated_fft_block / emulated_encoder / emulated_decode
                               the oracle restated with a `round` hook on both operands (activation where
                               LoadF32<bf16> / LoadConvRows<bf16> round it, weight once) of every GEMM the HIP bf16
                               mode feeds with bf16 -- qkv, fc, conv1, conv2, bridge, head; bias, residual, LayerNorm
                               and softmax stay fp32 -- and a `mutate` hook that plants bugs.  round = identity gives
                               the oracle bitwise (tests/test_xfmrprofile_cpu.py).  acc64 = True accumulates the
                               rounded products in float64 (a second realization of the same floor).
  assert_row_profile           max row error of `out` <= factor x max row error of `floor_out`; no row exempt; in
                               f32 mode the bar is also capped at F32_ROW_BAR = 1e-5 absolute (the per-frame fp32 bar
                               of tests/_codecprofile.py).

Floors (measured on the reference alone): f32 = fp32 oracle against fp64 oracle, bf16 = bf16 emulation against the
fp64 oracle.

`mutate(site, value, ctx)` sites (CPU calibration only):
  "att"      masked logits (H*B, n, n) before the softmax; ctx: raw (unmasked), B, n, n_head, p (layer prefix)
  "conv1"    conv1 output (B, F, n) before the ReLU; ctx: x (rounded input (B, D, n)), w (rounded (F, D, k)), p
  "conv2"    conv2 output (B, D, n); ctx: x (rounded input (B, F, n)), w (rounded (D, F, k)), p
  "dec_in"   decoder q's input (B, P + T, D) before the position table; ctx: q, P, prompt_emb, target_emb
  "slice"    decoder q's target slice (B, T, D); ctx: q, P, full (the stack output (B, P + T, D))
  "head"     logits (B, nq, T, V + 1) before the mask; ctx: x (rounded embs), w, b

Factors
  FACTOR_BF16 = 2.0: the larger of 2.0 and 1.5 x the worst ratio between two realizations of the bf16 floor.  Over
      (B, T, P) = (2, 12, 20), (1, 65, 64), (2, 100, 221) with one block per stack and (3, 28, 20), (2, 96, 16),
      (3, 140, 84) on the full stack, embs and logits, a second input seed gives 0.95 .. 1.05 of the first seed's
      row max and fp64 instead of fp32 GEMM accumulation 0.96 .. 1.03 (test_bf16_floor_spread): 1.5 x 1.05 < 2.
      The floor is as flat as the denoiser's (row max over median 1.2 .. 1.3) although the softmax is peaky.
  FACTOR_F32 = 4.0, capped at F32_ROW_BAR = 1e-5 per row: the HIP fp32 path (MFMA FMA chains over K, __expf, the
      online softmax's other summation order) stands 1.33 .. 2.16 above the fp32 oracle's own distance to fp64 on
      the MI355X (table below); 4.0 is below 2 x 2.16.  The resulting bars are 7.9e-7 .. 2.6e-6, under 1/30 of the
      weakest planted bug's row max (8.7e-5).

Calibration (CPU, seeded weights, tests/test_xfmrprofile_cpu.py).  "small": one block on lens [129, 100] or a decode
(2, 40, 25) with one block per stack; "batch": one block on 8 x 580 rows (lens 580 .. 64) or a decode (8, 420, 160) with
one block per stack.  Row max | x floor | global rel-L2 and whether the global bar used alone would have passed
(decoder f32 1e-4, encoder 2e-5, bf16 1e-2).  Bugs (a)-(d) sit in the attention, which is fp32 in both modes, and are
judged in f32 mode; the GEMM-side bugs (e)-(j) in both.

  floors                                   f32 row max          bf16 row max
  one decoder block, small / batch         2.5e-7 / 2.8e-7      2.4e-3 / 2.3e-3
  one encoder block, small / batch         2.7e-7 / 2.7e-7      (the encoder is always fp32)
  decode, one block per stack, embs        4.3e-7 / 4.5e-7      3.9e-3 / 4.1e-3
  decode, one block per stack, logits      5.7e-7 / 6.0e-7      4.8e-3 / 4.9e-3
  decode, full stack (2, 40, 25)           5.4e-7, 6.4e-7       5.8e-3, 6.3e-3   (embs, logits)
  full encoder [97, 60]                    5.0e-7
  second seed (test_f32_floor_...): 2.8e-7 .. 6.6e-7 over the same cases, row max over median 1.16 .. 1.96

  one decoder block, f32                         small                                batch
  (a) query 70 loses key 63, all heads           1.16e-2  47294x  8.7e-4 failed       3.37e-3  12160x  6.6e-5 passed
  (b) query 70 loses key n-1 in head 1           3.86e-4   1571x  2.9e-5 passed       8.68e-5    313x  1.7e-6 passed
  (c) queries 32..63 lose key n-1, all heads     2.13e-2  86739x  5.1e-3 failed       4.59e-3  16546x  2.4e-4 failed
  (d) first padded key of utterance 1 attended   3.77e-2 153214x  1.1e-2 failed       1.13e-2  40691x  1.2e-3 failed
  one encoder block, f32
  (a)                                            1.08e-2  40363x  8.4e-4 failed       2.43e-3   8901x  4.9e-5 failed
  (b)                                            9.39e-3  35220x  7.3e-4 failed       1.27e-3   4659x  2.5e-5 failed
  (c)                                            3.17e-2 118715x  4.1e-3 failed       6.72e-3  24646x  2.7e-4 failed
  (d)                                            4.64e-2 174138x  1.2e-2 failed       1.53e-2  56211x  1.1e-3 failed
  (e) frame 0 of utterance 1 reads utterance 0
      through tap -4 only (k = 9)                2.02e-1   7.6e5x 1.3e-2 failed       1.87e-1   6.8e5x 3.2e-3 failed
  (f) last row of utterance 0 loses tap -1       1.80e-1   6.8e5x 1.2e-2 failed       2.09e-1   7.7e5x 3.6e-3 failed
  (i) conv2 drops the upper K/2 slice on rows
      32..63 x columns 64..95                    2.41e-1   9.0e5x 6.6e-2 failed       2.40e-1   8.8e5x 1.7e-2 failed
  one decoder block, bf16 (f32: the same row max, 5e5 .. 1.4e6 x the floor, global bar failed)
  (e) ... through tap -1 (k = 3)                 3.35e-1    140x  2.2e-2 failed       3.27e-1    141x  6.0e-3 passed
  (f)                                            3.09e-1    129x  2.1e-2 failed       3.33e-1    143x  6.1e-3 passed
  (i)                                            1.39e-1     58x  4.5e-2 failed       1.41e-1     60x  1.2e-2 failed
  decode, one block per stack, bf16 (f32: the same row max, global bar failed)
  (g) decoder 3's input row P gets prompt_emb    4.27e-2   10.9x  5.1e-3 passed       3.85e-2    9.3x  3.4e-3 passed
  (h) decoder 5's target slice shifted one row   5.65e-1    145x  1.1e-1 failed       5.50e-1    133x  8.5e-2 failed
  (j) head column 1024 from the zero padding     7.27e-2   15.3x  2.7e-2 failed       9.23e-2   19.0x  2.9e-2 failed
  (e) in the shared decoder's block              1.86e-1   47.5x  1.4e-2 failed       (at batch size: the one-block rows above)
  (f) in the shared decoder's block              1.86e-1   47.5x  1.3e-2 failed
  (i) in the shared decoder's block              9.76e-2   25.0x  1.6e-2 failed
  decode, full stack (2, 40, 25), bf16: (g) 4.3x, (h) 73x, (j) 11.8x, (e) 25.5x, (f) 24.8x, (i) 14.4x the floor
The weakest GEMM-side bug on the one-block configurations, (g), stands 4.7 x above the bf16 bar (needed: 1.5 x); on the
full stack, where later attention layers smear it, 2.1 x.

Measured HIP / floor row-max ratios on the MI355X per test family (tests/test_prior_profile_gpu.py; embs | logits):

  family                                             f32                          bf16
  one-block encoder, 8 ragged batches, attn_mfma 1   1.50 .. 1.94
  the same, attn_mfma 0                              1.50 .. 1.98
  full encoder ([129, 64, 1], 8 x 250)               1.33 .. 1.81
  one-block decode, 12 edge shapes, attn_mfma 1      1.81 .. 2.08 | 1.73 .. 1.92   0.98 .. 1.02 | 0.97 .. 1.04
  the same, attn_mfma 0                              1.77 .. 2.07 | 1.68 .. 1.87
  full decode, 14 dispatch shapes + batch            1.70 .. 2.06 | 1.61 .. 1.90   0.94 .. 1.03 | 0.94 .. 1.03
  split-K on / off (3 shapes), graph                                               0.99 .. 1.05 | 0.99 .. 1.04
  one utterance of (3, 64, 20) alone                 1.95 .. 2.16 | 1.78 .. 2.02   0.98 .. 1.03 | 0.96 .. 1.04
  decoder position override (max_seq_len 48)         1.73 .. 1.99 | 1.60 .. 1.79   1.00 .. 1.03 | 0.97 .. 0.98
f32 row max 3.0e-7 .. 1.02e-6 everywhere (cap 1e-5).  bf16: the emulation has the rounding points the kernels have.
An utterance decoded alone equals the same utterance inside the batch bitwise in f32 mode at the tested shape; in
bf16 mode the two differ at floor level (row max 3.5e-3 .. 4.7e-3: another split-K slice count changes fp32 sums
in the last bit, and the next bf16 rounding amplifies that), each within the bar of the fp64 oracle.
"""
import torch
import torch.nn.functional as F
import numpy as np

from _common import orc

FACTOR_BF16 = 2.0
FACTOR_F32 = 4.0
F32_ROW_BAR = 1e-5


def bf16_round(x):
    """bf16 round-to-nearest-even of an fp32 tensor, kept as fp32."""
    return x.to(torch.bfloat16).float()


def _ident(x):
    return x


def to64(sd):
    """float64 copy of a state dict (integer tensors untouched)."""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def row_errors(out, ref, valid=None):
    """(B, n, D) x 2 [, valid (B, n) bool] -> (B*n,) float64: per-row error norm over the global RMS row norm of ref,
    both over the unpadded rows only (padded rows report 0)."""
    o = torch.as_tensor(out, dtype=torch.float64)
    r = torch.as_tensor(ref, dtype=torch.float64)
    assert o.shape == r.shape and o.dim() == 3, (o.shape, r.shape)
    D = o.shape[-1]
    v = torch.ones(o.shape[:2], dtype=torch.bool) if valid is None else torch.as_tensor(valid, dtype=torch.bool)
    v = v.reshape(-1)
    assert v.numel() == o.shape[0] * o.shape[1] and bool(v.any())
    num = torch.linalg.vector_norm((o - r).reshape(-1, D), dim=1)
    rms = torch.sqrt(r.reshape(-1, D).pow(2).sum(1)[v].mean())
    return torch.where(v, num / rms.clamp_min(1e-300), torch.zeros_like(num))


def logit_rows(logits):
    """(B, V + 1, nq, T) -> (B, nq * T, V + 1): one row per (quantizer, frame)."""
    B, V1, nq, T = logits.shape
    return logits.permute(0, 2, 3, 1).reshape(B, nq * T, V1)


def emb_rows(embs):
    """(B, nq, T, D) -> (B, nq * T, D)."""
    B, nq, T, D = embs.shape
    return embs.reshape(B, nq * T, D)


# ------------------------------------------------------------------------------------------------------------
# the oracle restated with hooks (oracle/flamed_oracle.py: fft_block, prior_encoder, prior_decoder_stack,
# prior_decode -- the same torch calls on the same operands in the same order)
# ------------------------------------------------------------------------------------------------------------

def _lin(x, w, b, rnd, acc64):
    x, w = rnd(x), rnd(w)
    if acc64:
        return F.linear(x.double(), w.double(), b.double()).float()
    return F.linear(x, w, b)


def _conv(x, w, b, rnd, acc64):
    """Conv1d with `same` zero padding on rounded operands -> (output, rounded x, rounded w)."""
    x, w = rnd(x), rnd(w)
    pad = (w.shape[-1] - 1) // 2
    if acc64:
        return F.conv1d(x.double(), w.double(), b.double(), padding=pad).float(), x, w
    return F.conv1d(x, w, b, padding=pad), x, w


def emulated_fft_block(sd, p, x, mask, n_head, round=bf16_round, mutate=None, acc64=False):
    """orc.fft_block with `round` on both operands of qkv, fc, conv1 and conv2 and `mutate` at the logits and the
    two conv outputs."""
    rnd = _ident if round is None else round
    B, n, D = x.shape
    dk = D // n_head
    a = p + ".slf_attn."

    def heads(name):
        return _lin(x, sd[a + name + ".weight"], sd[a + name + ".bias"], rnd, acc64).view(B, n, n_head, dk) \
            .permute(2, 0, 1, 3).reshape(n_head * B, n, dk)

    q, k, v = heads("w_qs"), heads("w_ks"), heads("w_vs")
    raw = torch.bmm(q, k.transpose(1, 2)) / float(np.power(dk, 0.5))
    att = raw.masked_fill(mask.unsqueeze(1).expand(-1, n, -1).repeat(n_head, 1, 1), -np.inf)
    if mutate is not None:
        att = mutate("att", att, {"raw": raw, "B": B, "n": n, "n_head": n_head, "p": p})
    o = torch.bmm(torch.softmax(att, dim=2), v).view(n_head, B, n, dk).permute(1, 2, 0, 3).reshape(B, n, D)
    o = _lin(o, sd[a + "fc.weight"], sd[a + "fc.bias"], rnd, acc64)
    x = F.layer_norm(o + x, (D,), sd[a + "layer_norm.weight"], sd[a + "layer_norm.bias"], 1e-5)
    x = x.masked_fill(mask.unsqueeze(-1), 0)
    f = p + ".pos_ffn."
    h, xr, wr = _conv(x.transpose(1, 2), sd[f + "w_1.weight"], sd[f + "w_1.bias"], rnd, acc64)
    if mutate is not None:
        h = mutate("conv1", h, {"x": xr, "w": wr, "p": p})
    h, xr, wr = _conv(F.relu(h), sd[f + "w_2.weight"], sd[f + "w_2.bias"], rnd, acc64)
    if mutate is not None:
        h = mutate("conv2", h, {"x": xr, "w": wr, "p": p})
    h = h.transpose(1, 2)
    x = F.layer_norm(h + x, (D,), sd[f + "layer_norm.weight"], sd[f + "layer_norm.bias"], 1e-5)
    return x.masked_fill(mask.unsqueeze(-1), 0)


def _pos(sd, p, n):
    pe = sd[p + ".position_enc"][0]
    return orc.sinusoid_table(n, pe.shape[-1]) if n > pe.shape[0] - 1 else pe[:n]


def emulated_encoder(sd, texts, src_mask, round=None, mutate=None, acc64=False, p="prior_generator.encoder", n_head=4):
    """orc.prior_encoder over emulated_fft_block (the HIP encoder is always fp32: round defaults to identity)."""
    B, n = texts.shape
    x = F.embedding(texts, sd[p + ".src_word_emb.weight"]) + _pos(sd, p, n).unsqueeze(0).expand(B, -1, -1)
    for i in range(orc._n_layers(sd, p)):
        x = emulated_fft_block(sd, f"{p}.layer_stack.{i}", x, src_mask, n_head, round, mutate, acc64)
    return x


def _stack(sd, p, x, mask, n_head, rnd, mutate, acc64):
    B, n, _ = x.shape
    x = x + _pos(sd, p, n).unsqueeze(0).expand(B, -1, -1)
    for i in range(orc._n_layers(sd, p)):
        x = emulated_fft_block(sd, f"{p}.layer_stack.{i}", x, mask, n_head, rnd, mutate, acc64)
    return x


def emulated_decode(sd, x_lr, tgt_lens, prompts, round=bf16_round, mutate=None, acc64=False, p="prior_generator",
                    n_head=12):
    """orc.prior_decode with `round` on the bridge, every decoder block's four GEMMs and the head, and `mutate` at
    the decoder inputs, the target slices and the head."""
    rnd = _ident if round is None else round
    B, T, _ = x_lr.shape
    P = prompts.shape[-1]
    tgt_mask = orc.mask_from_lengths(tgt_lens, T)
    out = _stack(sd, p + ".shared_decoder", _lin(x_lr, sd[p + ".bridge.weight"], sd[p + ".bridge.bias"], rnd, acc64),
                 tgt_mask, n_head, rnd, mutate, acc64)
    dec_mask = orc.mask_from_lengths(P + tgt_lens, P + T)
    pemb = F.embedding(prompts, sd[p + ".code_embedding.weight"])
    hid = []
    nq = prompts.shape[1]
    for q in range(nq):
        z = torch.cat([pemb[:, q], out], dim=1)
        z = torch.cat([z[:, :P] + sd[p + ".pre_encode.prompt_emb"], z[:, P:] + sd[p + ".pre_encode.target_emb"]], 1)
        if mutate is not None:
            z = mutate("dec_in", z, {"q": q, "P": P, "prompt_emb": sd[p + ".pre_encode.prompt_emb"],
                                     "target_emb": sd[p + ".pre_encode.target_emb"]})
        z = z + sd[p + ".pre_encode.quantizer_emb.weight"][q]
        full = _stack(sd, f"{p}.prior_decoder.{q}", z, dec_mask, n_head, rnd, mutate, acc64)
        out = full[:, P:]
        if mutate is not None:
            out = mutate("slice", out, {"q": q, "P": P, "full": full})
        hid.append(out.unsqueeze(1))
    embs = torch.cat(hid, dim=1)
    xr, wr = rnd(embs), rnd(sd[p + ".head.weight"])
    if acc64:
        logits = F.linear(xr.double(), wr.double(), sd[p + ".head.bias"].double()).float()
    else:
        logits = F.linear(xr, wr, sd[p + ".head.bias"])
    if mutate is not None:
        logits = mutate("head", logits, {"x": xr, "w": wr, "b": sd[p + ".head.bias"]})
    logits = logits * ~tgt_mask.unsqueeze(1).expand(-1, nq, -1).unsqueeze(3)
    return embs, logits.permute(0, 3, 1, 2).contiguous(), tgt_mask


# ------------------------------------------------------------------------------------------------------------
# models: configs/prior.yaml, optionally with one FFT block per stack (a localized bug is not smeared by later
# attention layers) and a lowered decoder position table; seeded as build_flamed seeds the full model
# ------------------------------------------------------------------------------------------------------------

def prior_config(reduced=False, dec_max_seq=None):
    import os
    import yaml
    from _common import PKG
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prior.yaml")))
    tc = cfg["transformer"]
    if reduced:
        tc["encoder_layer"] = 1
        tc["decoder_shared_layers"] = 1
        tc["decoder_layers"] = [1] * len(tc["decoder_layers"])
    if dec_max_seq is not None:
        tc["decoder_max_seq_len"] = dec_max_seq
    return cfg


def build_prior(reduced=False, dec_max_seq=None, seed=None):
    """(PriorGenerator (eval, CPU, hip_dec_dtype "f32"), oracle state dict with the "prior_generator." prefix)."""
    from _common import SEED, fill_state_dict
    from flamed.models.synthesizer.prior_generator import PriorGenerator
    pg = PriorGenerator(prior_config(reduced, dec_max_seq)).eval()
    sd = fill_state_dict({"prior_generator." + k: v for k, v in pg.state_dict().items()}, SEED if seed is None else seed)
    pg.load_state_dict({k[len("prior_generator."):]: v for k, v in sd.items()})
    pg.hip_dec_dtype = "f32"
    return pg, sd


# ------------------------------------------------------------------------------------------------------------
# the GEMM dispatch of the decoder side, restated from csrc (xfmr.hpp xf_gemm, prior.hip pr_gemm, gemm.hpp pick_cfg
# and choose_split with Prior::kSplitTarget = 512, max_split = 4, 2,048 counters, a 512 x 32 x 64-float slab): the
# GPU tests pick their row counts from it and check its split prediction against what the library does
# ------------------------------------------------------------------------------------------------------------

def gemm_dispatch(M, N, K, bf16, split=True):
    """(BM, BN, split-K slices) of one decoder-side GEMM."""
    if M < 2048 and (N // 64) * ((M + 31) // 32) < 256 and N % 32 == 0:
        BM, BN = 32, 32
    elif M < 2048:
        BM, BN = 32, 64
    elif M < 8192:
        BM, BN = 64, 64
    else:
        BM, BN = 128, 64
    n = 1
    if bf16 and split:
        BKE, target, max_split = 64, 512, 4
        tiles = (N // BN) * ((M + BM - 1) // BM)
        while n * 2 <= max_split and tiles * n * 2 <= target and (K // BKE) % (n * 2) == 0 and K // (n * 2) >= 2 * BKE:
            n *= 2
        if tiles > 2048 or tiles * n * BM * BN > 512 * 32 * 64:
            n = 1
    return BM, BN, n


def decode_dispatch(B, T, P, bf16=True, split=True, D=384, De=192, Fd=1536, k0=3, nq=6, head_n=1088):
    """{GEMM: (M, BM, BN, slices)} of one decode: the shared stack runs on B*T rows, the six decoders on B*(P+T),
    the head on B*nq*T."""
    out = {}

    def add(name, M, N, K):
        out[name] = (M,) + gemm_dispatch(M, N, K, bf16, split)
    add("bridge", B * T, D, De)
    for stack, M in (("shared", B * T), ("dec", B * (P + T))):
        add(stack + ".qkv", M, 3 * D, D)
        add(stack + ".fc", M, D, D)
        add(stack + ".conv1", M, Fd, k0 * D)
        add(stack + ".conv2", M, D, Fd)
    add("head", B * nq * T, head_n, D)
    return out


# (B, T, P) on both sides of every switch above (the table in tests/test_prior_profile_gpu.py's docstring)
DISPATCH_SHAPES = [(1, 37, 123), (1, 38, 123), (2, 40, 72), (1, 81, 144), (2, 96, 64), (3, 50, 57), (4, 60, 52),
                   (1, 300, 149), (3, 150, 74), (1, 400, 273), (4, 200, 136), (5, 180, 89), (23, 60, 29), (8, 180, 76)]


def max_slices(B, T, P):
    return max(v[3] for v in decode_dispatch(B, T, P).values())


# ------------------------------------------------------------------------------------------------------------
# references and floors, computed once per input and shared by the tests of one run
# ------------------------------------------------------------------------------------------------------------
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def encode_refs(sd, sd64, ids, mask):
    """(fp64 oracle, fp32 oracle) encoder outputs."""
    with torch.inference_mode():
        return orc.prior_encoder(sd64, ids, mask), orc.prior_encoder(sd, ids, mask)


def decode_refs(sd, sd64, x, tgt, prompts, bf16=True):
    """{"ref": fp64 oracle (embs, logits), "f32": fp32 oracle, "bf16": bf16 emulation} of one decode."""
    with torch.inference_mode():
        r = {"ref": orc.prior_decode(sd64, x.double(), tgt, prompts)[:2], "f32": orc.prior_decode(sd, x, tgt, prompts)[:2]}
        if bf16:
            r["bf16"] = emulated_decode(sd, x, tgt, prompts)[:2]
    return r


# ------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------

def row_profile(out, ref, floor_out, valid=None):
    """(row max of out, row max of the floor, argmax (utterance, row), row_errors(out, ref))."""
    n = ref.shape[1]
    e = row_errors(out, ref, valid)
    f = row_errors(floor_out, ref, valid)
    r = int(torch.argmax(e))
    return float(e.max()), float(f.max()), (r // n, r % n), e


def bar_of(fmax, mode):
    """The row bar of a mode from the floor's worst row."""
    if mode == "bf16":
        return FACTOR_BF16 * fmax
    assert mode == "f32", mode
    return min(FACTOR_F32 * fmax, F32_ROW_BAR)


def assert_row_profile(out, ref, floor_out, label, mode, valid=None):
    """No unpadded row of `out` may stand further from `ref` than factor x the worst row of the mode's floor (f32:
    and never further than F32_ROW_BAR)."""
    assert torch.isfinite(torch.as_tensor(out)).all(), f"{label}: non-finite output"
    emax, fmax, (u, t), e = row_profile(out, ref, floor_out, valid)
    bar = bar_of(fmax, mode)
    v = e[e > 0]
    med = float(v.median()) if v.numel() else 0.0
    print(f"xfmr profile {label} [{mode}]: row max {emax:.3e}, floor row max {fmax:.3e}, ratio {emax / fmax:.2f}, "
          f"argmax (utterance {u}, row {t}), median {med:.3e}, bar {bar:.3e}")
    assert emax <= bar, (f"{label}: row {t} of utterance {u} is {emax:.3e} from the fp64 oracle, {emax / fmax:.2f}x the "
                         f"{mode} floor's worst row {fmax:.3e} (bar {bar:.3e})")
    return emax / fmax
