"""CPU calibration of the prior stack's per-row error profile (tests/_xfmrprofile.py).

  * the emulation with round = identity is the pinned oracle, bitwise, block, encoder and decode;
  * the fp32 floor (fp32 oracle against fp64 oracle) is a property of the arithmetic: a second seed stays in range;
  * two realizations of the bf16 floor (a second input seed; fp64 instead of fp32 GEMM accumulation) agree within
    FACTOR_BF16 / 1.5;
  * ten planted single-site bugs, on one FFT block / the one-block-per-stack configuration and on the full
    configuration, each stand above the bar of their mode (GEMM-side bugs on one block: >= 1.5 x the bar), at a small
    shape and at a batch-sized one -- where most of them pass the global rel-L2 bars the GPU tests used alone.
The printed tables are the ones recorded in tests/_xfmrprofile.py's docstring.
"""
import pytest
import torch

from _common import orc, rel_l2
import _xfmrprofile as xp
from _xfmrprofile import (bf16_round, emulated_decode, emulated_encoder, emulated_fft_block, row_errors, to64)

DEC_BLOCK = "prior_generator.prior_decoder.0.layer_stack.0"
ENC_BLOCK = "prior_generator.encoder.layer_stack.0"
OLD_BAR = {("f32", "dec"): 1e-4, ("f32", "enc"): 2e-5, ("bf16", "dec"): 1e-2}  # tests/test_prior_gpu.py


@pytest.fixture(scope="module")
def reduced():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    _, sd = xp.build_prior(reduced=True)
    return sd, to64(sd)


@pytest.fixture(scope="module")
def full():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    _, sd = xp.build_prior()
    return sd, to64(sd)


def _block_inputs(seed, lens, D):
    g = torch.Generator().manual_seed(seed)
    B, n = len(lens), max(lens)
    return torch.randn(B, n, D, generator=g), orc.mask_from_lengths(torch.tensor(lens), n)


def _decode_inputs(seed, T, P, tl):
    g = torch.Generator().manual_seed(seed)
    B = len(tl)
    tgt = torch.tensor(tl)
    x = torch.randn(B, T, 192, generator=g).masked_fill(orc.mask_from_lengths(tgt, T).unsqueeze(-1), 0)
    return x, tgt, torch.randint(0, 1025, (B, 6, P), generator=g)


def test_row_errors_definition():
    ref = torch.zeros(2, 3, 4)
    ref[..., 0] = 2.0                     # every row norm 2 -> global RMS row norm 2
    ref[1, 2, 0] = 200.0                  # a padded row does not enter the RMS ...
    out = ref.clone()
    out[1, 1, 1] = 1.0
    out[1, 2, 2] = 7.0                    # ... nor the errors
    valid = torch.tensor([[True, True, True], [True, True, False]])
    e = row_errors(out, ref, valid)
    assert e.dtype == torch.float64 and e.shape == (6,)
    assert torch.equal(e, torch.tensor([0, 0, 0, 0, 0.5, 0], dtype=torch.float64))


def test_identity_emulation_is_the_oracle(reduced, full):
    for sd, _ in (reduced, full):
        x, mask = _block_inputs(1, [70, 33], 384)
        seen = []
        out = emulated_fft_block(sd, DEC_BLOCK, x, mask, 12, round=None,
                                 mutate=lambda s, v, ctx: (seen.append(s), v)[1])
        assert torch.equal(out, orc.fft_block(sd, DEC_BLOCK, x, mask, 12))
        assert seen == ["att", "conv1", "conv2"]
        ids = torch.randint(1, 361, (2, 70), generator=torch.Generator().manual_seed(2))
        assert torch.equal(emulated_encoder(sd, ids, mask), orc.prior_encoder(sd, ids, mask))
        xl, tgt, prompts = _decode_inputs(3, 24, 9, [24, 13])
        for a, b in zip(emulated_decode(sd, xl, tgt, prompts, round=None, mutate=lambda s, v, ctx: v),
                        orc.prior_decode(sd, xl, tgt, prompts)):
            assert torch.equal(a, b)


def test_identity_emulation_rebuilds_the_position_table():
    _, sd = xp.build_prior(reduced=True, dec_max_seq=48)
    assert sd["prior_generator.shared_decoder.position_enc"].shape[1] == 49
    xl, tgt, prompts = _decode_inputs(4, 49, 21, [49, 30])
    for a, b in zip(emulated_decode(sd, xl, tgt, prompts, round=None), orc.prior_decode(sd, xl, tgt, prompts)):
        assert torch.equal(a, b)


def test_dispatch_shapes_straddle_the_switches():
    """The dispatch table of tests/test_prior_profile_gpu.py's docstring against gemm_dispatch (csrc restated)."""
    d = {s: xp.decode_dispatch(*s) for s in xp.DISPATCH_SHAPES}
    M = [v["dec.qkv"][0] for v in d.values()]
    assert M == [160, 161, 224, 225, 320, 321, 448, 449, 672, 673, 1344, 1345, 2047, 2048]
    col = lambda name: [v[name][1:] for v in d.values()]  # noqa: E731
    assert col("dec.conv1") == [(32, 32, 2)] + [(32, 32, 1)] * 4 + [(32, 64, 1)] * 8 + [(64, 64, 1)]
    assert col("dec.qkv") == [(32, 32, 2)] * 3 + [(32, 32, 1)] * 4 + [(32, 64, 1)] * 6 + [(64, 64, 1)]
    assert col("dec.conv2") == [(32, 32, 4)] * 5 + [(32, 32, 2)] * 4 + [(32, 32, 1)] * 2 + [(32, 64, 1)] * 2 + [(64, 64, 1)]
    assert col("dec.fc") == [(32, 32, 2)] * 9 + [(32, 32, 1)] * 2 + [(32, 64, 1)] * 2 + [(64, 64, 1)]
    assert [v["head"] for v in list(d.values())[:4]] == [(222, 32, 32, 2), (228, 32, 32, 1), (480, 32, 32, 1),
                                                         (486, 32, 64, 1)]
    assert [v["head"][1:3] for v in list(d.values())[4:]] == [(32, 64)] * 4 + [(64, 64)] * 4 + [(128, 64)] * 2
    assert d[(1, 400, 273)]["shared.conv2"][1:] == (32, 32, 2)
    assert all(v["bridge"][3] == 1 for v in d.values())
    # fp32: the same tiles, never split
    assert xp.gemm_dispatch(320, 384, 1536, False) == (32, 32, 1) and xp.gemm_dispatch(1345, 384, 1536, False) == (32, 64, 1)


# ------------------------------------------------------------------------------------------------------------
# floors
# ------------------------------------------------------------------------------------------------------------
F32_FLOOR_RANGE = (1.5e-7, 8e-7)  # row max of fp32 oracle against fp64 oracle; measured 2.6-5.4e-7 over 65-129 rows


def _f32_floor_cases(reduced, full, seed):
    sd, sd64 = reduced
    fsd, fsd64 = full
    with torch.inference_mode():
        x, mask = _block_inputs(seed, [129, 64, 1], 384)
        yield "decoder block [129, 64, 1]", orc.fft_block(sd, DEC_BLOCK, x, mask, 12), \
            orc.fft_block(sd64, DEC_BLOCK, x.double(), mask, 12), ~mask
        x, mask = _block_inputs(seed + 1, [65, 17], 192)
        yield "encoder block [65, 17]", orc.fft_block(sd, ENC_BLOCK, x, mask, 4), \
            orc.fft_block(sd64, ENC_BLOCK, x.double(), mask, 4), ~mask
        ids = torch.randint(1, 361, (2, 97), generator=torch.Generator().manual_seed(seed))
        mask = orc.mask_from_lengths(torch.tensor([97, 60]), 97)
        yield "full encoder [97, 60]", orc.prior_encoder(fsd, ids, mask), orc.prior_encoder(fsd64, ids, mask), ~mask
        xl, tgt, prompts = _decode_inputs(seed, 40, 25, [40, 29])
        valid = (~orc.mask_from_lengths(tgt, 40)).unsqueeze(1).expand(-1, 6, -1).reshape(2, -1)
        a, b = orc.prior_decode(fsd, xl, tgt, prompts), orc.prior_decode(fsd64, xl.double(), tgt, prompts)
        yield "full decode (2, 40, 25) embs", xp.emb_rows(a[0]), xp.emb_rows(b[0]), valid
        yield "full decode (2, 40, 25) logits", xp.logit_rows(a[1]), xp.logit_rows(b[1]), valid


@pytest.mark.parametrize("seed", [11, 12])
def test_f32_floor_is_a_property_of_the_arithmetic(reduced, full, seed):
    for label, o32, o64, valid in _f32_floor_cases(reduced, full, seed):
        e = row_errors(o32, o64, valid)
        v = e[valid.reshape(-1)]
        print(f"f32 floor seed {seed} {label}: row max {float(v.max()):.2e}, median {float(v.median()):.2e}, "
              f"max / median {float(v.max() / v.median()):.2f}")
        assert F32_FLOOR_RANGE[0] <= float(v.max()) <= F32_FLOOR_RANGE[1], label
        assert xp.F32_ROW_BAR >= 10 * float(v.max())


def _bf16_floor(sd, sd64, T, P, tl, seed, acc64=False):
    xl, tgt, prompts = _decode_inputs(seed, T, P, tl)
    B = len(tl)
    valid = (~orc.mask_from_lengths(tgt, T)).unsqueeze(1).expand(-1, 6, -1).reshape(B, -1)
    with torch.inference_mode():
        ref = orc.prior_decode(sd64, xl.double(), tgt, prompts)
        emu = emulated_decode(sd, xl, tgt, prompts, acc64=acc64)
    return (float(row_errors(xp.emb_rows(emu[0]), xp.emb_rows(ref[0]), valid).max()),
            float(row_errors(xp.logit_rows(emu[1]), xp.logit_rows(ref[1]), valid).max()))


@pytest.mark.parametrize("cfg,T,P,tl", [("reduced", 12, 20, [12, 1]), ("reduced", 65, 64, [65]),
                                        ("reduced", 100, 221, [100, 77]), ("full", 28, 20, [28, 28, 9]),
                                        ("full", 96, 16, [96, 61]), ("full", 140, 84, [140, 90, 33])])
def test_bf16_floor_spread(reduced, full, cfg, T, P, tl):
    """Two more realizations of the bf16 floor at shapes the GPU tests use: FACTOR_BF16 >= 1.5 x their worst ratio."""
    sd, sd64 = reduced if cfg == "reduced" else full
    base = _bf16_floor(sd, sd64, T, P, tl, 3)
    seed2 = _bf16_floor(sd, sd64, T, P, tl, 4)
    acc = _bf16_floor(sd, sd64, T, P, tl, 3, acc64=True)
    for what, i in (("embs", 0), ("logits", 1)):
        rs, ra = seed2[i] / base[i], acc[i] / base[i]
        print(f"bf16 floor {cfg} ({len(tl)}, {T}, {P}) {what}: row max {base[i]:.2e}; second seed x{rs:.2f}, "
              f"fp64 accumulation x{ra:.2f}")
        for r in (rs, ra):
            assert 1.5 * max(r, 1 / r) <= xp.FACTOR_BF16, (what, r)


# ------------------------------------------------------------------------------------------------------------
# planted bugs
# ------------------------------------------------------------------------------------------------------------

def _at(site, fn):
    def mutate(s, v, ctx):
        if s != site:
            return v
        v = v.clone()
        r = fn(v, ctx)
        return v if r is None else r
    return mutate


def _ninf(v, rows, q, k):
    v[rows, q, k] = float("-inf")


def _head_rows(ctx, b, heads=None):
    hs = range(ctx["n_head"]) if heads is None else heads
    return [h * ctx["B"] + b for h in hs]


def _attention_bugs(n, len1):
    """(a)-(d) on the logits of one block; utterance 0 is full length, utterance 1 has len1 < n rows."""
    def a(v, c):
        for r in _head_rows(c, 0):
            v[r, 70, 63] = float("-inf")

    def b(v, c):
        v[_head_rows(c, 0, [1])[0], 70, n - 1] = float("-inf")

    def cc(v, c):
        for r in _head_rows(c, 0):
            v[r, 32:64, n - 1] = float("-inf")

    def d(v, c):
        for r in _head_rows(c, 1):
            v[r, :, len1] = c["raw"][r, :, len1]
    return [("(a) query 70 loses key 63 (end of chunk 0), all heads", _at("att", a)),
            ("(b) query 70 loses key n-1 in head 1", _at("att", b)),
            ("(c) queries 32..63 lose key n-1, all heads", _at("att", cc)),
            ("(d) first padded key of utterance 1 attended", _at("att", d))]


def _gemm_bugs(n, k0, leak_tap):
    """(e), (f), (i) on one block's conv GEMMs (k0 taps in conv1); utterance 0 is full length."""
    def e(v, c):
        v[1, :, 0] += c["w"][:, :, k0 // 2 + leak_tap] @ c["x"][0, :, n + leak_tap]

    def f(v, c):
        v[0, :, n - 1] -= c["w"][:, :, k0 // 2 - 1] @ c["x"][0, :, n - 2]

    def i(v, c):
        K = c["x"].shape[1]
        v[0, 64:96, 32:64] -= c["w"][64:96, K // 2:, 0] @ c["x"][0, K // 2:, 32:64]
    return [(f"(e) frame 0 of utterance 1 reads utterance 0 through tap {leak_tap} only", _at("conv1", e)),
            ("(f) last row of utterance 0 loses tap -1", _at("conv1", f)),
            ("(i) conv2 drops the upper K/2 slice on rows 32..63 x columns 64..95", _at("conv2", i))]


def _decode_bugs():
    def g(v, c):
        if c["q"] == 3:
            v[:, c["P"]] += (c["prompt_emb"] - c["target_emb"])[0, 0]

    def h(v, c):
        if c["q"] == 5:
            return c["full"][:, c["P"] - 1:-1]

    def j(v, c):
        v[..., 1024] = 0.0
    return [("(g) decoder 3's input row P gets prompt_emb", _at("dec_in", g), "embs"),
            ("(h) decoder 5's target slice shifted by one row", _at("slice", h), "embs"),
            ("(j) head column 1024 from the zero padding", _at("head", j), "logits")]


def _report(rows, title):
    print(f"\n{title}")
    print(f"  {'case':<76} {'mode':<5} {'row max':>9} {'x floor':>8} {'x bar':>6}  global rel-L2 (old bar)")
    for label, mode, emax, fmax, bar, glob, old in rows:
        verdict = "passed" if glob < old else "failed"
        print(f"  {label:<76} {mode:<5} {emax:9.2e} {emax / fmax:8.1f} {emax / bar:6.1f}  {glob:.2e} ({old:g}: {verdict})")


def _block_table(sd, sd64, p, n_head, D, lens, bugs, modes, kind):
    """Run every bug of `bugs` on one block in every mode of `modes`; rows of the table + the asserts."""
    x, mask = _block_inputs(7, lens, D)
    valid = ~mask
    rows = []
    with torch.inference_mode():
        ref = orc.fft_block(sd64, p, x.double(), mask, n_head)
        for mode in modes:
            rnd = bf16_round if mode == "bf16" else None
            floor = emulated_fft_block(sd, p, x, mask, n_head, round=rnd)
            fmax = float(row_errors(floor, ref, valid).max())
            bar = xp.bar_of(fmax, mode)
            rows.append((f"floor: one {kind} block, lens {lens[:3]}{'...' if len(lens) > 3 else ''}", mode, fmax, fmax, bar,
                         rel_l2(floor[valid], ref[valid]), OLD_BAR[(mode, kind)]))
            for label, mut in bugs:
                out = emulated_fft_block(sd, p, x, mask, n_head, round=rnd, mutate=mut)
                emax = float(row_errors(out, ref, valid).max())
                rows.append((label, mode, emax, fmax, bar, rel_l2(out[valid], ref[valid]), OLD_BAR[(mode, kind)]))
    return rows


def _check(rows, margin):
    for label, mode, emax, fmax, bar, _, _ in rows:
        if not label.startswith("floor"):
            assert emax >= margin * bar, f"{label} [{mode}]: row max {emax:.3e} under {margin} x the bar {bar:.3e}"


SMALL = [129, 100]
BATCH = [580, 571, 540, 500, 433, 377, 290, 64]


@pytest.mark.parametrize("lens", [SMALL, BATCH], ids=["small", "batch"])
def test_planted_attention_bugs(reduced, lens):
    """(a)-(d): attention stays fp32 in both modes, so its bugs are judged against the f32 bar -- which must stay
    below half the weakest of them."""
    sd, sd64 = reduced
    n = max(lens)
    rows = _block_table(sd, sd64, DEC_BLOCK, 12, 384, lens, _attention_bugs(n, lens[1]), ["f32"], "dec")
    rows += _block_table(sd, sd64, ENC_BLOCK, 4, 192, lens, _attention_bugs(n, lens[1]), ["f32"], "enc")
    _report(rows, f"attention bugs, one block, {len(lens)} x {n} rows")
    _check(rows, 2.0)


@pytest.mark.parametrize("lens", [SMALL, BATCH], ids=["small", "batch"])
def test_planted_gemm_bugs_one_block(reduced, lens):
    """(e), (f), (i) on one decoder block in both modes (>= 1.5 x the bar) and on one encoder block (fp32)."""
    sd, sd64 = reduced
    n = max(lens)
    rows = _block_table(sd, sd64, DEC_BLOCK, 12, 384, lens, _gemm_bugs(n, 3, -1), ["f32", "bf16"], "dec")
    rows += _block_table(sd, sd64, ENC_BLOCK, 4, 192, lens, _gemm_bugs(n, 9, -4), ["f32"], "enc")
    _report(rows, f"GEMM-side bugs, one block, {len(lens)} x {n} rows")
    _check(rows, 1.5)


def _decode_table(sd, sd64, T, P, tl, bugs, title):
    xl, tgt, prompts = _decode_inputs(8, T, P, tl)
    B = len(tl)
    valid = (~orc.mask_from_lengths(tgt, T)).unsqueeze(1).expand(-1, 6, -1).reshape(B, -1)
    pick = {"embs": lambda r: xp.emb_rows(r[0]), "logits": lambda r: xp.logit_rows(r[1])}
    rows = []
    with torch.inference_mode():
        ref = orc.prior_decode(sd64, xl.double(), tgt, prompts)
        for mode in ("f32", "bf16"):
            rnd = bf16_round if mode == "bf16" else None
            floor = emulated_decode(sd, xl, tgt, prompts, round=rnd)
            fm = {k: float(row_errors(f(floor), f(ref), valid).max()) for k, f in pick.items()}
            for k in pick:
                rows.append((f"floor: decode ({B}, {T}, {P}) {k}", mode, fm[k], fm[k], xp.bar_of(fm[k], mode),
                             rel_l2(pick[k](floor), pick[k](ref)), OLD_BAR[(mode, "dec")]))
            for label, mut, k in bugs:
                out = emulated_decode(sd, xl, tgt, prompts, round=rnd, mutate=mut)
                emax = float(row_errors(pick[k](out), pick[k](ref), valid).max())
                rows.append((f"{label} [{k}]", mode, emax, fm[k], xp.bar_of(fm[k], mode),
                             rel_l2(pick[k](out), pick[k](ref)), OLD_BAR[(mode, "dec")]))
    _report(rows, title)
    return rows


def _stack_bugs(n):
    """(e), (f), (i) in the first block of the shared decoder only (n = T rows per utterance: with a prompt the leak
    of (e) lands on a prompt row, which a one-block decoder never shows in its target slice)."""
    def only(mut):
        return lambda s, v, c: mut(s, v, c) if c.get("p", "").endswith("shared_decoder.layer_stack.0") else v
    return [(lab + ", shared decoder", only(m), "embs") for lab, m in _gemm_bugs(n, 3, -1)]


@pytest.mark.parametrize("T,P,tl", [(40, 25, [40, 29]), (420, 160, [420, 400, 377, 350, 301, 256, 199, 64])],
                         ids=["small", "batch"])
def test_planted_decode_bugs_one_block_per_stack(reduced, T, P, tl):
    """(g), (h), (j) and (e), (f), (i) inside the shared decoder, one block per stack: >= 1.5 x the bar in both modes."""
    sd, sd64 = reduced
    bugs = _decode_bugs() + (_stack_bugs(T) if len(tl) == 2 else [])  # (e), (f), (i) at batch size: the one-block test
    rows = _decode_table(sd, sd64, T, P, tl, bugs, f"decode bugs, one block per stack, ({len(tl)}, {T}, {P})")
    _check(rows, 1.5)


def test_planted_decode_bugs_full_stack(full):
    """The same on the full configuration (later attention layers smear a localized bug): above the bar."""
    sd, sd64 = full
    T, P, tl = 40, 25, [40, 29]
    rows = _decode_table(sd, sd64, T, P, tl, _decode_bugs() + _stack_bugs(T), f"decode bugs, full stack, (2, {T}, {P})")
    _check(rows, 1.0)
