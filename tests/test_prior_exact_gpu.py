"""GPU: exact lengths in the prior stage -- the persistent PVA flow's exact-lengths instantiation and the graph path
(flamed_pva_flow_exact), the exact length regulator (flamed_lr_lengths_exact), the prior decode with per-utterance
prompt lengths (flamed_prior_decode_lens) and Flamed.sample_batch(exact_prior=True).  The reference of every check is
the oracle run on every utterance ALONE (tests/_priorexact.py: the definition and the bars)."""
import os
import warnings

import numpy as np
import pytest
import torch

from _common import golden, orc, rel_l2, t32
import _priorexact as px
import _xfmrprofile as xp
from test_prior_profile_gpu import _check_decode, _decode_inputs, _model
from test_pva_gpu import pva  # noqa: F401  (fixture: the seeded PVA on the GPU and its oracle state dict)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 1024


def _tune(**knobs):
    from flamed import _native as nat
    for k, v in knobs.items():
        nat.check(nat.lib().flamed_tune(k.encode(), int(v)), "flamed_tune")


# ------------------------------------------------------------------------------------------------------------
# PVA exact flow
# ------------------------------------------------------------------------------------------------------------
# (B, L, lengths, nfe): an end inside a 16-row tile; ends on and one before tile edges and a one-phoneme utterance;
# the default step count on one-tile groups; 10 tiles in two-tile groups (staged windows); seven-tile groups with an
# end in the middle of a four-tile pass
PVA_CASES = [(3, 13, [13, 7, 2], 8), (4, 16, [16, 15, 1, 9], 6), (3, 41, [41, 30, 11], 64), (4, 40, [40, 23, 17, 1], 6),
             (2, 247, [247, 100], 16)]
PVA_BIG = (3, 230, [230, 129, 64], 4)  # B L > 640: the graph path
NOISE_SEED = 7
# encoder-output seeds for which the oracle ALONE has no duration within 1e-3 of a .5 rounding boundary (picked on the CPU)
ENC_SEED = {(3, 13): 301, (4, 16): 300, (3, 41): 300, (4, 40): 300, (2, 247): 302, (3, 230): 302}


def pva_inputs(B, L, lens, nfe):
    """(enc, dn, sn): the encoder output and the two draws PVA.flow makes after torch.manual_seed(NOISE_SEED)."""
    enc = torch.randn(B, L, 192, generator=torch.Generator().manual_seed(ENC_SEED[(B, L)]))
    torch.manual_seed(NOISE_SEED)
    return enc, torch.randn((B, L)), torch.randn((B, L))


_FLOW_REF = {}


def _flow_ref(sd, B, L, lens, nfe):
    key = (B, L, tuple(lens), nfe)
    if key not in _FLOW_REF:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        enc, dn, sn = pva_inputs(B, L, lens, nfe)
        _FLOW_REF[key] = px.flow_alone(sd, enc, lens, dn, sn, nfe, 0.3)
    return _FLOW_REF[key]


def _check_flow(d, s, ref, lens, what):
    near = flips = 0
    for u, n in enumerate(lens):
        for name, got, r in (("dur", d[u], ref[u][0]), ("sil", s[u], ref[u][1])):
            assert torch.isfinite(got).all(), what
            assert torch.count_nonzero(got[n:]) == 0, f"{what}: utterance {u} {name}: rows behind its end are not 0"
            e = rel_l2(got[:n], r)
            print(f"{what}: utterance {u} (len {n}) {name} vs the oracle alone rel-L2 {e:.3e}")
            assert e <= px.DUR_BAR, (what, u, name, e)
            a, b = px.near_and_flips(got[:n], r)
            near, flips = near + a, flips + b
    assert near <= 1, f"{what}: {near} positions within 1e-4 of a .5 boundary (at most one may be excused)"
    assert flips == 0, f"{what}: {flips} integer-frame flips"


def _exact_flow(m, B, L, lens, nfe):
    enc, _, _ = pva_inputs(B, L, lens, nfe)
    mask = orc.mask_from_lengths(torch.tensor(lens), L)
    hp = m.hip()
    r0 = hp.persist_status()[0]
    with torch.inference_mode():
        torch.manual_seed(NOISE_SEED)
        d, s = m.flow(enc.to(DEV), mask.to(DEV), nfe, 0.3, exact=True)
    torch.cuda.synchronize()
    runs, fails = hp.persist_status()
    return d.cpu(), s.cpu(), runs - r0, fails


@pytest.mark.parametrize("B,L,lens,nfe", PVA_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_pva_exact_persistent(pva, B, L, lens, nfe):
    """One persistent launch (B L <= 640), every utterance against the oracle alone, 0 behind every end, bitwise
    deterministic."""
    m, sd = pva
    d, s, ran, fails = _exact_flow(m, B, L, lens, nfe)
    assert ran == 1 and fails == 0, (ran, fails)
    _check_flow(d, s, _flow_ref(sd, B, L, lens, nfe), lens, f"exact persistent flow ({B}, {L})")
    d2, s2, _, _ = _exact_flow(m, B, L, lens, nfe)
    assert torch.equal(d, d2) and torch.equal(s, s2)


@pytest.mark.parametrize("B,L,lens,nfe", [PVA_CASES[0], PVA_CASES[-1], PVA_BIG], ids=lambda v: str(v).replace(" ", ""))
def test_pva_exact_graph_path(pva, B, L, lens, nfe):
    """The graph of launches: persistent flow switched off, and a batch above 640 rows with it on."""
    m, sd = pva
    big = B * L > 640
    try:
        if not big:
            _tune(pva_persist=0)
        d, s, ran, _ = _exact_flow(m, B, L, lens, nfe)
    finally:
        _tune(pva_persist=1)
    assert ran == 0
    _check_flow(d, s, _flow_ref(sd, B, L, lens, nfe), lens, f"exact graph flow ({B}, {L})")


def _direct(hp, enc, d0, s0, nfe, lens=None, mask=None):
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    with torch.inference_mode():
        d, s = hp.flow(enc.to(DEV), None if mask is None else mask.to(DEV), d0.to(DEV), s0.to(DEV), ts, nfe, lens=lens)
    torch.cuda.synchronize()
    return d.cpu(), s.cpu()


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("B,L,lens,nfe", [PVA_CASES[0], PVA_CASES[3]], ids=lambda v: str(v).replace(" ", ""))
def test_pva_exact_padding_is_never_read(pva, B, L, lens, nfe, persist):
    """NaN in enc and in both states at every padded position: the valid outputs keep their bits."""
    m, _ = pva
    enc, dn, sn = pva_inputs(B, L, lens, nfe)
    pad = orc.mask_from_lengths(torch.tensor(lens), L)
    nan = float("nan")
    try:
        _tune(pva_persist=persist)
        clean = _direct(m.hip(), enc, dn * 0.3, sn * 0.3, nfe, lens)
        dirty = _direct(m.hip(), enc.masked_fill(pad.unsqueeze(-1), nan), (dn * 0.3).masked_fill(pad, nan),
                        (sn * 0.3).masked_fill(pad, nan), nfe, lens)
    finally:
        _tune(pva_persist=1)
    for a, b in zip(clean, dirty):
        assert torch.isfinite(b).all() and torch.equal(a, b)
        assert torch.count_nonzero(b[pad]) == 0


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("B,L,nfe", [(3, 13, 8), (4, 40, 6), (2, 247, 4)])
def test_pva_exact_all_lengths_equal_is_the_dense_flow(pva, B, L, nfe, persist):
    m, _ = pva
    enc, dn, sn = pva_inputs(B, L, [L] * B, nfe)
    try:
        _tune(pva_persist=persist)
        dense = _direct(m.hip(), enc, dn * 0.3, sn * 0.3, nfe, mask=torch.zeros(B, L, dtype=torch.bool))
        exact = _direct(m.hip(), enc, dn * 0.3, sn * 0.3, nfe, lens=[L] * B)
    finally:
        _tune(pva_persist=1)
    assert torch.equal(dense[0], exact[0]) and torch.equal(dense[1], exact[1])


def test_pva_exact_failure_rerun(pva):
    """pva_inject at step 3 of an exact flow: valid rows NaN, padded rows 0, counted; with the check on the wrapper
    warns and re-runs the flow EXACT on the graph path."""
    from flamed.models.synthesizer.pva import PvaHIP
    m, sd = pva
    hp = PvaHIP(m)  # a fresh pair: the module's own stays on the persistent path
    B, L, lens, nfe = PVA_CASES[0]
    enc, dn, sn = pva_inputs(B, L, lens, nfe)
    pad = orc.mask_from_lengths(torch.tensor(lens), L)
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    with torch.inference_mode():
        ref = hp._graph_flow(enc.to(DEV), None, (dn * 0.3).to(DEV), (sn * 0.3).to(DEV), ts, nfe, 1 | 2, lens)
        try:
            _tune(pva_inject=3)
            hp.check_persist = False
            raw = _direct(hp, enc, dn * 0.3, sn * 0.3, nfe, lens)
            for r in raw:
                assert torch.isnan(r[~pad]).all() and torch.count_nonzero(r[pad]) == 0
            assert hp.persist_status()[1] == 1
            hp.check_persist = True
            with warnings.catch_warnings(record=True) as wl:
                warnings.simplefilter("always")
                out = _direct(hp, enc, dn * 0.3, sn * 0.3, nfe, lens)
            assert any("persistent PVA flow failed" in str(w.message) for w in wl)
        finally:
            _tune(pva_inject=-1)
    assert torch.equal(out[0], ref[0].cpu()) and torch.equal(out[1], ref[1].cpu())
    _check_flow(out[0], out[1], _flow_ref(sd, B, L, lens, nfe), lens, "exact flow re-run on the graph path")


# ------------------------------------------------------------------------------------------------------------
# length regulator, exact
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,L,H,log", [(5, 37, 192, False), (7, 3, 8, False), (1, 1, 192, False), (3, 50, 16, True)])
def test_length_regulator_exact_bit_exact(B, L, H, log):
    from flamed.models.synthesizer.pva import hip_length_regulate
    rng = np.random.default_rng(B * 7919 + L)
    x = torch.from_numpy(rng.standard_normal((B, L, H)).astype(np.float32))
    if log:
        d = torch.from_numpy(rng.uniform(-1, 3, (B, L)).astype(np.float32))
        s = torch.from_numpy(rng.uniform(-1, 1.5, (B, L)).astype(np.float32))
    else:
        d = torch.from_numpy(rng.integers(0, 9, (B, L)).astype(np.float32))
        s = torch.from_numpy(rng.integers(0, 4, (B, L)).astype(np.float32))
    sl = [L] + [int(v) for v in rng.integers(1, L + 1, (B - 1,))]
    ref = px.lr_alone(x, list(d), list(s), sl, log_domain=log)
    out, tl = hip_length_regulate(x.to(DEV), d.to(DEV), s.to(DEV), torch.tensor(sl).to(DEV), None, log_domain=log,
                                  exact=True)
    out, tl = out.cpu(), tl.cpu()
    assert tl.tolist() == [t for _, t in ref]
    assert out.shape[1] == max(t for _, t in ref)
    for u, (xu, tu) in enumerate(ref):
        assert torch.equal(out[u, :tu], xu) and torch.count_nonzero(out[u, tu:]) == 0
    if B > 1 and min(sl) < L:  # the default regulator counts one frame per padded phoneme
        _, tl0 = hip_length_regulate(x.to(DEV), d.to(DEV), s.to(DEV), torch.tensor(sl).to(DEV), None, log_domain=log)
        assert tl0.cpu().tolist() == [t + (L - n) for (_, t), n in zip(ref, sl)]


# ------------------------------------------------------------------------------------------------------------
# prior decode with prompt lengths
# ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def red():
    return _model(reduced=True)


@pytest.fixture(scope="module")
def red48():
    return _model(reduced=True, dec_max_seq=48)


@pytest.fixture(scope="module")
def full():
    return _model()


def _alone_refs(m, x, tgt, prompts, plens, key):
    """{"ref": fp64 oracle, "f32": fp32 oracle, "bf16": bf16 emulation}, every utterance alone behind its own prompt."""
    _, sd, sd64 = m

    def make():
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        return {"ref": px.decode_alone(sd64, x.double(), tgt, prompts, plens),
                "f32": px.decode_alone(sd, x, tgt, prompts, plens),
                "bf16": px.decode_alone(sd, x, tgt, prompts, plens, fn=xp.emulated_decode)}
    return xp.memo(("alone",) + key, make)


def _hip_decode_lens(pg, x, mask, prompts, P, plens, mode):
    try:
        pg.hip_dec_dtype = mode
        with torch.inference_mode():
            pe, pl = pg.hip().decode(x.to(DEV), mask.to(DEV), prompts.to(DEV), P, prompt_lens=plens)
    finally:
        pg.hip_dec_dtype = "f32"
    return pe.cpu(), pl.cpu()


def _lens_case(m, tag, B, T, P, tl, plens, mode, profile=True):
    x, tgt, mask, prompts = _decode_inputs(3, B, T, P, tl)
    prompts = px.pad_prompts(prompts, plens, PAD)
    pe, pl = _hip_decode_lens(m[0], x, mask, prompts, P, plens, mode)
    refs = _alone_refs(m, x, tgt, prompts, plens, (tag, B, T, P, tuple(tl), tuple(plens)))
    label = f"{tag} decode ({B}, {T}, {P}) prompt lengths {plens}"
    if profile:
        _check_decode(pe, pl, refs, mask, mode, label)
    for u in range(B):
        ee, el = rel_l2(pe[u], refs["f32"][0][u]), rel_l2(pl[u], refs["f32"][1][u])
        print(f"{label} [{mode}] utterance {u}: vs the fp32 oracle alone embs {ee:.3e} logits {el:.3e}")
        assert ee <= px.DEC_BAR[mode] and el <= px.DEC_BAR[mode], (label, u, ee, el)
        assert torch.count_nonzero(pe[u, :, tl[u]:]) == 0 and torch.count_nonzero(pl[u, :, :, tl[u]:]) == 0
    return pe, pl


# (B, T, P, target lengths, prompt lengths): the issue's measured case; an utterance without a prompt; P_u on and off
# the 4-row LayerNorm block and the 32-row tile; a prompt 67 codes shorter than P (more than one 64-key chunk)
LENS_CASES = [(3, 24, 11, [24, 17, 9], [11, 6, 3]), (2, 40, 30, [40, 22], [30, 0]), (2, 33, 32, [33, 20], [32, 31]),
              (2, 80, 70, [80, 40], [70, 3])]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,P,tl,plens", LENS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_decode_prompt_lens_one_block(red, B, T, P, tl, plens, mode):
    _lens_case(red, "one-block", B, T, P, tl, plens, mode)


def test_decode_prompt_lens_fma_attention(red):
    try:
        _tune(attn_mfma=0)
        _lens_case(red, "one-block", *LENS_CASES[0], "f32")
    finally:
        _tune(attn_mfma=1)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_prompt_lens_position_override(red48, mode):
    """P + T above decoder_max_seq_len (48): the rebuilt table serves every utterance at its own positions."""
    _lens_case(red48, "maxseq48", 2, 40, 30, [40, 22], [30, 7], mode)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_prompt_lens_full_stack(full, mode):
    _lens_case(full, "full", 3, 50, 57, [50, 38, 26], [57, 20, 5], mode, profile=False)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_all_prompt_lens_equal_is_the_dense_decode(red, mode):
    B, T, P, tl = 2, 33, 31, [33, 20]
    x, tgt, mask, prompts = _decode_inputs(3, B, T, P, tl)
    pg = red[0]
    try:
        pg.hip_dec_dtype = mode
        with torch.inference_mode():
            a = pg.hip().decode(x.to(DEV), mask.to(DEV), prompts.to(DEV), P)
            b = pg.hip().decode(x.to(DEV), mask.to(DEV), prompts.to(DEV), P, prompt_lens=[P] * B)
    finally:
        pg.hip_dec_dtype = "f32"
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_decode_dense_after_lens_keeps_its_graph(red):
    """Dense and prompt-length decodes through one handle, alternating: each keeps its bits (separate graph caches)."""
    B, T, P, tl, plens = LENS_CASES[0]
    x, tgt, mask, prompts = _decode_inputs(3, B, T, P, tl)
    pg = red[0]
    with torch.inference_mode():
        outs = [pg.hip().decode(x.to(DEV), mask.to(DEV), prompts.to(DEV), P, prompt_lens=pl) for pl in (None, plens, None, plens)]
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[1][0], outs[3][0])
    assert not torch.equal(outs[0][0][1], outs[1][0][1])


def test_opcheck_new_ops(pva):
    """torch.library.opcheck (schema, fake tensors) on the three new ops; fresh owners, whose I/O buffers are not
    inference tensors."""
    from flamed.models.synthesizer.pva import PvaHIP
    utils = ("test_schema", "test_faketensor")
    m, _ = pva
    hp = PvaHIP(m)
    B, L, lens, nfe = PVA_CASES[0]
    enc, dn, sn = pva_inputs(B, L, lens, nfe)
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    torch.library.opcheck(torch.ops.flamed_hip.pva_flow_exact.default,
                          (hp.oid, enc.to(DEV), dn.to(DEV), sn.to(DEV), ts, nfe, lens), test_utils=utils)
    x = torch.randn(2, 5, 8, device=DEV)
    torch.library.opcheck(torch.ops.flamed_hip.length_regulate_exact.default,
                          (x, torch.tensor([[1., 2, 0, 3, 1], [2, 1, 1, 0, 0]], device=DEV),
                           torch.zeros(2, 5, device=DEV), torch.tensor([5, 3], device=DEV), 12, False), test_utils=utils)
    Bd, T, P, tl, plens = LENS_CASES[0]
    xd, _, mask, prompts = _decode_inputs(3, Bd, T, P, tl)
    pg = _model(reduced=True)[0]
    torch.library.opcheck(torch.ops.flamed_hip.prior_decode_lens.default,
                          (pg.hip().oid, xd.to(DEV), mask.to(DEV), prompts.to(DEV), P, plens), test_utils=utils)


# ------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------
E2E_SEED, E2E_NFE = 99, 4
E2E_PLENS = [20, 13, 6]


def e2e_inputs():
    g = golden("flamed_sample")
    gen = torch.Generator().manual_seed(17)
    ph, sl = t32(g["phonemes"]), t32(g["src_lens"])
    extra = torch.zeros(1, ph.shape[1], dtype=ph.dtype)
    extra[0, :5] = torch.randint(1, 300, (5,), generator=gen)
    phonemes = torch.cat([ph, extra])
    src = torch.cat([sl, torch.tensor([5])])
    pr = t32(g["prompts"])
    prompts = px.pad_prompts(torch.cat([pr, torch.randint(0, PAD, (1,) + tuple(pr.shape[1:]), generator=gen)]), E2E_PLENS, PAD)
    timbres = torch.cat([t32(g["timbres"]), torch.randn(1, 256, generator=gen)])
    return phonemes, src, prompts, timbres


def e2e_prior_alone(sd, phonemes, src, prompts):
    """The prior stage of every utterance alone by the oracle, from the draws sample_batch makes after
    torch.manual_seed(E2E_SEED) -> (tgt lengths, prior_embs (B, nq, T, D), near-boundary positions)."""
    B, L = phonemes.shape
    lens = src.tolist()
    torch.manual_seed(E2E_SEED)
    dn, sn = torch.randn((B, L)), torch.randn((B, L))
    with torch.inference_mode():
        enc = orc.prior_encoder(sd, phonemes, orc.mask_from_lengths(src, L))
    flow = px.flow_alone(sd, enc, lens, dn, sn, E2E_NFE, 0.3)
    near = sum(px.near_and_flips(r, r)[0] for f in flow for r in f)
    lr = px.lr_alone(enc, [f[0] for f in flow], [f[1] for f in flow], lens)
    tgt = torch.tensor([t for _, t in lr])
    x = torch.zeros(B, int(tgt.max()), enc.shape[-1])
    for u, (xu, tu) in enumerate(lr):
        x[u, :tu] = xu
    embs, _ = px.decode_alone(sd, x, tgt, prompts, E2E_PLENS)
    return tgt, embs, near


def test_sample_batch_exact_prior_end_to_end():
    """Flamed.sample_batch(exact_lengths=True, exact_prior=True) on a batch of three (the fixture's two lines and a
    shorter one, prompts of three lengths padded with the pad id): frame counts equal to, prior_embs within the bf16
    bar of, and latents within the solve bar of every utterance ALONE; zeros behind every end.  Without exact_prior the
    shortest utterance gets another frame count (one frame per padded phoneme at least)."""
    from _flamed_common import build_flamed
    from test_exact_lengths_cpu import alone_oracle
    from test_exact_lengths_gpu import _check_vs_oracle
    m, _ = build_flamed(DEV, "bf16")
    phonemes, src, prompts, timbres = e2e_inputs()
    kw = dict(phonemes=phonemes, src_lens=src, prompts=prompts, timbres=timbres, temp_durgen=0.3, temp_denoiser=0.3,
              nsteps_durgen=E2E_NFE, nsteps_denoiser=8)
    torch.manual_seed(E2E_SEED)
    out = m.sample_batch(exact_lengths=True, exact_prior=True, **kw)
    torch.manual_seed(E2E_SEED)
    off = m.sample_batch(exact_lengths=True, **kw)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = {"prior_generator." + k: v.detach().float().cpu() for k, v in m.prior_generator.state_dict().items()}
    tgt, embs, near = e2e_prior_alone(sd, phonemes, src, prompts)
    assert near <= 1
    got_t = (~out["tgt_mask"]).sum(-1).cpu()
    assert torch.equal(got_t, tgt), (got_t, tgt)
    assert int((~off["tgt_mask"]).sum(-1)[2]) != int(tgt[2])
    pe, lat = out["prior_embs"].cpu(), out["latents"].cpu()
    B, T = len(tgt), int(tgt.max())
    assert pe.shape[2] == T and lat.shape == (B, 256, T)
    for u in range(B):
        n = int(tgt[u])
        e = rel_l2(pe[u], embs[u])
        print(f"end to end utterance {u} ({n} frames): prior_embs vs the oracle alone rel-L2 {e:.3e}")
        assert e <= px.DEC_BAR["bf16"]
        assert torch.count_nonzero(pe[u, :, n:]) == 0 and torch.count_nonzero(lat[u, :, n:]) == 0
    # the solve, from the prior embeddings the GPU produced: the draw ProbGenerator.sample makes next
    torch.manual_seed(E2E_SEED)
    torch.randn((B, phonemes.shape[1])), torch.randn((B, phonemes.shape[1]))
    noise = torch.randn((B, T, 256))
    psd = {"prob_generator." + k: v.detach().float().cpu() for k, v in m.prob_generator.state_dict().items()}
    ref = alone_oracle(psd, pe, timbres, noise, tgt.tolist(), 8, 0.3)
    for u in range(B):
        n = int(tgt[u])
        _check_vs_oracle(lat[u, :, :n], ref[u, :, :n], n, f"end to end latents utterance {u} (len {n})")
