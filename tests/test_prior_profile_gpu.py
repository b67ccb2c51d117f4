"""Per-row error profiles of the prior transformer stack on the HIP library (tests/_xfmrprofile.py; calibration in
tests/test_xfmrprofile_cpu.py).  Reference: the fp64 oracle.  Floor: the fp32 oracle (hip_dec_dtype "f32", and the
encoder, which is always fp32) or the bf16 emulation ("bf16", the package default) against it.  No unpadded row of
prior_embs / the logits / the encoder output may stand above FACTOR x the floor's worst row; padded rows and masked
logits are exactly 0.

One-block-per-stack models (configs/prior.yaml with the layer counts reduced in memory) keep a localized error from
being smeared by later attention layers; their sweeps walk the attention kernels' edges (the 16 QW-query tile, the
64-key chunk, 1..6 and 10 chunks dealt to KG key groups, a fully padded chunk, groups without a chunk) with both
attention kernels, and the decoder-input seams (P on and off ln_mask_kernel's 4-row block and the 32-row GEMM tile).

Full-stack row counts sit on both sides of every dispatch switch of the decoder-side GEMMs (D = 384, F = 1536, k = 3;
_xfmrprofile.gemm_dispatch restates xf_gemm / pr_gemm / pick_cfg / choose_split; the shared stack runs on M = B T
rows, the six decoders on M = B (P + T), the head on 6 B T):

  GEMM (N, K)           32 x 32 tiles up to   above            bf16 split-K slices
  qkv   (1152,  384)    M <=  448             32 x 64          2: M <= 224
  fc    ( 384,  384)    M <= 1344             32 x 64          2: M <= 672
  conv1 (1536, 1152)    M <=  320             32 x 64          2: M <= 160
  conv2 ( 384, 1536)    M <= 1344             32 x 64          4: M <= 320, 2: M <= 672
  bridge( 384,  192)    M <= 1344             32 x 64          none (K / 64 is odd)
  head  (1088,  384)    M <=  480             32 x 64          2: M <= 224
  every GEMM: 64 x 64 tiles from M = 2048, 128 x 64 from M = 8192 (pick_cfg; only the head gets there)

  (B, T, P)       B T    B (P+T)  6 B T   what changes there
  (1, 37, 123)     37     160      222    conv1 splits (2); head 32 x 32 split 2
  (1, 38, 123)     38     161      228    conv1 no longer splits; head no longer splits
  (2, 40, 72)      80     224      480    qkv splits (2); head still 32 x 32
  (1, 81, 144)     81     225      486    qkv no longer splits; head 32 x 64
  (2, 96, 64)     192     320      1152   conv1 32 x 32, conv2 4 slices
  (3, 50, 57)     150     321      900    conv1 32 x 64, conv2 2 slices
  (4, 60, 52)     240     448      1440   qkv 32 x 32
  (1, 300, 149)   300     449      1800   qkv 32 x 64
  (3, 150, 74)    450     672      2700   fc / conv2 2 slices; head 64 x 64 (6 B T >= 2048)
  (1, 400, 273)   400     673      2400   decoders unsplit (the shared stack still splits)
  (4, 200, 136)   800     1344     4800   fc / conv2 32 x 32
  (5, 180, 89)    900     1345     5400   fc / conv2 32 x 64
  (23, 60, 29)    1380    2047     8280   32-row tiles; head 128 x 64 (6 B T >= 8192)
  (8, 180, 76)    1440    2048     8640   64 x 64 tiles in the decoders
tests/test_xfmrprofile_cpu.py checks this table against gemm_dispatch, and test_split_k_ab checks
gemm_dispatch's split prediction against the library (bitwise equal to the unsplit run exactly where it predicts no
split).

The timbre encoder (64-wide heads) exposes only the mean-pooled `spk`, not its frames: `spk` is checked at more
lengths with test_vq_timbre_vs_oracle's bar.
"""
import pytest
import torch

from _common import orc, rel_l2
import _xfmrprofile as xp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(**kw):
    pg, sd = xp.build_prior(**kw)
    return pg.to(DEV), sd, xp.to64(sd)


@pytest.fixture(scope="module")
def red():
    return _model(reduced=True)


@pytest.fixture(scope="module")
def full():
    return _model()


@pytest.fixture(scope="module")
def red48():
    return _model(reduced=True, dec_max_seq=48)


def _tune(**knobs):
    from flamed import _native as nat
    for k, v in knobs.items():
        nat.check(nat.lib().flamed_tune(k.encode(), int(v)), "flamed_tune")


def _tl(B, T):
    """Ragged target lengths: utterance 0 full, the others shorter."""
    return [max(1, T - (i * T) // (B + 1)) for i in range(B)]


def _decode_inputs(seed, B, T, P, tl):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.tensor(tl)
    mask = orc.mask_from_lengths(tgt, T)
    x = torch.randn(B, T, 192, generator=g).masked_fill(mask.unsqueeze(-1), 0)  # the length regulator zero-pads
    return x, tgt, mask, torch.randint(0, 1025, (B, 6, P), generator=g)


def _hip_decode(pg, x, mask, prompts, P, mode):
    try:
        pg.hip_dec_dtype = mode
        with torch.inference_mode():
            pe, pl = pg.hip().decode(x.to(DEV), mask.to(DEV), prompts.to(DEV), P)
    finally:
        pg.hip_dec_dtype = "f32"
    return pe.cpu(), pl.cpu()


def _refs(tag, m, x, tgt, prompts, seed):
    _, sd, sd64 = m
    B, T, _ = x.shape
    key = (tag, seed, B, T, prompts.shape[-1], tuple(tgt.tolist()))
    return xp.memo(key, lambda: xp.decode_refs(sd, sd64, x, tgt, prompts))


def _check_decode(pe, pl, refs, mask, mode, label):
    """Row profiles of prior_embs and the logits over the target rows; padded rows / masked logits exactly 0."""
    B, T = mask.shape
    valid = (~mask).unsqueeze(1).expand(-1, 6, -1).reshape(B, -1)
    (re, rl), (fe, fl) = refs["ref"], refs[mode]
    assert pe.shape == re.shape and pl.shape == rl.shape
    r1 = xp.assert_row_profile(xp.emb_rows(pe), xp.emb_rows(re), xp.emb_rows(fe), label + " embs", mode, valid)
    r2 = xp.assert_row_profile(xp.logit_rows(pl), xp.logit_rows(rl), xp.logit_rows(fl), label + " logits", mode, valid)
    assert torch.all(pl.permute(0, 2, 3, 1)[mask.unsqueeze(1).expand(-1, 6, -1)] == 0)
    assert torch.all(pe[mask.unsqueeze(1).expand(-1, 6, -1)] == 0)
    return r1, r2


def _decode_case(m, tag, B, T, P, tl, mode, seed=3, label=None):
    x, tgt, mask, prompts = _decode_inputs(seed, B, T, P, tl)
    pe, pl = _hip_decode(m[0], x, mask, prompts, P, mode)
    refs = _refs(tag, m, x, tgt, prompts, seed)
    _check_decode(pe, pl, refs, mask, mode, label or f"{tag} decode ({B}, {T}, {P})")
    return pe, pl, refs


# ------------------------------------------------------------------------------------------------------------
# one block per stack: the attention kernels' edges, both kernels
# ------------------------------------------------------------------------------------------------------------
ENC_LENS = [[129, 64, 1], [17, 16, 15], [65, 63], [128, 127], [257, 193, 65], [1], [16], [257]]


@pytest.mark.parametrize("attn_mfma", [1, 0])
@pytest.mark.parametrize("lens", ENC_LENS, ids=lambda v: "-".join(map(str, v)))
def test_encoder_one_block(red, lens, attn_mfma):
    """48-wide heads, key-padding mask, k = 9 conv gather; [129, 64, 1]: chunk 1 and 2 of the short utterances are
    all padding.  The encoder is fp32 in both decoder modes."""
    pg, sd, sd64 = red
    B, L = len(lens), max(lens)
    ids = torch.randint(1, 361, (B, L), generator=torch.Generator().manual_seed(1))
    mask = orc.mask_from_lengths(torch.tensor(lens), L)
    try:
        _tune(attn_mfma=attn_mfma)
        with torch.inference_mode():
            out = pg.hip().encode(ids.to(DEV), mask.to(DEV)).cpu()
    finally:
        _tune(attn_mfma=1)
    ref64, ref32 = xp.memo(("enc1", tuple(lens)), lambda: xp.encode_refs(sd, sd64, ids, mask))
    xp.assert_row_profile(out, ref64, ref32, f"one-block encoder {lens} attn_mfma={attn_mfma}", "f32", ~mask)
    assert torch.all(out[mask] == 0)


def test_encoder_full_stack(full):
    pg, sd, sd64 = full
    for lens in ([129, 64, 1], [250, 247, 200, 180, 150, 99, 64, 12]):
        B, L = len(lens), max(lens)
        ids = torch.randint(1, 361, (B, L), generator=torch.Generator().manual_seed(1))
        mask = orc.mask_from_lengths(torch.tensor(lens), L)
        with torch.inference_mode():
            out = pg.hip().encode(ids.to(DEV), mask.to(DEV)).cpu()
        ref64, ref32 = xp.encode_refs(sd, sd64, ids, mask)
        xp.assert_row_profile(out, ref64, ref32, f"full encoder {lens}", "f32", ~mask)
        assert rel_l2(out[~mask], ref32[~mask]) < 2e-5  # the global bar of tests/test_prior_gpu.py
        assert torch.all(out[mask] == 0)


# (B, T, P, tl): P + T in {1, 31, 32, 33, 64, 65, 128, 129, 193, 257, 321, 577}; P = 0 and P > T; utterances of
# length 1; P = 20 / 32 / 64 / 256 on a 4-row LayerNorm block, 31 / 33 / 57 / 129 / 221 off it; P = 32 / 64 on the
# 32-row GEMM tile, 31 / 33 beside it
DEC_EDGES = [(1, 1, 0, [1]), (2, 31, 0, [31, 1]), (2, 12, 20, [12, 7]), (3, 1, 32, [1, 1, 1]), (2, 33, 31, [33, 20]),
             (2, 32, 33, [32, 1]), (1, 128, 0, [128]), (2, 65, 64, [65, 40]), (2, 64, 129, [64, 33]),
             (1, 200, 57, [200]), (2, 100, 221, [100, 77]), (1, 321, 256, [321])]


@pytest.mark.parametrize("mode,attn_mfma", [("f32", 1), ("bf16", 1), ("f32", 0)])
@pytest.mark.parametrize("B,T,P,tl", DEC_EDGES, ids=lambda v: str(v).replace(" ", ""))
def test_decode_one_block(red, B, T, P, tl, mode, attn_mfma):
    try:
        _tune(attn_mfma=attn_mfma)
        _decode_case(red, "one-block", B, T, P, tl, mode, label=f"one-block decode ({B}, {T}, {P}) attn_mfma={attn_mfma}")
    finally:
        _tune(attn_mfma=1)


# ------------------------------------------------------------------------------------------------------------
# full stack: both sides of every dispatch switch
# ------------------------------------------------------------------------------------------------------------
DISPATCH = xp.DISPATCH_SHAPES


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,P", DISPATCH, ids=lambda v: str(v))
def test_decode_full_stack_dispatch(full, B, T, P, mode):
    pe, pl, refs = _decode_case(full, "full", B, T, P, _tl(B, T), mode)
    bar = 1e-4 if mode == "f32" else 1e-2  # the global bars of tests/test_prior_gpu.py, against the fp32 oracle
    assert rel_l2(pe, refs["f32"][0]) < bar and rel_l2(pl, refs["f32"][1]) < bar


# ------------------------------------------------------------------------------------------------------------
# split-K, graphs, handle reuse, batch isolation
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,P", [(2, 96, 20), (2, 200, 100), (5, 150, 20)], ids=lambda v: str(v))
def test_split_k_ab(full, B, T, P):
    """prior_split 1, 1, 0 in bf16 mode: deterministic, both inside the profile, and different bits exactly where
    choose_split splits ((2, 96, 20): up to 4 slices, (2, 200, 100): 2, (5, 150, 20): none)."""
    slices = xp.max_slices(B, T, P)
    assert slices == {(2, 96, 20): 4, (2, 200, 100): 2, (5, 150, 20): 1}[(B, T, P)]
    x, tgt, mask, prompts = _decode_inputs(5, B, T, P, _tl(B, T))
    refs = _refs("full", full, x, tgt, prompts, 5)
    outs = []
    try:
        for v in (1, 1, 0):
            _tune(prior_split=v)
            outs.append(_hip_decode(full[0], x, mask, prompts, P, "bf16"))
    finally:
        _tune(prior_split=1)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for (pe, pl), what in ((outs[0], "split on"), (outs[2], "split off")):
        _check_decode(pe, pl, refs, mask, "bf16", f"full decode ({B}, {T}, {P}) {what}")
    same = torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    assert same == (slices == 1), f"{slices} slices predicted, split on / off bitwise equal: {same}"


def test_graph_equals_eager_bf16_split(full):
    """The captured split-K graph against eager launches, also after tune changes that re-capture."""
    pg = full[0]
    B, T, P = 2, 80, 30
    x, tgt, mask, prompts = _decode_inputs(4, B, T, P, [80, 50])
    try:
        for attn_mfma in (1, 0, 1):
            _tune(attn_mfma=attn_mfma, prior_split=1)
            outs = []
            for graph in (True, False, True):
                pg.hip_graph = graph
                outs.append(_hip_decode(pg, x, mask, prompts, P, "bf16"))
            for o in outs[1:]:
                assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), f"attn_mfma={attn_mfma}"
    finally:
        pg.hip_graph = True
        _tune(attn_mfma=1, prior_split=1)
    assert xp.max_slices(B, T, P) == 4
    _check_decode(*outs[0], _refs("full", full, x, tgt, prompts, 4), mask, "bf16", "full decode (2, 80, 30) graph")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_shape_sequence_through_one_handle(full, mode):
    """(2, 96, 20) -> (1, 10, 0) -> encode -> (8, 80, 4) -> (2, 96, 20) through one handle: stale split counters,
    workspace rows past M or a stale dmask tail would change the bits against a fresh handle's."""
    pg = full[0]
    seq = [(2, 96, 20), (1, 10, 0), None, (8, 80, 4), (2, 96, 20)]
    ins = {s: _decode_inputs(6, s[0], s[1], s[2], _tl(s[0], s[1])) for s in seq if s}
    ids = torch.randint(1, 361, (3, 130), generator=torch.Generator().manual_seed(7)).to(DEV)
    smask = orc.mask_from_lengths(torch.tensor([130, 64, 9]), 130).to(DEV)

    def run(s):
        if s is None:
            with torch.inference_mode():
                return (pg.hip().encode(ids, smask).cpu(),)
        x, _, mask, prompts = ins[s]
        return _hip_decode(pg, x, mask, prompts, s[2], mode)

    outs = [run(s) for s in seq]
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[4]))
    for s, o in zip(seq[:4], outs[:4]):
        pg._hip = None  # a fresh handle (the previous one is destroyed with its PriorHIP)
        assert all(torch.equal(a, b) for a, b in zip(run(s), o)), f"{s}: differs from a fresh handle"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batch_isolation(full, mode):
    """Utterance u decoded alone at the same padded T against the same utterance inside the batch."""
    B, T, P, tl = 3, 64, 20, [64, 40, 17]
    x, tgt, mask, prompts = _decode_inputs(8, B, T, P, tl)
    pe, pl, refs = _decode_case(full, "full", B, T, P, tl, mode, seed=8)
    for u in range(B):
        se, sl = _hip_decode(full[0], x[u:u + 1], mask[u:u + 1], prompts[u:u + 1], P, mode)
        one = {k: (v[0][u:u + 1], v[1][u:u + 1]) for k, v in refs.items()}  # fp64 rows of u do not see the batch
        _check_decode(se, sl, one, mask[u:u + 1], mode, f"full decode utterance {u} of (3, 64, 20) alone")
        bitwise = torch.equal(se[0], pe[u]) and torch.equal(sl[0], pl[u])
        valid = (~mask[u:u + 1]).unsqueeze(1).expand(-1, 6, -1).reshape(1, -1)
        de = float(xp.row_errors(xp.emb_rows(se), xp.emb_rows(pe[u:u + 1]), valid).max())
        dl = float(xp.row_errors(xp.logit_rows(sl), xp.logit_rows(pl[u:u + 1]), valid).max())
        print(f"batch isolation [{mode}] utterance {u}: alone vs in batch row max embs {de:.3e} logits {dl:.3e}, "
              f"bitwise {bitwise}")
        if mode == "f32":
            fe = float(xp.row_errors(xp.emb_rows(one["f32"][0]), xp.emb_rows(one["ref"][0]), valid).max())
            fl = float(xp.row_errors(xp.logit_rows(one["f32"][1]), xp.logit_rows(one["ref"][1]), valid).max())
            assert de <= xp.bar_of(fe, "f32") and dl <= xp.bar_of(fl, "f32")


# ------------------------------------------------------------------------------------------------------------
# decoder position override, timbre encoder
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,T,P,tl", [(2, 40, 30, [40, 22]), (1, 49, 0, [49])], ids=lambda v: str(v).replace(" ", ""))
def test_decoder_position_override(red48, B, T, P, tl, mode):
    """P + T above decoder_max_seq_len (lowered to 48 in memory): the module passes a rebuilt sinusoid table, as the
    oracle rebuilds it (Models.py:150-155)."""
    assert P + T > red48[0].shared_decoder.max_seq_len == 48
    _decode_case(red48, "maxseq48", B, T, P, tl, mode)


@pytest.mark.parametrize("T", [16, 63, 64, 65, 129, 257])
def test_timbre_spk_lengths(T):
    """test_vq_timbre_vs_oracle's `spk` check (64-wide-head attention, no mask) at the chunk and tile edges."""
    from _flamed_common import build_flamed
    dec = xp.memo("facodec_dec", lambda: build_flamed(DEV, "f32")[1])
    sd = xp.memo("facodec_sd", lambda: {k: v.detach().cpu() for k, v in dec.state_dict().items()})
    x = torch.randn(2, 256, T, generator=torch.Generator().manual_seed(11))
    with torch.inference_mode():
        spk = dec(x.to(DEV), eval_vq=False, vq=True)[4].cpu()
        ref = orc.timbre_encoder(sd, x.transpose(1, 2)).transpose(1, 2).mean(dim=2)
    assert dec._vq_hip is not None and dec._vq_hip.handle is not None  # the HIP path ran
    e = rel_l2(spk, ref)
    print(f"timbre spk T={T}: rel-L2 {e:.3e}")
    assert e < 1e-4
