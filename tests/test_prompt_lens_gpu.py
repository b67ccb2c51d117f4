"""Exact lengths in the prompt stage on HIP (flamed_enc_encode_lens, flamed_vq_encode_lens): every prompt of a padded
batch against the oracle on that prompt alone, f32 and bf16 encoder handles.  Shapes, bars and references:
tests/_promptlens.py.

  parity           encoder frames, codes, outs / qbuf per frame, last-LayerNorm rows and spk of every utterance alone
                   (both attn_mfma settings); behind every end exact 0 / the pad code, as whole slices
  padding          0, 100 x randn, NaN and inf behind every end: four bitwise equal, finite results
  neighbours       utterance 1 replaced (data and length): every other utterance bitwise unchanged
  position row     the utterances permuted: spk, codes and z bitwise what they were at their old index (pe[0] for all)
  dense identity   lens = [n] * B is the call without lens, graph on and off; the dense call is unchanged after a ragged
                   one; the VQ call at B = 1, lens = [T] likewise
  stale state      dense large -> ragged A -> ragged B -> dense small -> ragged A on one handle, graph on == graph off
  pipeline         Flamed.encode_prompts against solo calls, its result through sample_batch; synthesize.py
                   --batch-prompts true in metadata mode"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _common import PKG, golden, t32, rel_l2
import _promptprofile as pp
import _promptlens as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VQ_KEYS = ("codes", "outs", "qbuf", "rows", "spk")


@pytest.fixture(scope="module")
def encs():
    return {m: pl.make_encoder(m, DEV) for m in ("f32", "bf16")}


@pytest.fixture(scope="module")
def dec():
    return pl.make_decoder(DEV)


def _tune(**knobs):
    from flamed import _native as nat
    for k, v in knobs.items():
        nat.check(nat.lib().flamed_tune(k.encode(), int(v)), "flamed_tune")


def _enc(e, wav, lens=None, graph=True):
    e.hip_graph = graph
    try:
        with torch.inference_mode():
            z = e(wav.to(DEV), lens=lens).cpu()
    finally:
        e.hip_graph = True
    assert e._hip is not None and e._hip.dtype_name == e.hip_dtype  # the HIP path ran
    return z


def _vq(d, x, lens=None, graph=True, pad=None):
    """One (ragged) quantizer / timbre call -> CPU {codes, outs, qbuf (G, B, 256, T), rows (B, T, 256), spk}; the rows
    are the workspace's H buffer, which mean_t_kernel has just averaged."""
    from flamed import _native as nat
    B, _, T = x.shape
    d.hip_graph = graph
    try:
        with torch.inference_mode():
            outs, codes, _, qb, spk = d(x.to(DEV), eval_vq=False, vq=True, lens=lens, pad_code=pad)
            h = d._vq_hip
            assert h is not None and h.handle is not None  # the HIP path ran
            off = (ctypes.c_size_t * 6)()
            nat.check(nat.lib().flamed_vq_ws_offsets(h.handle, B, T, off), "flamed_vq_ws_offsets")
            rows = h.ws.buf[off[2]:off[2] + 4 * B * T * 256].view(torch.float32).view(B, T, 256).clone()
    finally:
        d.hip_graph = True
    return {"codes": codes.cpu(), "outs": outs.cpu(), "qbuf": torch.stack(list(qb)).cpu(), "rows": rows.cpu(), "spk": spk.cpu()}


def _same(a, b, what, sel=None):
    for k in VQ_KEYS:
        u, v = a[k], b[k]
        if sel is not None:  # utterance axis: codes (n_q, B, T), qbuf (G, B, C, T), the others (B, ...)
            ax = 1 if k in ("codes", "qbuf") else 0
            u, v = u.index_select(ax, sel), v.index_select(ax, sel)
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {k} differs"


def _check_vq(o, lens, refs, label):
    assert all(torch.isfinite(o[k]).all() for k in ("outs", "qbuf", "rows", "spk"))
    pl.check_codes(o["codes"], lens, refs, label)
    pl.check_quantized(o, lens, refs, label)
    pl.check_timbre(o, lens, refs, label)
    for u, Tu in enumerate(lens):
        assert torch.count_nonzero(o["rows"][u, Tu:]) == 0, f"{label}: utterance {u}: rows behind its end are not 0"


# ------------------------------------------------------------------------------------------------------------
# parity of each utterance alone
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n,lens", pl.E2E_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_end_to_end_each_utterance_alone(encs, dec, mode, B, n, lens):
    """Encoder frames of both handles; behind the f32 encoder the ragged quantizer / timbre call: codes equal to the
    oracle's (no near-tie on these shapes: none excused), spk at the bar of the existing chained check, exact 0 / pad
    behind every end."""
    wav, per = pl.e2e_case(B, n, lens)
    z = _enc(encs[mode], pl.filled(wav, lens, "big"), lens)
    assert z.shape == (B, 256, pl.out_len(n))
    pl.check_encoder(mode, z, lens, per, f"e2e {B}x{n}")
    if mode != "f32":
        return
    frames = [pl.out_len(m) for m in lens]
    refs = [p["vq"] for p in per]
    o = _vq(dec, z, frames)
    pl.check_codes(o["codes"], frames, refs, f"e2e {B}x{n}")
    for u, Tu in enumerate(frames):
        assert not bool((o["codes"][:, u, :Tu] != refs[u]["r32"]["codes"][:, 0]).any()), "code mismatch (none excused)"
        rel = rel_l2(o["spk"][u:u + 1], refs[u]["r32"]["spk"])
        print(f"e2e {B}x{n} utterance {u}: spk rel-L2 behind the HIP encoder {rel:.2e}")
        assert rel < pl.SPK_CHAIN
        assert torch.count_nonzero(o["outs"][u, :, Tu:]) == 0 and torch.count_nonzero(o["qbuf"][:, u, :, Tu:]) == 0


@pytest.mark.parametrize("attn_mfma", [1, 0])
@pytest.mark.parametrize("B,T,lens", pl.VQ_SHAPES, ids=lambda v: str(v))
def test_vq_timbre_each_utterance_alone(dec, B, T, lens, attn_mfma):
    x, refs = pl.vq_case(B, T, lens)
    try:
        _tune(attn_mfma=attn_mfma)
        o = _vq(dec, pl.filled(x, lens, "big"), lens)
    finally:
        _tune(attn_mfma=1)
    _check_vq(o, lens, refs, f"vq ({B}, {T}) attn_mfma={attn_mfma}")
    if (B, T) != (3, 130):  # no oracle near-tie on these: no mismatch is excused
        for u, Tu in enumerate(lens):
            assert not bool((o["codes"][:, u, :Tu] != refs[u]["r32"]["codes"][:, 0]).any()), "code mismatch (none excused)"


# ------------------------------------------------------------------------------------------------------------
# padding, neighbours, position row: bitwise
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_padding_is_never_read(encs, mode):
    B, n, lens = pl.E2E_SHAPES[1]
    wav, _ = pl.e2e_case(B, n, lens)
    zs = [_enc(encs[mode], pl.filled(wav, lens, kind), lens) for kind in pl.FILLS]
    assert torch.isfinite(zs[0]).all()
    for kind, z in zip(pl.FILLS[1:], zs[1:]):
        assert torch.equal(zs[0], z), f"the encoder output moved with the padding ({kind})"


@pytest.mark.parametrize("attn_mfma", [1, 0])
def test_vq_padding_is_never_read(dec, attn_mfma):
    B, T, lens = pl.VQ_SHAPES[0]
    x, _ = pl.vq_case(B, T, lens)
    try:
        _tune(attn_mfma=attn_mfma)
        os_ = [_vq(dec, pl.filled(x, lens, kind), lens) for kind in pl.FILLS]
    finally:
        _tune(attn_mfma=1)
    assert all(torch.isfinite(os_[0][k]).all() for k in ("outs", "qbuf", "rows", "spk"))
    for kind, o in zip(pl.FILLS[1:], os_[1:]):
        _same(os_[0], o, f"the result moved with the padding ({kind})")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_neighbours(encs, mode):
    B, n, lens = pl.E2E_SHAPES[0]
    wav, _ = pl.e2e_case(B, n, lens)
    wavb = wav.clone()
    wavb[1] = pl.wav_input(B, n, seed=1)[1]
    lensb = (lens[0], 1200, lens[2])
    a, b = _enc(encs[mode], wav, lens), _enc(encs[mode], wavb, lensb)
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "an utterance changed with its neighbour"


def test_vq_neighbours(dec):
    B, T, lens = pl.VQ_SHAPES[0]
    x, _ = pl.vq_case(B, T, lens)
    xb = x.clone()
    xb[1] = pp.case_input(B, T, 1)[1]
    a, b = _vq(dec, x, lens), _vq(dec, xb, (lens[0], 17, lens[2]))
    assert not torch.equal(a["spk"][1], b["spk"][1])
    _same(a, b, "an utterance changed with its neighbour", torch.tensor([0, 2]))


def test_position_row_is_the_same_for_every_utterance(encs, dec):
    """A permuted batch: every utterance keeps its spk, codes and encoder frames bitwise (the dense call would hand it
    another position row, pe[b])."""
    perm = [2, 0, 3, 1]
    B, T, lens = pl.VQ_SHAPES[2]
    x, _ = pl.vq_case(B, T, lens)
    a = _vq(dec, x, lens)
    b = _vq(dec, x[perm], [lens[i] for i in perm])
    for new, old in enumerate(perm):
        assert torch.equal(b["spk"][new], a["spk"][old]) and torch.equal(b["codes"][:, new], a["codes"][:, old]), (new, old)
        assert torch.equal(b["outs"][new], a["outs"][old])
    B, n, lens = pl.E2E_SHAPES[1]
    wav, _ = pl.e2e_case(B, n, lens)
    za = _enc(encs["f32"], wav, lens)
    zb = _enc(encs["f32"], wav[perm], [lens[i] for i in perm])
    for new, old in enumerate(perm):
        assert torch.equal(zb[new], za[old]), (new, old)


# ------------------------------------------------------------------------------------------------------------
# dense identity, graph replay, stale state
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_dense_identity(encs, mode):
    e = encs[mode]
    B, n, lens = pl.E2E_SHAPES[0]
    wav, _ = pl.e2e_case(B, n, lens)
    for graph in (True, False):
        dense = _enc(e, wav, graph=graph)
        assert torch.equal(_enc(e, wav, [n] * B, graph=graph), dense), f"graph={graph}"
        ragged = _enc(e, wav, lens, graph=graph)
        assert not torch.equal(ragged, dense)
        assert torch.equal(_enc(e, wav, graph=graph), dense), f"the dense call moved after a ragged one (graph={graph})"


def test_vq_dense_identity_at_one_full_utterance(dec):
    x = pp.case_input(1, 7)
    for graph in (True, False):
        dense = _vq(dec, x, graph=graph)
        _same(_vq(dec, x, [7], graph=graph), dense, f"B = 1, lens = [T] (graph={graph})")
        _vq(dec, x, [3], graph=graph)
        _same(_vq(dec, x, graph=graph), dense, f"the dense call moved after a ragged one (graph={graph})")
    # B > 1 with every length T is NOT the dense call: pe[0] against pe[b]
    x2 = pp.case_input(2, 9)
    a, b = _vq(dec, x2), _vq(dec, x2, [9, 9])
    assert torch.equal(a["codes"], b["codes"]) and not torch.equal(a["spk"][1], b["spk"][1])
    assert rel_l2(b["spk"][0:1], a["spk"][0:1]) < 1e-5


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encoder_sequence_no_stale_state(encs, mode):
    """dense large -> ragged A -> ragged B (same (B, n), other lengths) -> dense small -> ragged A on one handle."""
    e = encs[mode]
    B, n, la = pl.E2E_SHAPES[0]
    lb = (403, 2600, 1999)
    wav, _ = pl.e2e_case(B, n, la)
    wavb, perb = pl.e2e_case(B, n, lb)
    big, small = pl.wav_input(3, 2755, seed=2), pl.wav_input(1, 152, seed=2)
    runs = {}
    for graph in (True, False):
        _enc(e, big, graph=graph)
        a1 = _enc(e, wav, la, graph=graph)
        b = _enc(e, wavb, lb, graph=graph)
        _enc(e, small, graph=graph)
        a2 = _enc(e, wav, la, graph=graph)
        assert torch.equal(a1, a2), f"graph={graph}"
        pl.check_encoder(mode, b, lb, perb, f"ragged B after A (graph={graph})")
        runs[graph] = (a1, b)
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])


def test_vq_sequence_no_stale_state(dec):
    B, T, la = pl.VQ_SHAPES[2]
    lb = (9, 8, 5, 1)
    x, _ = pl.vq_case(B, T, la)
    xb, refb = pl.vq_case(B, T, lb)
    big, small = pp.case_input(3, 161), pp.case_input(1, 1)
    runs = {}
    for graph in (True, False):
        _vq(dec, big, graph=graph)
        a1 = _vq(dec, x, la, graph=graph)
        b = _vq(dec, xb, lb, graph=graph)
        _vq(dec, small, graph=graph)
        a2 = _vq(dec, x, la, graph=graph)
        _same(a1, a2, f"ragged A again (graph={graph})")
        _check_vq(b, lb, refb, f"ragged B after A (graph={graph})")
        runs[graph] = (a1, b)
    _same(runs[True][0], runs[False][0], "graph against eager, A")
    _same(runs[True][1], runs[False][1], "graph against eager, B")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tile_skip_changes_no_bit(encs, mode):
    """tn().enc_skip: row tiles wholly behind an end exit at once; with it off they run and store rows nobody reads."""
    B, n, lens = pl.E2E_SHAPES[0]
    wav, _ = pl.e2e_case(B, n, lens)
    on = _enc(encs[mode], wav, lens)
    try:
        _tune(enc_skip=0)
        off = _enc(encs[mode], wav, lens)
    finally:
        _tune(enc_skip=1)
    assert torch.equal(on, off)


# ------------------------------------------------------------------------------------------------------------
# pipeline
# ------------------------------------------------------------------------------------------------------------

def test_encode_prompts_against_solo_calls(encs):
    from _flamed_common import build_flamed
    m, cdec = build_flamed(DEV, "f32")
    enc = encs["f32"]
    B, n, lens = pl.E2E_SHAPES[0]
    wav, per = pl.e2e_case(B, n, lens)
    prompts = [wav[u, 0, :lens[u]].clone() for u in range(B)]
    codes, plens, timbres = m.encode_prompts([prompts[0].numpy(), prompts[1], prompts[2].numpy()], sr=16000,
                                             codec_encoder=enc, codec_decoder=cdec)
    assert plens == [13, 10, 2] and codes.shape == (3, 6, 13) and timbres.shape == (3, 256)
    pad = m.prior_generator.code_embedding.padding_idx
    with torch.inference_mode():
        for u in range(B):  # as synthesize.encode_prompt_features encodes one prompt
            _, c, _, _, t = cdec(enc(prompts[u].reshape(1, 1, -1).to(DEV)), eval_vq=False, vq=True)
            assert torch.equal(codes[u, :, :plens[u]], c.permute(1, 0, 2)[0]), f"prompt {u}: codes differ from alone"
            assert bool((codes[u, :, plens[u]:] == pad).all())
            r = per[u]["vq"]
            se = float(pp.spk_err(timbres[u:u + 1].cpu(), t.cpu(), r["r64"]["rows"]).max())
            print(f"encode_prompts prompt {u}: timbre against the solo call {se:.2e}")
            assert se <= pp.bar_of(pp.floors(r)["spk"])
    pl.check_codes(codes.permute(1, 0, 2).cpu(), plens, [p["vq"] for p in per], "encode_prompts")
    g = golden("flamed_sample")
    ph = t32(g["phonemes"])[:1].repeat(3, 1)
    out = m.sample_batch(phonemes=ph, src_lens=t32(g["src_lens"])[:1].repeat(3), prompts=codes, timbres=timbres,
                         nsteps_durgen=4, nsteps_denoiser=4, exact_prior=True, prompt_lens=plens)
    assert out["latents"].shape[0] == 3 and torch.isfinite(out["latents"]).all()


def test_cli_metadata_mode_batch_prompts(tmp_path):
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed.utils.audio import load_wav, write_wav
    from flamed.utils.random_ckpt import write
    paths = write(str(tmp_path / "ck"))
    pr = tmp_path / "pr"
    os.makedirs(pr)
    rng = np.random.default_rng(0)
    for i in range(2):
        write_wav(str(pr / f"p{i}.wav"), rng.normal(0, 0.1, 8000 + 4000 * i).astype(np.float32), 16000)
    meta = tmp_path / "meta.txt"
    meta.write_text("u0.wav|p0.wav|hello world.\nu1.wav|p1.wav|good morning to you all.\n")
    args = syn.build_arg_parser().parse_args([
        "--ckpt-path", paths["ckpt"], "--cfg-path", paths["cfg"], "--codec-ckpt-dir", str(tmp_path / "ck"),
        "--text-file", str(meta), "--input-dir", str(pr), "--output-dir", str(tmp_path / "out"),
        "--device", "cuda:0", "--nsteps-durgen", "8", "--nsteps-denoiser", "8", "--batch-size", "2",
        "--batch-prompts", "true"])
    rtf = syn.main(args)
    assert rtf is not None and rtf > 0
    d = tmp_path / "out" / "nfe8-temp0.3"  # the flag adds nothing to a name
    assert sorted(os.listdir(d)) == ["u0.wav", "u1.wav"]
    for name in ("u0.wav", "u1.wav"):
        w = load_wav(str(d / name), 16000)
        assert len(w) > 0 and len(w) % 200 == 0 and np.all(np.isfinite(w))
