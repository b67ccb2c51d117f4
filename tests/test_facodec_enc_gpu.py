"""HIP FaCodec encoder (prompt encoding) vs the reference fixture and the oracle.
Tolerances: exact-fp32 MFMA mode rel-L2 <= 2e-5 (reassociation only) and the RVQ codes computed from
it bit-identical to the reference's; bf16 mode: error vs the fp32 reference within 1 dB of what the
reference itself reaches under CPU bf16 autocast (rel-L2 <= 1.122 x, as the decoder test); graph
replay == eager bitwise.
Frame profile (tests/_codecprofile.py; weight-norm gains x the `facodec_calm` gain, as the decoder's profile
tests): no output frame of the bf16 mode stands further from the oracle than 1.2 x the worst frame of the bf16
emulation on the same inputs; the f32 mode holds every frame within F32_FRAME_BAR (1e-5)."""
import numpy as np
import pytest
import torch

from _common import golden, seeded, t32, rel_l2, orc
from _flamed_common import build_codec_encoder
from _codecprofile import emulated_encode, frame_errors, assert_frame_profile, F32_FRAME_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def enc():
    return build_codec_encoder(DEV)


def test_encode_golden_f32(enc):
    g = golden("facodec_encode")
    enc.hip_dtype = "f32"
    with torch.inference_mode():
        z = enc(t32(g["wav"]).to(DEV))
    assert enc._hip is not None and enc._hip.dtype_name == "f32"  # the HIP path ran
    assert z.shape == g["enc_out"].shape
    assert rel_l2(z.cpu(), g["enc_out"]) < 2e-5


def test_codes_from_hip_encoder_match_reference(enc):
    from _flamed_common import build_flamed
    _, dec = build_flamed(DEV, "f32")
    g = golden("facodec_encode")
    enc.hip_dtype = "f32"
    with torch.inference_mode():
        _, codes, _, _, spk = dec(enc(t32(g["wav"]).to(DEV)), eval_vq=False, vq=True)
    assert np.array_equal(codes.cpu().numpy(), g["codes"])
    assert rel_l2(spk.cpu(), g["spk"]) < 1e-4


@pytest.mark.parametrize("n", [8137, 1000, 16003])
def test_encode_odd_lengths_vs_oracle(enc, n):
    gen = torch.Generator().manual_seed(n)
    wav = 0.1 * torch.randn(1, 1, n, generator=gen)
    ref = orc.facodec_encode(seeded("facodec_encoder"), wav)
    enc.hip_dtype = "f32"
    with torch.inference_mode():
        z = enc(wav.to(DEV))
    assert z.shape == ref.shape
    assert rel_l2(z.cpu(), ref) < 2e-5


def test_encode_bf16_and_graph(enc):
    g = golden("facodec_encode")
    x = t32(g["wav"]).to(DEV)
    enc.hip_dtype = "bf16"
    try:
        with torch.inference_mode():
            enc.hip_graph = False
            z_eager = enc(x)
            enc.hip_graph = True
            z_graph = enc(x)
            z_graph2 = enc(x)
    finally:
        enc.hip_dtype = "f32"
        enc.hip_graph = True
    assert torch.equal(z_eager, z_graph) and torch.equal(z_graph, z_graph2)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        ref_bf16 = orc.facodec_encode(seeded("facodec_encoder"), t32(g["wav"])).float()
    e_ref = rel_l2(ref_bf16, g["enc_out"])
    assert rel_l2(z_graph.cpu(), g["enc_out"]) < 1.122 * max(e_ref, 1e-3)


@pytest.mark.parametrize("B,T", [(2, 240), (1, 37)])
def test_vq_timbre_vs_oracle(B, T):
    """Prompt-side RVQ codes + timbre speaker embedding on HIP (flamed_vq_encode) vs the oracle
    (decoder_vq: facodec.py:470-533) on random encoder outputs.  Codes bit-exact except where the
    oracle's top-2 distance gap is below 1e-5 (fp32 summation-order ties; at most as many excused cells as the
    oracle has near-ties), spk rel-L2 <= 1e-4; quantized sums vs the module's own torch path on CPU on every frame
    without a code mismatch.  Per-row and per-frame profiles: tests/test_prompt_profile_gpu.py."""
    from _flamed_common import build_flamed
    _, dec = build_flamed(DEV, "f32")
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    x = torch.randn(B, 256, T, generator=torch.Generator().manual_seed(11))
    with torch.inference_mode():
        outs, codes, _, qb, spk = dec(x.to(DEV), eval_vq=False, vq=True)
        gaps = []
        rc, rspk = orc.decoder_vq(sd, x, gaps=gaps)
        dec_cpu = dec.to("cpu")
        couts, ccodes, _, cqb, cspk = dec_cpu(x, eval_vq=False, vq=True)
        dec.to(DEV)
    assert dec._vq_hip is not None and dec._vq_hip.handle is not None  # the HIP path ran
    codes = codes.cpu()
    assert codes.shape == rc.shape
    near = torch.stack(gaps) < 1e-5  # (n_q, B, T) near-ties of the oracle's own distances
    neq = codes != rc
    # a mismatch in one layer changes every later residual of that group: only frames whose first
    # mismatch sits on a near-tie are excused
    first = neq.float().cumsum(0) == 1
    assert bool((near | ~(neq & first)).all()), "code mismatch away from a near-tie"
    # ... and never more of them than the oracle itself has near-ties
    assert int((neq & first).sum()) <= int(near.sum()), "more excused cells than the oracle has near-ties"
    assert rel_l2(spk.cpu(), rspk) < 1e-4
    # quantized sums on every frame whose codes all match (a mismatching frame carries another code vector)
    keep = ~neq.any(0)  # (B, T)
    assert int((~keep).sum()) <= int(near.sum()) and bool(keep.any())
    sel = keep.unsqueeze(1).expand(-1, 256, -1)
    assert rel_l2(outs.cpu()[sel], couts[sel]) < 1e-4
    assert len(qb) == len(cqb)
    for a, b in zip(qb, cqb):
        assert rel_l2(a.cpu()[sel], b[sel]) < 1e-4


# ------------------------------------------------------------------------------------------------------------
# frame profiles at the edges (tests/_codecprofile.py)
# ------------------------------------------------------------------------------------------------------------
F32_REL = 2e-5  # the file's f32 bar, here per utterance; every frame: F32_FRAME_BAR (20 x the oracle's own
                # reassociation noise, tests/_codecprofile.py)


@pytest.fixture(scope="module")
def calm_enc():
    from flamed.utils.seeded_init import scale_weight_norm_gains
    sd = scale_weight_norm_gains(seeded("facodec_encoder"), float(golden("facodec_calm")["gain"]))
    encs = {}
    for mode in ("f32", "bf16"):
        e = build_codec_encoder("cpu")
        e.load_state_dict(sd)
        e.hip_dtype = mode
        encs[mode] = e.to(DEV)
    return encs, sd


_cases = {}


def _case(sd, B, n, seed=0):
    """(wav, oracle, bf16 emulation) of one seeded input, computed once per run."""
    key = (B, n, seed)
    if key not in _cases:
        wav = 0.1 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(1000 * B + n + 7919 * seed))
        _cases[key] = (wav, orc.facodec_encode(sd, wav), emulated_encode(sd, wav))
    return _cases[key]


def _encode(e, wav):
    with torch.inference_mode():
        z = e(wav.to(DEV)).cpu()
    assert e._hip is not None and e._hip.dtype_name == e.hip_dtype  # the HIP path ran
    return z


def _check(mode, z, ref, floor, label):
    assert z.shape == ref.shape
    if mode == "f32":
        rels = [rel_l2(z[i], ref[i]) for i in range(z.shape[0])]
        e = frame_errors(z, ref)
        print(f"{label} f32: rel-L2 per utterance max {max(rels):.2e}, frame max {float(e.max()):.2e}, "
              f"median {float(e.median()):.2e}")
        assert max(rels) < F32_REL
        assert float(e.max()) <= F32_FRAME_BAR
    else:
        assert_frame_profile(z, ref, floor, f"{label} bf16")


# stage lengths floor(n / 2), floor(. / 4), floor((. + 1) / 5), floor((. + 1) / 5)
ENC_EDGE_SHAPES = [
    (1, 152),   # the shortest legal input, one output frame
    (3, 152),   # the same with utterance edges
    (2, 1001),  # odd remainders at every stride
    (3, 2055),  # an utterance edge inside every tile size; the first-stage C = 32 path at 6,165 rows
    (2, 8137),  # the odd length of test_encode_odd_lengths_vs_oracle, batched
]


@pytest.mark.parametrize("B,n", ENC_EDGE_SHAPES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encode_edge_profiles(calm_enc, mode, B, n):
    encs, sd = calm_enc
    wav, ref, floor = _case(sd, B, n)
    _check(mode, _encode(encs[mode], wav), ref, floor, f"edge {B}x{n}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encode_too_short_raises(calm_enc, mode):
    """152 samples are the shortest input the stride chain accepts (152 -> 76 -> 19 -> 4 -> 1); 151 leave 3 samples
    to the last k10 conv, which does not fit (the oracle's conv1d raises): ValueError before any launch."""
    encs, sd = calm_enc
    e = encs[mode]
    for B in (1, 3):
        with pytest.raises(ValueError, match="too short"), torch.inference_mode():
            e(torch.zeros(B, 1, 151, device=DEV))
        with pytest.raises(RuntimeError):
            orc.facodec_encode(sd, torch.zeros(B, 1, 151))
        assert _encode(e, _case(sd, B, 152)[0]).shape == (B, 256, 1)
    assert e._hip.out_len(151) == 0 and e._hip.out_len(1) == 0 and e._hip.out_len(152) == 1


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encode_batch_isolation(calm_enc, mode):
    """As test_decode_batch_isolation, at (3, 1001)."""
    encs, sd = calm_enc
    e = encs[mode]
    B, n = 3, 1001
    wav, ref, floor = _case(sd, B, n)
    wavb = wav.clone()
    wavb[1] = _case(sd, B, n, seed=1)[0][1]
    a, b = _encode(e, wav), _encode(e, wavb)
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "an utterance changed with its neighbour"
    for i in range(B):
        alone = _encode(e, wav[i:i + 1])
        _check(mode, alone, ref[i:i + 1], floor[i:i + 1], f"isolation {B}x{n} utterance {i} alone")
        if mode == "f32":
            assert rel_l2(alone[0], a[i]) < F32_REL


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_encode_shape_sequence_no_stale_state(calm_enc, mode):
    """(1, 152) -> (3, 2055) -> (1, 152) on one handle, graph on then off: the third result equals the first
    bitwise."""
    encs, sd = calm_enc
    e = encs[mode]
    wav = _case(sd, 1, 152)[0]
    big = _case(sd, 3, 2055, seed=2)[0]
    try:
        for graph in (True, False):
            e.hip_graph = graph
            first = _encode(e, wav)
            mid = _encode(e, big)
            third = _encode(e, wav)
            assert mid.shape == (3, 256, 10) and torch.isfinite(mid).all()
            assert torch.equal(first, third), f"graph={graph}"
    finally:
        e.hip_graph = True
