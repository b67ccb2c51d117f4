"""GPU parity: HIP FaCodec decoder (FACodecDecoder.inference) vs reference golden waveforms and the
oracle.

* Seeded unit-gain weights (golden `facodec`): the decoder is chaotic there (~85-90 % of samples
  saturate the tanh); f32 mode per-sample max |diff| <= 5e-4; bf16 SNR no worse than the reference's
  own bf16 behaviour (oracle under torch.autocast(cpu, bfloat16)) minus 1 dB.
* Non-saturating weights (golden `facodec_calm`, weight-norm gains x 0.6; output std 0.04, no
  saturation): SURVEY.md §8(c)'s absolute bars — f32 max |diff| <= 5e-3 (measured far below), bf16
  SNR >= 30 dB — at T = 64 against the reference fixture and at the bench length T = 400 (80,000
  samples, the bench's bf16 decode) against the oracle.
* Window profile (tests/_codecprofile.py), calm weights only: no window of 25 samples of the bf16 waveform
  stands further from the oracle than 1.4 x the worst window of the bf16 emulation on the same inputs -- at the
  shapes that put utterance, tile and config edges inside the decode, across batch neighbours (bitwise) and
  across a sequence of shapes on one handle (bitwise)."""
import math

import numpy as np
import pytest
import torch

from _common import golden, seeded, t32, rel_l2, orc
from _codecprofile import emulated_decode, window_errors, assert_window_profile, W_DEC, F32_WINDOW_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dec(dtype):
    from flamed.models.facodec import FACodecDecoder
    d = FACodecDecoder(in_channels=256, upsample_initial_channel=1024, ngf=32, up_ratios=[5, 5, 4, 2],
                       vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256, codebook_dim=8,
                       use_gr_x_timbre=True, use_gr_residual_f0=True, use_gr_residual_phone=True).eval()
    sd = seeded("facodec_decoder")
    d.load_state_dict(sd)
    d.hip_dtype = dtype
    return d.to(DEV), sd


@pytest.fixture(scope="module")
def dec_f32():
    return _dec("f32")


@pytest.fixture(scope="module")
def dec_bf16():
    return _dec("bf16")


def snr_db(x, ref):
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    return 10 * math.log10(np.sum(ref ** 2) / max(np.sum((x - ref) ** 2), 1e-30))


def ref_bf16_snr(sd, lat, spk, ref):
    with torch.autocast("cpu", dtype=torch.bfloat16):
        w = orc.facodec_decode(sd, t32(lat), t32(spk)).float().numpy()
    return snr_db(w, ref)


def _run(dec, lat, spk):
    with torch.inference_mode():
        return dec.inference(t32(lat).to(DEV), t32(spk).to(DEV)).cpu().numpy()


def test_state_dict_schema_and_extra_keys(dec_f32):
    d, sd = dec_f32
    assert set(d.state_dict().keys()) <= set(sd.keys())
    assert all(k.split(".")[0] in ("model", "timbre_linear", "timbre_encoder", "quantizer") for k in d.state_dict())
    assert len(d.unused_state) == len(sd) - len(d.state_dict())
    assert all(k.split(".")[0].endswith("_predictor") for k in d.unused_state)


@pytest.mark.parametrize("case", ["1", "2"])
def test_decode_golden_f32(case, dec_f32):
    d, _ = dec_f32
    g = golden("facodec")
    wav = _run(d, g["lat" + case], g["spk" + case])
    assert wav.shape == g["wav" + case].shape
    assert np.max(np.abs(wav - g["wav" + case])) < 5e-4


@pytest.mark.parametrize("case", ["1", "2"])
def test_decode_golden_bf16_snr(case, dec_bf16):
    d, sd = dec_bf16
    g = golden("facodec")
    wav = _run(d, g["lat" + case], g["spk" + case])
    floor = ref_bf16_snr(sd, g["lat" + case], g["spk" + case], g["wav" + case])
    assert snr_db(wav, g["wav" + case]) > floor - 1.0


def test_decode_longer_vs_oracle(dec_f32, dec_bf16):
    gen = torch.Generator().manual_seed(12)
    lat = torch.randn(2, 256, 37, generator=gen)
    spk = torch.randn(2, 256, generator=gen)
    _, sd = dec_f32
    ref = orc.facodec_decode(sd, lat, spk).numpy()
    w32 = _run(dec_f32[0], lat, spk)
    assert np.max(np.abs(w32 - ref)) < 5e-4
    assert snr_db(_run(dec_bf16[0], lat, spk), ref) > ref_bf16_snr(sd, lat, spk, ref) - 1.0


def _calm(dtype):
    from flamed.utils.seeded_init import scale_weight_norm_gains
    d, sd = _dec(dtype)
    sd = scale_weight_norm_gains(sd, float(golden("facodec_calm")["gain"]))
    with torch.inference_mode():
        d.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=False)
    return d, sd


@pytest.fixture(scope="module")
def calm():
    return {"f32": _calm("f32"), "bf16": _calm("bf16")}


def test_decode_calm_golden(calm):
    g = golden("facodec_calm")
    w32 = _run(calm["f32"][0], g["lat"], g["spk"])
    wbf = _run(calm["bf16"][0], g["lat"], g["spk"])
    d32, sbf = float(np.max(np.abs(w32 - g["wav"]))), snr_db(wbf, g["wav"])
    print(f"calm T=64: f32 max|d| {d32:.2e}, bf16 SNR {sbf:.1f} dB")
    assert d32 < 5e-3 and sbf >= 30.0
    floor = emulated_decode(calm["bf16"][1], t32(g["lat"]), t32(g["spk"]))
    assert_window_profile(wbf, t32(g["wav"]), floor, "calm golden 1x64")


def test_decode_calm_bench_length(calm):
    """The bench's decode shape (T = 400 frames -> 80,000 samples) vs the oracle."""
    gen = torch.Generator().manual_seed(40)
    lat = torch.randn(1, 256, 400, generator=gen)
    spk = torch.randn(1, 256, generator=gen)
    ref = orc.facodec_decode(calm["f32"][1], lat, spk).numpy()
    w32 = _run(calm["f32"][0], lat, spk)
    wbf = _run(calm["bf16"][0], lat, spk)
    d32, sbf = float(np.max(np.abs(w32 - ref))), snr_db(wbf, ref)
    print(f"calm T=400: f32 max|d| {d32:.2e}, bf16 SNR {sbf:.1f} dB")
    assert wbf.shape == (1, 1, 80000)
    assert d32 < 5e-3 and sbf >= 30.0
    assert_window_profile(wbf, ref, emulated_decode(calm["bf16"][1], lat, spk), "calm bench length 1x400")


def test_graph_equals_eager(dec_f32):
    d, _ = dec_f32
    gen = torch.Generator().manual_seed(4)
    lat = torch.randn(1, 256, 11, generator=gen)
    spk = torch.randn(1, 256, generator=gen)
    d.hip_graph = True
    a = _run(d, lat, spk)
    b = _run(d, lat, spk)
    d.hip_graph = False
    c = _run(d, lat, spk)
    d.hip_graph = True
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------------------
# window profiles at the edges (calm weights; tests/_codecprofile.py)
# ------------------------------------------------------------------------------------------------------------
F32_BAR = 5e-3  # SURVEY.md 8(c), as test_decode_calm_*
_cases = {}


def _case(sd, B, T, seed=0):
    """(lat, spk, oracle, bf16 emulation) of one seeded input, computed once per run."""
    key = (B, T, seed)
    if key not in _cases:
        gen = torch.Generator().manual_seed(1000 * B + T + 7919 * seed)
        lat = torch.randn(B, 256, T, generator=gen)
        spk = torch.randn(B, 256, generator=gen)
        _cases[key] = (lat, spk, orc.facodec_decode(sd, lat, spk), emulated_decode(sd, lat, spk))
    return _cases[key]


def _check(mode, out, ref, floor, label):
    """f32: per-sample bar and worst window within 20 x the oracle's own reassociation noise; bf16: window profile +
    whole-signal SNR within 1 dB of the emulation's own."""
    out = torch.as_tensor(out)
    assert out.shape == ref.shape
    if mode == "f32":
        d, w = float((out - ref).abs().max()), float(window_errors(out, ref, W_DEC).max())
        print(f"{label} f32: max|d| {d:.2e}, window max {w:.2e}")
        assert d < F32_BAR
        assert w <= F32_WINDOW_BAR
    else:
        assert_window_profile(out, ref, floor, f"{label} bf16")
        s, sf = snr_db(out, ref), snr_db(floor, ref)
        print(f"{label} bf16: SNR {s:.1f} dB, emulation {sf:.1f} dB")
        assert s >= sf - 1.0


# stage lengths T x {1, 5, 25, 100, 200}; GEMM rows B n (B (n + 1) for the conv-transpose)
EDGE_SHAPES = [
    (1, 1),    # every stage shorter than the dilation-9 reach until n = 100; replicate padding on both sides
    (1, 2), (2, 1),  # an utterance edge with n = 1
    (3, 13),   # n = 65: one 64-sample act1d tile + 1; 2,600 = 20 x 128 + 40 in fac_out; rows 39 .. 7,800: utterance
               # edges inside 32- and 64-row tiles, the 2,048-row config switch inside the decode
    (2, 32),   # n = 3,200 / 6,400: utterance edge = act1d tile edge = fac_out tile edge = GEMM tile edge
    (1, 41),   # 8,200 rows: first shape on the 128-row config, last tile of 8 rows
    (5, 7),    # five utterance edges, odd everything
]


@pytest.mark.parametrize("B,T", EDGE_SHAPES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_edge_profiles(calm, mode, B, T):
    d, sd = calm[mode]
    lat, spk, ref, floor = _case(sd, B, T)
    _check(mode, _run(d, lat, spk), ref, floor, f"edge {B}x{T}")


@pytest.mark.parametrize("B,T", [(3, 13), (2, 32)])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_batch_isolation(calm, mode, B, T):
    """Replacing utterance 1 (latents and speaker row) leaves the other utterances' samples bitwise: same shape,
    same tiles, same summation order, so any difference is a leak across an utterance edge.  Each utterance decoded
    alone (other tile config, other row offsets) still meets the mode's bar."""
    d, sd = calm[mode]
    lat, spk, ref, floor = _case(sd, B, T)
    lat2, spk2, _, _ = _case(sd, B, T, seed=1)
    latb, spkb = lat.clone(), spk.clone()
    latb[1], spkb[1] = lat2[1], spk2[1]
    a, b = _run(d, lat, spk), _run(d, latb, spkb)
    assert not np.array_equal(a[1], b[1])
    for i in range(B):
        if i != 1:
            assert np.array_equal(a[i], b[i]), f"utterance {i} changed with its neighbour"
    for i in range(B):
        alone = _run(d, lat[i:i + 1], spk[i:i + 1])
        _check(mode, alone, ref[i:i + 1], floor[i:i + 1], f"isolation {B}x{T} utterance {i} alone")
        if mode == "f32":
            assert float(np.max(np.abs(alone[0] - a[i]))) < F32_BAR


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_decode_shape_sequence_no_stale_state(calm, mode):
    """(1, 13) -> (3, 41) -> (1, 13) on one handle, graph on then off: the third result equals the first bitwise
    (stale workspace rows past n, a graph replayed for another shape)."""
    d, sd = calm[mode]
    lat, spk, _, _ = _case(sd, 1, 13)
    big = _case(sd, 3, 41, seed=2)
    try:
        for graph in (True, False):
            d.hip_graph = graph
            first = _run(d, lat, spk)
            mid = _run(d, big[0], big[1])
            third = _run(d, lat, spk)
            assert mid.shape == (3, 1, 8200) and np.isfinite(mid).all()
            assert np.array_equal(first, third), f"graph={graph}"
    finally:
        d.hip_graph = True
