"""CPU calibration of the codec window profile (tests/_codecprofile.py): the emulation with the identity round is
the oracle bitwise; single-site bugs planted on top of the bf16 emulation stand >= 1.5x above the bar while the
whole-waveform SNR bar (30 dB) lets (a)-(e) through; the floor of a second input seed stays within 1.3 of the
first's.  W and the factors are fixed here, before any GPU run; the table is in the helper's docstring.  Bugs
marked "recorded" are the same bugs at sites where they stay under the bf16 floor: printed, not asserted."""
import math

import pytest
import torch
import torch.nn.functional as F

from _common import golden, seeded, rel_l2, orc
from _codecprofile import (emulated_decode, emulated_encode, window_errors, frame_errors, assert_window_profile,
                           W_DEC, FACTOR_DEC, FACTOR_ENC, F32_WINDOW_BAR, F32_FRAME_BAR)

SHAPES = [(3, 13), (1, 41)]
ENC_SHAPES = [(3, 152), (3, 2055)]
SNR_BAR = 30.0     # test_decode_calm_*
MARGIN = 1.5       # every planted bug stands this far above the bar
SEED_RATIO = 1.3   # floor of a second input seed / floor of the first


_NT = torch.get_num_threads()


@pytest.fixture(scope="module", autouse=True)
def single_thread():
    """The calibration runs on one thread: the convolutions' summation order, and with it every rounding decision
    of the emulation, otherwise follows the thread count (the floor's worst window moves by up to 10 %)."""
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(_NT)


@pytest.fixture(scope="module")
def calm_sd():
    from flamed.utils.seeded_init import scale_weight_norm_gains
    return scale_weight_norm_gains(seeded("facodec_decoder"), float(golden("facodec_calm")["gain"]))


@pytest.fixture(scope="module")
def enc_sd():
    from flamed.utils.seeded_init import scale_weight_norm_gains
    return scale_weight_norm_gains(seeded("facodec_encoder"), float(golden("facodec_calm")["gain"]))


def _inputs(B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 256, T, generator=gen), torch.randn(B, 256, generator=gen)


def _wav(B, n, seed):
    return 0.1 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(seed))


def snr_db(x, ref):
    x, ref = x.double(), ref.double()
    return 10 * math.log10(float(ref.pow(2).sum()) / max(float((x - ref).pow(2).sum()), 1e-30))


# ------------------------------------------------------------------------------------------------------------
# oracle identity
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", [(2, 5), (1, 13)])
@pytest.mark.parametrize("rnd", [None, "ident"])
def test_decode_identity_round_is_the_oracle(calm_sd, B, T, rnd):
    lat, spk = _inputs(B, T, 3)
    out = emulated_decode(calm_sd, lat, spk, round=None if rnd is None else (lambda x: x))
    assert torch.equal(out, orc.facodec_decode(calm_sd, lat, spk))


def test_encode_identity_round_is_the_oracle(enc_sd):
    wav = _wav(2, 1000, 3)
    for rnd in (None, lambda x: x):
        assert torch.equal(emulated_encode(enc_sd, wav, round=rnd), orc.facodec_encode(enc_sd, wav))


def test_mutate_sees_every_site(calm_sd, enc_sd):
    seen = []

    def spy(site, y, ctx):
        seen.append((site, ctx["p"]))
        return y

    lat, spk = _inputs(1, 2, 0)
    emulated_decode(calm_sd, lat, spk, mutate=spy)
    assert [s for s, _ in seen].count("conv7") == 12 and [s for s, _ in seen].count("convt") == 4
    assert [s for s, _ in seen].count("act1d") == 4 * 7 + 1
    seen.clear()
    emulated_encode(enc_sd, _wav(1, 160, 0), mutate=spy)
    assert [s for s, _ in seen].count("conv7") == 12 and [s for s, _ in seen].count("stride") == 4
    assert [s for s, _ in seen].count("act1d") == 4 * 7 + 1


def test_window_errors_is_row_errors_over_windows():
    ref = torch.randn(2, 1, 40, generator=torch.Generator().manual_seed(0))
    out = ref.clone()
    out[1, 0, 23] += 0.5
    e = window_errors(out, ref, 10)
    assert e.shape == (8,) and int(torch.argmax(e)) == 6 and float(e.sum()) == float(e[6])
    rms = math.sqrt(float(ref.double().pow(2).sum()) / 8)
    assert abs(float(e[6]) - 0.5 / rms) < 1e-12
    with pytest.raises(AssertionError):
        assert_window_profile(out, ref, ref + 1e-3, "planted", 10, 2.0)


# ------------------------------------------------------------------------------------------------------------
# planted bugs (all on top of the bf16 emulation)
# ------------------------------------------------------------------------------------------------------------

def _act_zero_pad(sd, p, x):
    """orc.activation1d with zero padding in place of replicate padding."""
    C = x.shape[1]
    fu = sd[p + ".upsample.filter"].reshape(1, 1, -1)
    fd = sd[p + ".downsample.lowpass.filter"].reshape(1, 1, -1)
    K = fu.shape[-1]
    pad = K // 2 - 1
    pl, pr = pad * 2 + (K - 2) // 2, pad * 2 + (K - 2 + 1) // 2
    y = 2 * F.conv_transpose1d(F.pad(x, (pad, pad)), fu.expand(C, -1, -1), stride=2, groups=C)[..., pl:-pr]
    y = orc.snake_beta(y, sd[p + ".act.alpha"], sd[p + ".act.beta"])
    return F.conv1d(F.pad(y, (K // 2 - 1, K // 2)), fd.expand(C, -1, -1), stride=2, groups=C)


def bug_lost_tap(p, b, tap=0):
    """(a) one tap of a k7 conv lost at the middle sample of utterance b."""
    def m(site, y, ctx):
        if site == "conv7" and ctx["p"] == p:
            t = y.shape[2] // 2
            src = t + (tap - 3) * ctx["dil"]
            assert 0 <= src < y.shape[2]
            y = y.clone()
            y[b, :, t] -= ctx["w"][:, :, tap] @ ctx["x"][b, :, src]
        return y
    return m


def bug_edge_leak(p):
    """(b) the first sample of utterance 1 reads utterance 0's last sample through tap -1 (the m % L edge)."""
    def m(site, y, ctx):
        if site == "conv7" and ctx["p"] == p:
            assert ctx["dil"] == 1
            y = y.clone()
            y[1, :, 0] += ctx["w"][:, :, 2] @ ctx["x"][0, :, -1]
        return y
    return m


def bug_zero_pad_last(sd, p, b):
    """(c) Activation1d zero-pads instead of replicate-padding, at the last sample only."""
    def m(site, y, ctx):
        if site == "act1d" and ctx["p"] == p:
            y = y.clone()
            y[b, :, -1] = _act_zero_pad(sd, p, ctx["x"])[b, :, -1]
        return y
    return m


def bug_convt_last_row(sd, p, b):
    """(d) conv-transpose phase r = s - 1 of the last q that stores: o = q s + s - 1 - pad keeps only the bias."""
    def m(site, y, ctx):
        if site == "convt" and ctx["p"] == p:
            s, n = ctx["s"], ctx["x"].shape[2]
            pad = s // 2 + s % 2
            o = max(q * s + s - 1 - pad for q in range(n + 1) if q * s + s - 1 - pad < s * n)
            y = y.clone()
            y[b, :, o] = sd[p + ".bias"]
        return y
    return m


def bug_act_shift(p, b):
    """(e) samples 64..127 of one act1d output shifted by one sample."""
    def m(site, y, ctx):
        if site == "act1d" and ctx["p"] == p:
            y = y.clone()
            y[b, :, 64:128] = y[b, :, 63:127].clone()
        return y
    return m


def bug_stride_leak(p):
    """(f) encoder: output 0 of utterance 1 reads the last sample of utterance 0 through the tap at i = -1."""
    def m(site, y, ctx):
        if site == "stride" and ctx["p"] == p:
            s = ctx["s"]
            pad = s // 2 + s % 2
            y = y.clone()
            y[1, :, 0] += ctx["w"][:, :, pad - 1] @ ctx["x"][0, :, -1]
        return y
    return m


RECORDED = "recorded"


def decoder_bugs(sd, B):
    b = B - 1
    bugs = {
        "(a) dil-9 tap lost, last block": bug_lost_tap("model.4.block.4.block.1", b),
        "(a) dil-9 tap lost, first block": bug_lost_tap("model.1.block.4.block.1", b),
        "(c) zero pad at the last sample, block 3 pre-convT act": bug_zero_pad_last(sd, "model.3.block.0", b),
        "(d) convT last r = s-1 row lost, last stage": bug_convt_last_row(sd, "model.4.block.1", b),
        "(e) act1d 64..127 shifted, last block": bug_act_shift("model.4.block.4.block.0", b),
        "(c) the same in a residual unit of block 3, recorded": bug_zero_pad_last(sd, "model.3.block.3.block.0", b),
    }
    if B > 1:
        bugs["(b) utterance edge leak, dil-1, first block"] = bug_edge_leak("model.1.block.2.block.1")
        bugs["(b) the same in the last block, recorded"] = bug_edge_leak("model.4.block.2.block.1")
    return bugs


@pytest.fixture(scope="module")
def decoder_table(calm_sd):
    rows = {}
    for B, T in SHAPES:
        lat, spk = _inputs(B, T, 100 + T)
        ref = orc.facodec_decode(calm_sd, lat, spk)
        floor = emulated_decode(calm_sd, lat, spk)
        lat2, spk2 = _inputs(B, T, 200 + T)
        ref2 = orc.facodec_decode(calm_sd, lat2, spk2)
        floor2 = emulated_decode(calm_sd, lat2, spk2)
        r = {"floor": {}, "seed2": {}, "bugs": {}}
        Ws = (5, 10, 25, 200)
        for W in Ws:
            f = window_errors(floor, ref, W)
            r["floor"][W] = (float(f.max()), float(f.max() / f.median()))
            r["seed2"][W] = float(window_errors(floor2, ref2, W).max() / f.max())
        r["floor_snr"] = snr_db(floor, ref)
        for name, mut in decoder_bugs(calm_sd, B).items():
            out = emulated_decode(calm_sd, lat, spk, mutate=mut)
            assert not torch.equal(out, floor), name
            r["bugs"][name] = ({W: float(window_errors(out, ref, W).max()) / r["floor"][W][0] for W in Ws},
                               snr_db(out, ref))
        rows[(B, T)] = r
        print(f"\ndecoder ({B}, {T}): floor SNR {r['floor_snr']:.1f} dB; floor window max / (max/median) / seed-2 ratio: "
              + "; ".join(f"W={W} {r['floor'][W][0]:.3e} / {r['floor'][W][1]:.2f} / {r['seed2'][W]:.2f}" for W in r["floor"]))
        for name, (ratios, snr) in r["bugs"].items():
            print(f"  {name:56s} x floor " + " ".join(f"W={W} {v:6.2f}" for W, v in ratios.items()) + f"   SNR {snr:.1f} dB")
    return rows


@pytest.mark.parametrize("B,T", SHAPES)
def test_decoder_bugs_stand_above_the_bar(decoder_table, B, T):
    r = decoder_table[(B, T)]
    asserted = {k: v for k, v in r["bugs"].items() if RECORDED not in k}
    assert len(asserted) == (6 if B > 1 else 5)
    for name, (ratios, _) in asserted.items():
        assert ratios[W_DEC] >= MARGIN * FACTOR_DEC, (name, ratios)


@pytest.mark.parametrize("B,T", SHAPES)
def test_decoder_bugs_pass_the_snr_bar(decoder_table, B, T):
    """What the file is about: today's whole-waveform bar lets every planted bug through."""
    r = decoder_table[(B, T)]
    for name, (_, snr) in r["bugs"].items():
        assert snr >= SNR_BAR, (name, snr)


@pytest.mark.parametrize("B,T", SHAPES)
def test_decoder_floor_holds_across_seeds(decoder_table, B, T):
    r = decoder_table[(B, T)]
    assert 1 / SEED_RATIO <= r["seed2"][W_DEC] <= SEED_RATIO, r["seed2"]


@pytest.fixture(scope="module")
def encoder_table(enc_sd):
    rows = {}
    for B, n in ENC_SHAPES:
        wav, wav2 = _wav(B, n, 7), _wav(B, n, 8)
        ref, ref2 = orc.facodec_encode(enc_sd, wav), orc.facodec_encode(enc_sd, wav2)
        floor, floor2 = emulated_encode(enc_sd, wav), emulated_encode(enc_sd, wav2)
        f = frame_errors(floor, ref)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            auto = orc.facodec_encode(enc_sd, wav).float()
        r = {"floor": float(f.max()), "flat": float(f.max() / f.median()),
             "seed2": float(frame_errors(floor2, ref2).max() / f.max()),
             "floor_rel": rel_l2(floor, ref), "bar_rel": 1.122 * max(rel_l2(auto, ref), 1e-3), "bugs": {}}
        bugs = {
            "(f) stride-4 conv (stage 2) reads across the utterance edge": bug_stride_leak("block.2.block.4"),
            "(f) the same in the stride-5 conv of stage 3": bug_stride_leak("block.3.block.4"),
            "(h) utterance edge leak, dil-1, stage 4": bug_edge_leak("block.4.block.0.block.1"),
            "(f) the same in the stride-2 conv of stage 1, recorded": bug_stride_leak("block.1.block.4"),
        }
        if n >= 1000:
            bugs["(g) dil-9 tap lost, stage 3, recorded"] = bug_lost_tap("block.3.block.2.block.1", 1)
        for name, mut in bugs.items():
            out = emulated_encode(enc_sd, wav, mutate=mut)
            assert not torch.equal(out, floor), name
            r["bugs"][name] = (float(frame_errors(out, ref).max()) / r["floor"], rel_l2(out, ref))
        rows[(B, n)] = r
        print(f"\nencoder ({B}, {n}): {ref.shape[2]} frames, floor frame max {r['floor']:.3e}, max/median {r['flat']:.2f}, "
              f"seed-2 ratio {r['seed2']:.2f}, floor rel-L2 {r['floor_rel']:.3e}, global bar (1.122 x autocast) {r['bar_rel']:.3e}")
        for name, (ratio, rel) in r["bugs"].items():
            print(f"  {name:60s} x floor {ratio:6.2f}   rel-L2 {rel:.3e}")
    return rows


@pytest.mark.parametrize("B,n", ENC_SHAPES)
def test_encoder_bugs_stand_above_the_bar(encoder_table, B, n):
    r = encoder_table[(B, n)]
    asserted = {k: v for k, v in r["bugs"].items() if RECORDED not in k}
    assert len(asserted) == 3
    for name, (ratio, rel) in asserted.items():
        assert ratio >= MARGIN * FACTOR_ENC, (name, ratio)
    assert 1 / SEED_RATIO <= r["seed2"] <= SEED_RATIO


# ------------------------------------------------------------------------------------------------------------
# f32 bars: above the oracle's own reassociation noise, below the bugs the bf16 profile cannot see
# ------------------------------------------------------------------------------------------------------------

def _all_threads(fn):
    torch.set_num_threads(_NT)
    try:
        return fn()
    finally:
        torch.set_num_threads(1)


def test_f32_window_bar_between_noise_and_bugs(calm_sd):
    B, T = SHAPES[0]
    lat, spk = _inputs(B, T, 100 + T)
    ref = orc.facodec_decode(calm_sd, lat, spk)
    noise = float(window_errors(_all_threads(lambda: orc.facodec_decode(calm_sd, lat, spk)), ref, W_DEC).max())
    bugs = decoder_bugs(calm_sd, B)
    worst = {k: float(window_errors(emulated_decode(calm_sd, lat, spk, round=None, mutate=m), ref, W_DEC).max())
             for k, m in bugs.items()}
    print(f"\ndecoder fp32 ({B}, {T}): thread noise {noise:.2e}, bar {F32_WINDOW_BAR:.0e}, bugs on the fp32 oracle: "
          + "; ".join(f"{k[:3]} {v:.2e}" for k, v in worst.items()))
    assert noise <= F32_WINDOW_BAR / 5
    assert min(worst.values()) >= 10 * F32_WINDOW_BAR, worst


def test_f32_frame_bar_between_noise_and_bugs(enc_sd):
    B, n = ENC_SHAPES[1]
    wav = _wav(B, n, 7)
    ref = orc.facodec_encode(enc_sd, wav)
    noise = float(frame_errors(_all_threads(lambda: orc.facodec_encode(enc_sd, wav)), ref).max())
    bugs = {"(f) stage 1": bug_stride_leak("block.1.block.4"), "(f) stage 2": bug_stride_leak("block.2.block.4"),
            "(g)": bug_lost_tap("block.3.block.2.block.1", 1)}
    worst = {k: float(frame_errors(emulated_encode(enc_sd, wav, round=None, mutate=m), ref).max()) for k, m in bugs.items()}
    print(f"\nencoder fp32 ({B}, {n}): thread noise {noise:.2e}, bar {F32_FRAME_BAR:.0e}, bugs on the fp32 oracle: "
          + "; ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert noise <= F32_FRAME_BAR / 5
    assert min(worst.values()) >= 10 * F32_FRAME_BAR, worst
