"""Shared pieces of the exact-lengths FaCodec decode tests (test_facodec_lens_cpu.py, test_facodec_lens_gpu.py).

The definition under test: utterance u of a padded batch, decoded with lens, is what it would be alone --

    wav[u, :, :200 len_u] = decode(lat[u:u+1, :, :len_u], spk[u:u+1])        wav[u, :, 200 len_u:] = 0 exactly

so the reference of utterance u is always orc.facodec_decode on that slice and the bf16 floor is
_codecprofile.emulated_decode on the same slice; both are computed once per (shape, lengths, seed) and shared.  The
bars are those of test_facodec_gpu._check, restated: f32 max |d| < 5e-3 and worst 25-sample window <= F32_WINDOW_BAR;
bf16 assert_window_profile (1.4 x the emulation's worst window, no window exempt; 200 len is always a multiple of
W_DEC) and whole-signal SNR >= the emulation's - 1 dB.  Calm weights throughout (weight-norm gains x the
`facodec_calm` gain): with unit gains the decoder saturates its tanh and a floor means nothing."""
import math

import numpy as np
import torch

from _common import golden, seeded, orc
from _codecprofile import emulated_decode, window_errors, assert_window_profile, W_DEC, F32_WINDOW_BAR

HOP = 200
F32_BAR = 5e-3  # SURVEY.md 8(c), as test_facodec_gpu

# (B, T, lens): what each shape puts where (stage lengths T x {1, 5, 25, 100, 200})
SHAPES = [
    (3, 13, (13, 7, 2)),    # n = 65 (one act1d tile + 1); ends at 1,400 and 400 samples inside fac_out and act1d tiles; len 2
                            # shorter than the dilation-9 reach below n = 100; ends inside 32- and 64-row GEMM tiles
    (2, 32, (32, 19)),      # the dense tile-aligned shape with a ragged end inside every tile family
    (2, 32, (16, 32)),      # the end on a tile edge (3,200 = 25 x 128 fac_out, 1,600 = 25 x 64 act1d); short one first
    (4, 9, (9, 1, 5, 8)),   # len 1 replicates onto itself from both sides; len T - 1 the closest miss
    (3, 41, (41, 20, 3)),   # the 128-row config (24,600 rows at the last stage), ragged end deep inside the big tiles
]

_sd = {}
_cases = {}


def calm_sd():
    if "sd" not in _sd:
        from flamed.utils.seeded_init import scale_weight_norm_gains
        _sd["sd"] = scale_weight_norm_gains(seeded("facodec_decoder"), float(golden("facodec_calm")["gain"]))
    return _sd["sd"]


def make_decoder(dtype, device):
    """FACodecDecoder with the calm weights on `device` (hip_dtype = dtype)."""
    from flamed.models.facodec import FACodecDecoder
    d = FACodecDecoder(in_channels=256, upsample_initial_channel=1024, ngf=32, up_ratios=[5, 5, 4, 2],
                       vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=256, codebook_dim=8,
                       use_gr_x_timbre=True, use_gr_residual_f0=True, use_gr_residual_phone=True).eval()
    d.load_state_dict(calm_sd())
    d.hip_dtype = dtype
    return d.to(device)


def inputs(B, T, seed=0):
    gen = torch.Generator().manual_seed(1000 * B + T + 7919 * seed)
    return torch.randn(B, 256, T, generator=gen), torch.randn(B, 256, generator=gen)


def alone(lat, spk, lens):
    """Per utterance: (oracle, bf16 emulation) of its own slice decoded alone."""
    sd = calm_sd()
    return [(orc.facodec_decode(sd, lat[u:u + 1, :, :n], spk[u:u + 1]), emulated_decode(sd, lat[u:u + 1, :, :n], spk[u:u + 1]))
            for u, n in enumerate(lens)]


def case(B, T, lens, seed=0):
    """(lat, spk, [(oracle alone, emulation alone) per utterance]) of one seeded input; computed once, never changed.
    The padding frames of lat keep their random values."""
    key = (B, T, tuple(lens), seed)
    if key not in _cases:
        lat, spk = inputs(B, T, seed)
        _cases[key] = (lat, spk, alone(lat, spk, lens))
    return _cases[key]


def snr_db(x, ref):
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    return 10 * math.log10(np.sum(ref ** 2) / max(np.sum((x - ref) ** 2), 1e-30))


def check_utterance(mode, out, ref, floor, label):
    """out, ref, floor: (1, 1, 200 len).  The mode's bars; returns the figure it printed (f32 worst window, bf16
    HIP / floor ratio)."""
    out = torch.as_tensor(out)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{label}: non-finite output"
    if mode == "f32":
        d, w = float((out - ref).abs().max()), float(window_errors(out, ref, W_DEC).max())
        print(f"{label} f32: max|d| {d:.2e}, window max {w:.2e}")
        assert d < F32_BAR
        assert w <= F32_WINDOW_BAR
        return w
    ratio = assert_window_profile(out, ref, floor, f"{label} bf16")
    s, sf = snr_db(out, ref), snr_db(floor, ref)
    print(f"{label} bf16: SNR {s:.1f} dB, emulation {sf:.1f} dB")
    assert s >= sf - 1.0
    return ratio


def check_batch(mode, wav, lens, refs, label):
    """Every utterance of wav (B, 1, 200 T) against its own (oracle, floor) alone, and exact 0 behind its end."""
    wav = torch.as_tensor(wav)
    assert torch.isfinite(wav).all(), f"{label}: non-finite output"
    figs = []
    for u, n in enumerate(lens):
        ref, floor = refs[u]
        figs.append(check_utterance(mode, wav[u:u + 1, :, :HOP * n], ref, floor, f"{label} utterance {u} (len {n})"))
        tail = wav[u, :, HOP * n:]
        assert torch.count_nonzero(tail) == 0, f"{label}: utterance {u} has {int(torch.count_nonzero(tail))} non-zero samples past its end"
    return figs
