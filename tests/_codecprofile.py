"""Windowed error profiles for the bf16 FaCodec decoder / encoder parity tests.

The whole-waveform SNR bar of the bf16 decoder (30 dB) stands 7x in amplitude above the bf16 rounding floor
(47.5 dB): a tap lost at one sample, a leak across an utterance edge or a wrong replicate pad moves the SNR by
tenths of a dB.  The profile looks at every window of the waveform (every frame of the encoder output):

  window_errors(out, ref, W)  row_errors (tests/_rowprofile.py) over the waveform (B, 1, n) cut into windows of W
                              samples: ||out - ref|| per window over the RMS window norm of ref, float64
  frame_errors(out, ref)      row_errors over the encoder output transposed to (B, T', 256)
  emulated_decode / _encode   orc.facodec_decode / orc.facodec_encode restated from the oracle's own pieces
                              (activation1d, wn_weight, _lin) with a `round` hook where the bf16 kernels hold bf16
                              (facodec.hip):
                                decoder (fac_decode_impl<bf16>): the styled LayerNorm output h0 (LoadConvRows packs
                                it to DT), every Activation1d output (act1d_kernel stores OT = DT, the one feeding
                                fac_out_kernel included), every weight-normed conv / conv-transpose weight
                                (pack_conv_kernel<bf16> / pack_convt_kernel<bf16>) except the last Conv1d(-> 1, k7),
                                which fac_out_kernel reads in fp32.  timbre_linear (launch_gemm<float>), biases,
                                the residual stream X / Z and the activation maths stay fp32.
                                encoder (enc_impl<bf16>): enc_in_kernel fp32 throughout; every Activation1d output
                                and every later weight, the last k3 conv's included.
                              round = None or identity gives the oracle bitwise (test_codecprofile_cpu.py).
  assert_window_profile       max over all windows of `out` <= FACTOR_DEC x max over all windows of the bf16
                              emulation on the same inputs, W = W_DEC.  No window is exempt.
  assert_frame_profile        the same over the encoder's frames with FACTOR_ENC.

`mutate(site, value, ctx)` plants single-site bugs (CPU calibration only).  ctx["p"] is the state-dict prefix:
  "act1d"   every Activation1d output before rounding (B, C, n); ctx: x (its fp32 input)
  "conv7"   the output of every dilated k7 conv of a residual unit (B, C, n); ctx: x (rounded input), w (rounded,
            (C, C, 7)), dil
  "convt"   every conv-transpose output (B, C / 2, s n); ctx: x, w (rounded, (C, C / 2, 2 s)), s
  "stride"  every strided conv output of the encoder (B, 2 C, n'); ctx: x, w (rounded, (2 C, C, 2 s)), s

All profile tests use weight-norm gains x the `facodec_calm` gain (0.6): with the unit-gain seeded decoder weights
85-90 % of the samples saturate the tanh and a floor means nothing.

Calibration (CPU, one thread, tests/test_codecprofile_cpu.py; every bug on top of the bf16 emulation, in the last
utterance unless it names one; x floor = worst window of the bugged run / worst window of the emulation):

  decoder (3, 13) / (1, 41); floor SNR 47.4 / 47.3 dB      W = 5         W = 10        W = 25        W = 200     SNR dB
  floor worst window                                       9.8 / 9.6e-3  7.9 / 8.2e-3  6.7 / 6.7e-3  5.6 / 4.9e-3
  floor max / median over windows                          2.5 / 2.4     2.0 / 2.0     1.6 / 1.6     1.3 / 1.1
  floor of a second input seed / this floor                1.13 / 1.13   1.03 / 1.08   0.96 / 1.04   0.90 / 1.03
  (a) dil-9 k7 tap -3 lost at the middle sample,
      last block (model.4.block.4)                         6.4 / 4.9     5.6 / 4.1     4.3 / 3.1     2.1 / 2.3   46.8 / 46.8
  (a) the same in the first block (model.1.block.4)        4.9 / 6.0     5.9 / 6.5     6.4 / 7.0     4.6 / 6.1   44.5 / 43.7
  (b) sample 0 of utterance 1 reads the last sample of
      utterance 0 through tap -1, dil-1 conv of block 1    3.0 / -       2.8 / -       2.9 / -       1.9 / -     46.8 / -
  (c) zero pad instead of replicate pad at the last
      sample, the activation before block 3's convT        2.1 / 2.9     2.4 / 2.6     2.6 / 2.3     1.3 / 1.4   47.2 / 47.1
  (d) convT phase r = s - 1 of the last q that stores
      (o = 2 n - 2) keeps only the bias, last stage        21 / 22       19 / 19       15 / 15       6.4 / 7.3   43.0 / 43.1
  (e) samples 64..127 of one act1d output shifted by
      one sample, last block                               14 / 17       17 / 17       17 / 19       14 / 15     37.8 / 38.0
  recorded, not asserted -- the same bugs where they stay under the bf16 floor:
  (b) in the dil-1 conv of the last block                  1.7 / -       1.5 / -       1.2 / -       1.0 / -     47.4 / -
  (c) in an activation inside a residual unit (model.3.
      block.3.block.0; all 24 such sites: 0.9 .. 1.5)      1.0 / 1.0     1.0 / 1.0     1.0 / 1.0     1.0 / 1.0   47.4 / 47.3

  Every bug passes the 30 dB bar.  W = 10 with factor 2 (the first proposal) leaves (b) and (c) below 1.5 x the
  bar (2.4-2.8 < 3).  The weakest asserted bug is (c): 2.1 (W = 5), 2.4 (W = 10), 2.3 (W = 25); with all the CPU's
  threads, which changes every rounding decision of the emulation, 2.2 / 2.2 / 2.5.  W = 25 has the flattest floor
  (max / median 1.6) and the steadiest one (second seed 0.96-1.12 under either thread count), so W_DEC = 25; and
  FACTOR_DEC = 1.4 keeps (c) >= 1.5 x above the bar with 10 % to spare under either thread count (2.34 / 2.47
  against 2.1).  The floor side: the floor of a second seed is <= 1.12 of the first (<= 1.3 asked), and the worst
  window of six re-rounded runs of the emulation (inputs x (1 + 1e-6 noise): other rounding decisions, same
  oracle) is 1.00-1.17 of the floor at the seven GPU shapes.  What no bf16 check against an fp32 oracle can see is
  a one-sample pad bug inside a residual branch: its error (4e-4 .. 2e-3 per sample) is under the rounding noise
  of the window it falls in.  The f32 mode sees it: F32_WINDOW_BAR = 2e-5 (below), 100 x under that bug's 2.1e-3;
  the kernels' worst f32 window on the MI355X is 2e-6.

  encoder (3, 152) / (3, 2055), 1 / 10 frames per utterance           x floor          rel-L2 (1.122 x autocast bar)
  floor worst frame 1.63e-3 / 3.65e-3, max / median 1.02 / 1.07,
  second seed 1.01 / 1.00, floor rel-L2                                                1.6e-3 / 3.3e-3 (4.6e-3 / 1.1e-2)
  (f) output 0 of utterance 1 of the stride-4 conv (stage 2) reads
      the last sample of utterance 0 through the tap at i = -1        5.8 / 1.9        5.6e-3 / 3.7e-3
  (f) the same in the stride-5 conv of stage 3                        23 / 7.3         2.2e-2 / 7.9e-3
  (h) (b) in the dil-1 conv of stage 4                                8.7 / 2.9        8.2e-3 / 4.3e-3
  recorded: (f) in the stride-2 conv of stage 1                       1.7 / 1.0        2.1e-3 / 3.3e-3
  recorded: (a) in the dil-9 conv of stage 3                          - / 1.8          - / 3.7e-3

  One output frame sums 200 samples through every stage and is normalised by the RMS over all frames, which the
  interior frames dominate: a one-sample bug in an early stage at an utterance edge is 1.0-2.0 x the floor ((f):
  1.94 here, 2.00 with all threads, 1.9 at (2, 1001), 1.8 at (2, 8137)).  The floor is flat (max / median <= 1.2,
  second seed 0.97-1.02, re-rounded runs 0.93-1.05 at the five GPU shapes), so FACTOR_ENC = 1.2 holds: (f), the
  stage-3 (f) and (h) stand >= 1.5 x above the bar at both calibration shapes (1.94 against 1.8).  The f32 mode's
  frame bar F32_FRAME_BAR covers the stage-1 (f) and (g): 1.7e-3 and 5.3e-3 on the fp32 oracle against 1e-5.

Measured HIP / floor ratios on the MI355X (bars 1.4 decoder, 1.2 encoder), B x T or B x n:

  decoder, all 14: 0.77 .. 1.13
    test_decode_calm_golden 1x64 1.07; test_decode_calm_bench_length 1x400 1.10
    test_decode_edge_profiles: 1x1 1.07; 1x2 0.97; 2x1 0.77; 3x13 1.03; 2x32 1.04; 1x41 0.94; 5x7 1.13
    test_decode_batch_isolation, each utterance alone: 3x13 0.85, 1.10, 1.03; 2x32 1.04, 0.96
    (the HIP side is bitwise the same from run to run; the emulation's CPU convolutions sum in an order that
    depends on the threads they get, and its worst window moved by up to 10 % between two runs of the suite:
    1x64 0.97 / 1.07, 1x400 1.06 / 1.10, 3x13 1.06 / 1.03 -- inside the range either way)
    whole-signal SNR within -0.1 .. +1.0 dB of the emulation's (46.7-49.9 dB)
    f32 mode at the same shapes: max |d| 8.9e-8 .. 3.7e-7 (bar 5e-3), worst window 7.3e-7 .. 1.9e-6
  encoder, all 8: 0.95 .. 1.07
    test_encode_edge_profiles: 1x152 0.99; 3x152 0.96; 2x1001 1.00; 3x2055 1.06; 2x8137 1.01
    test_encode_batch_isolation, each utterance of 3x1001 alone: 1.07, 0.95, 1.02
    f32 mode: rel-L2 per utterance 4.4e-7 .. 9.8e-7 (bar 2e-5), worst frame 4.4e-7 .. 1.2e-6 (bar 1e-5)

No case comes near the bars: the emulation has the rounding points the kernels have, and no window at an act1d tile,
fac_out tile, GEMM tile, config switch or utterance edge stands out.  Batch neighbours and shape sequences are
bitwise.  The one finding was on the host side: flamed_enc_out_len gave 1 frame for every input shorter than 152
samples (int division truncating toward zero where Conv1d's floor gives 0), so a too-short input was encoded into
one frame instead of being refused; enc_stride_len now returns 0 there (out_len(151): 1 before, 0 after).
"""
import torch
import torch.nn.functional as F

from _common import orc
from _rowprofile import bf16_round, row_errors

W_DEC = 25         # decoder window, samples
FACTOR_DEC = 1.4   # decoder: worst HIP window <= FACTOR_DEC x worst window of the bf16 emulation
FACTOR_ENC = 1.2   # encoder: the same over output frames (B, T', 256)
# f32 mode, worst window (W_DEC) / worst frame.  The fp32 oracle run with 1 against 2, 3 and 8 threads
# (torch.set_num_threads) differs from itself by 0.5-1.2e-6 in its worst window (decoder, (1, 1) .. (1, 41)) and by
# 1.2-4.6e-7 in its worst frame (encoder, (1, 152) .. (2, 8137)): the reassociation of the few convolutions whose
# blocking depends on the thread count.  The kernels sum every GEMM (K up to 3,584) in another order and use the
# device's sinf / expf / tanhf, so the bars are 20 x the largest of those.  The pad bug the bf16 profile cannot see
# ((c) inside a residual unit) and the stage-1 (f) stand > 10 x above them (test_codecprofile_cpu.py).
F32_WINDOW_BAR = 2e-5
F32_FRAME_BAR = 1e-5

DEC_RATIOS = (5, 5, 4, 2)
ENC_RATIOS = (2, 4, 5, 5)


def _ident(x):
    return x


# ------------------------------------------------------------------------------------------------------------
# the oracle restated with hooks (oracle/flamed_oracle.py: residual_unit, decoder_block, facodec_decode,
# encoder_block, facodec_encode -- same torch calls on the same operands in the same order)
# ------------------------------------------------------------------------------------------------------------

def _act(sd, p, x, rnd, mutate):
    """Activation1d; the kernel stores it as the GEMM operand type (act1d_kernel: store_val<OT>)."""
    y = orc.activation1d(sd, p, x)
    if mutate is not None:
        y = mutate("act1d", y, {"p": p, "x": x})
    return rnd(y)


def _residual_unit(sd, p, x, dil, rnd, mutate):
    a = _act(sd, p + ".block.0", x, rnd, mutate)
    w = rnd(orc.wn_weight(sd, p + ".block.1"))
    y = F.conv1d(a, w, sd[p + ".block.1.bias"], padding=3 * dil, dilation=dil)
    if mutate is not None:
        y = mutate("conv7", y, {"p": p + ".block.1", "x": a, "w": w, "dil": dil})
    y = _act(sd, p + ".block.2", y, rnd, mutate)
    y = F.conv1d(y, rnd(orc.wn_weight(sd, p + ".block.3")), sd[p + ".block.3.bias"])
    return x + y


def emulated_decode(sd, lat, spk, round=bf16_round, mutate=None, up_ratios=DEC_RATIOS, p=""):
    """orc.facodec_decode with `round` where fac_decode_impl<bf16> holds bf16: the styled LayerNorm output
    (LoadConvRows packs h0 to DT), every Activation1d output (the last one included), every weight-normed
    weight but the last conv's (fac_out_kernel reads it fp32).  timbre_linear, biases, the residual stream and
    the activation maths stay fp32.  (B, 256, T) -> (B, 1, 200 T)."""
    rnd = _ident if round is None else round
    style = orc._lin(sd, p + "timbre_linear", spk).unsqueeze(2)
    gamma, beta = style.chunk(2, 1)
    h = F.layer_norm(lat.transpose(1, 2), (lat.shape[1],), None, None, 1e-5).transpose(1, 2)
    h = h * gamma + beta
    h = F.conv1d(rnd(h), rnd(orc.wn_weight(sd, p + "model.0")), sd[p + "model.0.bias"], padding=3)
    for i, s in enumerate(up_ratios):
        q = f"{p}model.{i + 1}"
        a = _act(sd, q + ".block.0", h, rnd, mutate)
        w = rnd(orc.wn_weight(sd, q + ".block.1"))
        h = F.conv_transpose1d(a, w, sd[q + ".block.1.bias"], stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
        if mutate is not None:
            h = mutate("convt", h, {"p": q + ".block.1", "x": a, "w": w, "s": s})
        for j, d in enumerate((1, 3, 9)):
            h = _residual_unit(sd, f"{q}.block.{j + 2}", h, d, rnd, mutate)
    n = len(up_ratios) + 1
    h = _act(sd, f"{p}model.{n}", h, rnd, mutate)
    h = F.conv1d(h, orc.wn_weight(sd, f"{p}model.{n + 1}"), sd[f"{p}model.{n + 1}.bias"], padding=3)
    return torch.tanh(h)


def emulated_encode(sd, wav, round=bf16_round, mutate=None, up_ratios=ENC_RATIOS, p=""):
    """orc.facodec_encode with `round` where enc_impl<bf16> holds bf16: every Activation1d output and every
    weight after conv_in (enc_in_kernel is fp32 throughout), the last k3 conv's included.
    (B, 1, n) -> (B, 256, T')."""
    rnd = _ident if round is None else round
    h = F.conv1d(wav, orc.wn_weight(sd, p + "block.0"), sd[p + "block.0.bias"], padding=3)
    for i, s in enumerate(up_ratios):
        q = f"{p}block.{i + 1}"
        for j, d in enumerate((1, 3, 9)):
            h = _residual_unit(sd, f"{q}.block.{j}", h, d, rnd, mutate)
        a = _act(sd, q + ".block.3", h, rnd, mutate)
        w = rnd(orc.wn_weight(sd, q + ".block.4"))
        h = F.conv1d(a, w, sd[q + ".block.4.bias"], stride=s, padding=s // 2 + s % 2)
        if mutate is not None:
            h = mutate("stride", h, {"p": q + ".block.4", "x": a, "w": w, "s": s})
    n = len(up_ratios) + 1
    h = _act(sd, f"{p}block.{n}", h, rnd, mutate)
    return F.conv1d(h, rnd(orc.wn_weight(sd, f"{p}block.{n + 1}")), sd[f"{p}block.{n + 1}.bias"], padding=1)


# ------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------

def window_errors(out, ref, W):
    """(B, 1, n) x 2 -> (B * n / W,) float64: row_errors over windows of W samples."""
    o = torch.as_tensor(out)
    r = torch.as_tensor(ref)
    assert o.shape == r.shape and o.dim() == 3 and o.shape[1] == 1 and o.shape[2] % W == 0, (o.shape, r.shape, W)
    B, _, n = o.shape
    return row_errors(o.reshape(B, n // W, W), r.reshape(B, n // W, W))


def frame_errors(out, ref):
    """Encoder output (B, 256, T') x 2 -> (B * T',) float64: row_errors over output frames."""
    return row_errors(torch.as_tensor(out).transpose(1, 2), torch.as_tensor(ref).transpose(1, 2))


def _assert_profile(e, f, per_utt, width, unit, label, factor):
    emax, fmax = float(e.max()), float(f.max())
    r = int(torch.argmax(e))
    u, s = r // per_utt, (r % per_utt) * width
    print(f"codec profile {label}: HIP {unit} max {emax:.3e}, floor {unit} max {fmax:.3e}, ratio {emax / fmax:.2f}, "
          f"argmax (utterance {u}, {'sample' if width > 1 else unit} {s}), median {float(e.median()):.3e}")
    assert emax <= factor * fmax, (f"{label}: {unit} at {s} of utterance {u} is {emax:.3e} from the oracle, "
                                   f"{emax / fmax:.2f}x the bf16 floor's worst {unit} {fmax:.3e} (bar {factor:g}x)")
    return emax / fmax


def assert_window_profile(out, ref, floor_out, label, W=W_DEC, factor=FACTOR_DEC):
    """No window of W samples of the waveform `out` may stand further from `ref` than factor x the worst window of
    the bf16 emulation `floor_out` on the same inputs.  No window is exempt."""
    assert torch.isfinite(torch.as_tensor(out)).all(), f"{label}: non-finite output"
    e, f = window_errors(out, ref, W), window_errors(floor_out, ref, W)
    return _assert_profile(e, f, torch.as_tensor(ref).shape[2] // W, W, "window", label, factor)


def assert_frame_profile(out, ref, floor_out, label, factor=FACTOR_ENC):
    """The same over the encoder's output frames."""
    assert torch.isfinite(torch.as_tensor(out)).all(), f"{label}: non-finite output"
    e, f = frame_errors(out, ref), frame_errors(floor_out, ref)
    return _assert_profile(e, f, torch.as_tensor(ref).shape[2], 1, "frame", label, factor)
