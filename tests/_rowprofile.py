"""Per-frame error profiles for the bf16 denoiser parity tests.

A global rel-L2 divides an error confined to a few frames by sqrt(frames): the space between the bf16
rounding floor (velocity 3.7e-3, 8-step solve 2.2e-3) and the global bars (8e-3 / 6e-3) hides a lost
depthwise tap, a stale row past T or a leak across an utterance edge.  The profile looks at every frame:

  row_errors(out, ref)       e[r] = ||out[r] - ref[r]|| / sqrt(mean_r' ||ref[r']||^2), float64, one value per frame
  emulated_forward / _solve  orc.denoiser_forward / orc.euler_solve restated from the oracle's own pieces with a
                             `round` hook on both operands (activation and weight) of proj_in, conv_2, conv_3,
                             mlp.0, mlp.2 and conv_out -- the GEMMs the HIP bf16 mode feeds with bf16 -- everything
                             else fp32.  round = identity gives the oracle bitwise (test_rowprofile_cpu.py).
  assert_row_profile         max(row_errors(out, ref)) <= 2 x max(row_errors(floor_out, ref)), floor_out being the
                             bf16 emulation on the same inputs (above 2,048 frames: on the first ceil(2048 / T)
                             utterances).  No frame is exempt.

Why 2x: the floor is flat over frames (max over median about 1.3), the weakest planted bug stands 12x above it,
so 2x leaves a factor 6 on the bug side and tolerates the kernels' other fp32 summation order and the slow growth
of a maximum over more frames than the emulated subset.

`mutate(site, value, ctx)` plants single-site bugs (CPU calibration only) at three sites:
  "dw"        depthwise-conv output (B, H, T); ctx: block (0..3 ResBlocks, 4 final layer), x (the conv input,
              (B, H, T)), w (H, 1, k), step
  "conv_out"  conv_out output (B, C, T); ctx: x (the rounded conv input (B, H, T)), w (rounded, (C, H, 3)), step
  "euler"     the updated state (B, T, C); ctx: step, nfe, prev (the state before the update)

Calibration (CPU, seeded weights, tests/test_rowprofile_cpu.py; (1, 400) 8-step solve unless stated):

  case (all on top of the bf16 emulation)                          row max    x floor   global rel-L2 (old bar)
  floor: bf16 emulation, 8-step solve                              2.57e-3    1.0       2.22e-3
  floor: bf16 emulation, velocity (6, 100)                         4.94e-3    1.0       3.79e-3
  (a) depthwise tap -15 lost on frame 200, ResBlock 2 only         3.17e-2    12.3      3.67e-3 (6e-3: passed)
  (b) the same in every block on frames 50, 100, ..., 350          7.83e-2    30.4      1.75e-2 (6e-3: failed)
  (c) last frame reads a stale row past T through tap +1           6.49e-2    25.2      5.46e-3 (6e-3: passed)
  (d) velocity (6, 100): frame 0 of utterance 5 reads the last
      frame of utterance 4 through tap -1, block 0 only            8.82e-2    17.9      7.02e-3 (8e-3: passed)
  (e) conv_out tap -1 lost at frame 200                            4.33e-1    168       2.33e-2 (6e-3: failed)
  (f) columns 32..63 x frames 48..63 of ResBlock 1's depthwise
      output shifted by one frame                                  4.02e-2    15.6      8.02e-3 (6e-3: failed)
  (g) frame 200 skips the last Euler update                        9.74e-2    37.8      5.35e-3 (6e-3: passed)
  floor under a second input seed against the first seed's floor: (1, 400) 8 steps 1.12, (3, 70) 0.99,
  (1, 17) 1.11, (2, 2) 1.15 (floor row max 1.3e-2 there: the bar adapts where GroupNorm over two frames amplifies
  rounding)

Measured HIP / floor row-max ratios on the MI355X per test family:

All 146 profiled results lie between 0.88 and 1.13 of the floor (bar 2): the emulation has the rounding points the
kernels have (the LayerNorm fold's bf16 x * alpha operand adds nothing visible), and no frame at a group, chunk,
tile or utterance edge stands out.  Notation: B x T, /p = row partition bit, x16 cases against the x16 floor.

  configs[1] 128 steps (test_persist_gpu / test_configs_gpu): 1.01 .. 1.02
      persistent configs[1] 128 steps 1.01; launch path configs[1] 128 steps 1.02; configs[1] bf16 128 steps
      1.01
  test_persist_lengths_vs_oracle: 0.96 .. 1.00
      16 0.99; 40 1.00; 131 0.99; 257 1.00; 512 0.96
  test_persist_multi_counter_groupnorm: 0.90 .. 1.06
      2x200/p0 1.05; 2x200/p2 1.06; 4x100/p0 0.97; 4x100/p2 0.97; 8x64/p0 0.90; 8x64/p2 0.90; 4x300/p0 0.99;
      4x300/p2 0.98
  test_persist_multi_utterance: 0.97 .. 1.03
      2x200 0.97; 4x100 0.99; 8x64 1.03; 2x37 1.01
  test_persist_padded_batch: 0.96 .. 1.02
      3x256 0.99; 3x100 1.02; 5x64 0.96; 6x100 0.99; 7x48 1.00
  test_persist_multi_chunk: 0.95 .. 1.01
      1x520 1.01; 1x1000 1.00; 1x2400 1.00; 2x400 0.98; 4x300 0.97; 2x1111 0.99; 1x3000 0.99; 4x800 0.98; 3x800
      0.99; 4x1024 0.99; 8x500 0.95
  test_persist_row_partition: 0.97 .. 1.04
      default 1x400 1.04; flipped 1x400 1.04; default 1x131 0.99; flipped 1x131 1.02; default 1x16 1.02; flipped
      1x16 1.02; default 2x37 1.00; flipped 2x37 1.03; default 1x1000 0.98; flipped 1x1000 0.99; default 2x400
      0.97; flipped 2x400 0.99
  test_persist_edge_profiles: 0.97 .. 1.03
      1x16/p0 1.02; 1x16/p2 1.01; 1x33/p0 1.03; 1x33/p2 1.02; 1x97/p0 1.00; 1x97/p2 0.99; 1x120/p0 1.01;
      1x120/p2 1.01; 1x121/p0 1.01; 1x121/p2 1.01; 1x127/p0 0.99; 1x127/p2 0.99; 1x128/p0 0.98; 1x128/p2 0.98;
      1x129/p0 1.01; 1x129/p2 1.00; 1x513/p0 1.03; 1x513/p2 1.00; 1x1025/p0 1.01; 1x1025/p2 1.00; 2x65/p0 0.98;
      2x65/p2 1.02; 4x17/p0 0.98; 4x17/p2 0.97; 4x129/p0 1.03; 4x129/p2 1.03; 8x16/p0 1.00; 8x16/p2 1.00;
      8x65/p0 1.00; 8x65/p2 1.00; 3x33/p0 1.03; 3x33/p2 1.03; 5x17/p0 1.03; 5x17/p2 1.03
  test_sample_ragged_profile: 0.99 .. 1.10
      lens [100, 77, 55, 31] persist=1 1.10; lens [100, 77, 55, 31] persist=0 1.08; lens [400, 301, 207, 90]
      persist=0 0.99
  test_prob_sample_golden[bf16]: 1.04
  test_split_k_solve_bf16: 1.02 .. 1.02
      target 512 max 2 1.02; target 1024 max 4 1.02
  test_velocity_large_m_bf16: 1.00 .. 1.05
      128x128 t/frame False 1.05; fused (big 0) t/frame False 1.00; 128x128 t/frame True 1.04; fused (big 0)
      t/frame True 1.03
  test_velocity_tuning_paths_bf16: 0.94 .. 1.07
      dma: 0, bn32: 0 1x200 1.00; dma: 1, bn32: 0 1x200 1.00; dma: 2, bn32: 0 1x200 1.00; dma: 0, bn32: 1 1x200
      0.96; dma: 2, bn32: 1 1x200 0.96; dma: 1, bn32: 1 3x1000 1.01; big_ns: 3 17x500 1.01; big: 1, dw_tc: 128
      17x500 1.01; dw_cg: 16 2x300 1.03; dw_cg32: 0 1x131 0.99; dma_ns: 8 1x400 1.02; dma_ns: 4, dma: 2 1x250
      1.01; lnfold: 0 1x400 1.02; lnfold: 0 17x500 1.07; lnfold: 0, big: 0 5x400 0.99; g8p_rows: 0 41x400 1.00;
      x16: 1 41x400 0.97; x16: 1, lnfold: 0 41x400 1.05; x16: 1 5x400 0.96; dwgn: 0 41x400 1.02; dwgn: 0, x16: 1
      41x400 1.03; dwgn: 1 30x64 1.05; dwgn: 1 12x130 0.98; dwgn: 1 4x512 1.01; dwgn: 1 4x513 0.97; dwgn: 1,
      x16: 1 7x333 0.97; dwgn_small: 0 1x400 1.02; dwgn_small: 0 2x300 1.03; dwgn_small: 1 1x577 0.99;
      dwgn_small: 1 1x449 0.94; dwgn_small: 1 3x130 1.05; dwgn_small: 1 1x64 0.95; dwgn_small: 1, lnfold: 0
      1x250 1.03
  test_velocity_path_boundaries_bf16: 0.88 .. 1.13
      2x1 0.94; 1x2 1.13; 1x17 0.88; 1x319 1.02; 1x320 1.01; 2x160 1.01; 1x1535 1.01; 1x1536 1.00; 3x512 1.01;
      4x1536 1.05; 1x6144 0.99
  test_launch_edge_profiles: 0.96 .. 1.09
       5x333 1.06;  3x513 1.03;  13x100 0.98;  16x100 0.96; g8p_rows: 0 46x250 1.09; g8p_rows: 11500 46x250
      1.09;  2x130 1.03;  1x319 0.97;  1x9 0.97
  test_cfg2_velocity_full_size: 1.06
"""
import math

import torch
import torch.nn.functional as F

from _common import orc

SUBSET_ROWS = 2048
FACTOR = 2.0


def bf16_round(x):
    """bf16 round-to-nearest-even of an fp32 tensor, kept as fp32."""
    return x.to(torch.bfloat16).float()


def _ident(x):
    return x


def row_errors(out, ref):
    """(B, T, C) x 2 -> (B*T,) float64: per-frame error norm over the global RMS frame norm of ref."""
    o = torch.as_tensor(out, dtype=torch.float64)
    r = torch.as_tensor(ref, dtype=torch.float64)
    assert o.shape == r.shape and o.dim() == 3, (o.shape, r.shape)
    C = o.shape[-1]
    num = torch.linalg.vector_norm((o - r).reshape(-1, C), dim=1)
    rms = torch.sqrt(r.reshape(-1, C).pow(2).sum(1).mean())
    return num / rms.clamp_min(1e-300)


# ------------------------------------------------------------------------------------------------------------
# the oracle restated with hooks (oracle/flamed_oracle.py: convnext, resblock, final_layer, denoiser_forward,
# euler_solve -- same torch calls on the same operands in the same order)
# ------------------------------------------------------------------------------------------------------------

def _lin_r(sd, p, x, rnd):
    return F.linear(rnd(x), rnd(sd[p + ".weight"]), sd.get(p + ".bias"))


def _convnext(sd, p, x, k, rnd, mutate, ctx, x16):
    H = x.shape[-1]
    h = x.transpose(1, -1)
    w = sd[p + ".conv_1.weight"]
    y = F.conv1d(h, w, sd[p + ".conv_1.bias"], padding=k // 2, groups=H)
    if mutate is not None:
        y = mutate("dw", y, dict(ctx, x=h, w=w))
    if x16:
        y = bf16_round(y)
    y = F.group_norm(y, H, sd[p + ".ln_1.weight"], sd[p + ".ln_1.bias"], 1e-5)
    y = F.conv1d(rnd(y), rnd(sd[p + ".conv_2.weight"]), sd[p + ".conv_2.bias"])
    y = F.gelu(y)
    y = F.conv1d(rnd(y), rnd(sd[p + ".conv_3.weight"]), sd[p + ".conv_3.bias"])
    return (h + y).transpose(1, -1)


def _resblock(sd, p, x, y, k, rnd, mutate, ctx, x16):
    xr = bf16_round if x16 else _ident
    m = orc._lin(sd, p + ".adaLN_modulation.1", F.silu(y))
    sh_c, sc_c, g_c, sh_m, sc_m, g_m = m.chunk(6, dim=-1)
    h = orc._layer_norm(x, sd[p + ".ln_conv.weight"], sd[p + ".ln_conv.bias"], 1e-6)
    x = xr(x + g_c * _convnext(sd, p + ".conv_in", h * (1 + sc_c) + sh_c, k, rnd, mutate, ctx, x16))
    h = orc._layer_norm(x, sd[p + ".ln_mlp.weight"], sd[p + ".ln_mlp.bias"], 1e-6)
    h = h * (1 + sc_m) + sh_m
    h = _lin_r(sd, p + ".mlp.2", F.silu(_lin_r(sd, p + ".mlp.0", h, rnd)), rnd)
    return xr(x + g_m * h)


def _final_layer(sd, p, x, y, k, rnd, mutate, ctx, x16):
    xr = bf16_round if x16 else _ident
    m = orc._lin(sd, p + ".adaLN_modulation.1", F.silu(y))
    sh_c, sc_c, g_c, sh_o, sc_o = m.chunk(5, dim=-1)
    h = orc._layer_norm(x, None, None, 1e-6)
    x = xr(x + g_c * _convnext(sd, p + ".conv_in", h * (1 + sc_c) + sh_c, k, rnd, mutate, ctx, x16))
    x = orc._layer_norm(x, None, None, 1e-6) * (1 + sc_o) + sh_o
    xin = rnd(x.transpose(1, -1))
    w = rnd(sd[p + ".conv_out.weight"])
    x = F.conv1d(xin, w, sd[p + ".conv_out.bias"], padding=1)
    if mutate is not None:
        x = mutate("conv_out", x, dict(ctx, x=xin, w=w))
    return x.transpose(1, -1)


def emulated_forward(sd, x, t, c, round=bf16_round, mutate=None, x16=False, step=0,
                     p="prob_generator.denoiser", n_blocks=4, k=31):
    """orc.denoiser_forward with `round` on both operands of the six GEMMs and `mutate` at the depthwise and
    conv_out outputs.  x16: the large-M bf16 residual stream (X rounded after proj_in and after each residual add,
    depthwise output rounded)."""
    rnd = _ident if round is None else round
    te = orc._lin(sd, p + ".time_embed.mlp.2", F.silu(orc._lin(sd, p + ".time_embed.mlp.0", orc.timestep_freq(t))))
    ce = orc._lin(sd, p + ".cond_embed", c)
    y = te + ce.unsqueeze(1)
    h = _lin_r(sd, p + ".proj_in", x, rnd)
    if x16:
        h = bf16_round(h)
    for i in range(n_blocks):
        h = _resblock(sd, f"{p}.res_blocks.{i}", h, y, k, rnd, mutate, {"block": i, "step": step}, x16)
    return _final_layer(sd, p + ".final_layer", h, y, k, rnd, mutate, {"block": n_blocks, "step": step}, x16)


def emulated_solve(sd, xt, spk, nfe, round=bf16_round, mutate=None, x16=False, n_blocks=4, k=31, steps=None):
    """orc.euler_solve over emulated_forward; `mutate` also sees the Euler update ("euler")."""
    ts = torch.linspace(0, 1, nfe + 1)
    dt = 1 / nfe
    for i in range(1, (steps if steps is not None else nfe) + 1):
        prev = xt
        xt = xt + dt * emulated_forward(sd, xt, ts[i - 1].unsqueeze(0).unsqueeze(1), spk, round, mutate, x16, i - 1,
                                        n_blocks=n_blocks, k=k)
        if mutate is not None:
            xt = mutate("euler", xt, {"step": i - 1, "nfe": nfe, "prev": prev})
    return xt


def emulated_prob_sample(sd, cond, spk, mask, nfe, temperature, noise, round=bf16_round):
    """orc.prob_sample with the solve emulated (the condition fold stays the oracle's fp32).  (B, T, C)."""
    xt = noise * temperature + orc.cond_fold(sd, cond, mask)
    return emulated_solve(sd, xt, spk, nfe, round)


# ------------------------------------------------------------------------------------------------------------
# the check
# ------------------------------------------------------------------------------------------------------------

def subset_utterances(B, T):
    """How many leading utterances the floor is computed on: all up to 2,048 frames, ceil(2048 / T) above."""
    return B if B * T <= SUBSET_ROWS else min(B, math.ceil(SUBSET_ROWS / T))


def row_profile(out, ref, floor_out, floor_ref=None):
    """(HIP row max, floor row max, argmax (utterance, frame), row_errors(out, ref)).  floor_out may cover only the
    first utterances of ref; floor_ref (default: the matching slice of ref) is what floor_out is measured against."""
    B, T, _ = ref.shape
    if floor_ref is None:
        floor_ref = ref[:floor_out.shape[0]]
    e = row_errors(out, ref)
    f = row_errors(floor_out, floor_ref)
    r = int(torch.argmax(e))
    return float(e.max()), float(f.max()), (r // T, r % T), e


def assert_row_profile(out, ref, floor_out, label, floor_ref=None):
    """No frame of `out` may stand further from `ref` than 2 x the worst frame of the bf16 emulation."""
    assert torch.isfinite(torch.as_tensor(out)).all(), f"{label}: non-finite output"
    emax, fmax, (u, t), e = row_profile(out, ref, floor_out, floor_ref)
    bar = FACTOR * fmax
    print(f"row profile {label}: HIP row max {emax:.3e}, floor row max {fmax:.3e}, ratio {emax / fmax:.2f}, "
          f"argmax (utterance {u}, frame {t}), median {float(e.median()):.3e}")
    assert emax <= bar, (f"{label}: frame {t} of utterance {u} is {emax:.3e} from the oracle, "
                         f"{emax / fmax:.2f}x the bf16 floor's worst frame {fmax:.3e} (bar {FACTOR:g}x)")
    return emax / fmax


def velocity_floor(sd, x, t, c, x16=False):
    """The bf16 emulation of one velocity on the floor subset of (x, t, c)."""
    B, T, _ = x.shape
    n = subset_utterances(B, T)
    tt = t if t.shape[0] == 1 else t[:n]
    return emulated_forward(sd, x[:n], tt, c[:n], x16=x16)


def solve_floor(sd, x0, spk, nfe, steps=None):
    """The bf16 emulation of a solve on the floor subset of (x0, spk)."""
    B, T, _ = x0.shape
    n = subset_utterances(B, T)
    return emulated_solve(sd, x0[:n], spk[:n], nfe, steps=steps)


_memo = {}


def memo(key, fn):
    """One expensive floor (the 128-step configs[1] emulation) shared by the test modules of one run."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]
