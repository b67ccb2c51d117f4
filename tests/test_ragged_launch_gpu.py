"""GPU: exact lengths at batch scale -- a ragged batch that the persistent kernel cannot take (B > 8, B x T > 4096, an
fp32 handle, knob persist 0) solved in ONE call on the launch path (flamed-tts_amd/csrc/denoiser.hip, den_solve_lens):
the (B, T) solve the dense range solver would run -- graph of launches, fused Euler steps, sub-batch chains, RK2 -- with
the depthwise conv + GroupNorm sub-block, the conv_out tap combine and the state update ended at every utterance's own
length.  The reference of every check is the utterance ALONE: the oracle on [:len_u], the HIP solve of the slice, and
the per-frame profile against the bf16 floor of the utterance alone (a wrong end touches about 15 frames, which a
global rel-L2 hides).

Bars (the project's): bf16 vs the oracle alone rel-L2 < 6e-3 with max|d| < 0.05 (2e-2 for an utterance of <= 2 frames),
fp32 < 1e-4, vs the HIP solve alone < 4e-3, row profile 2x the floor.  nfe = 8 evaluations (RK2: 4 steps), seeded
weights.  Shapes: the smallest that reach each step variant (SHAPES below)."""
import contextlib
import ctypes
import os

import pytest
import torch

from _common import rel_l2
from _rowprofile import assert_row_profile, emulated_solve
from test_exact_lengths_cpu import alone_oracle
from test_exact_lengths_gpu import (C, DEV, NFE, RAGGED, _check_padding_zero, _check_vs_oracle, _inputs, _oracle, _solve,
                                    _state, _ts, knob)
from test_denoiser_gpu import _prob_gen
from test_rk2_cpu import STAGE
from test_rk2_gpu import VS_LAUNCH

pytestmark = pytest.mark.gpu

SHAPES = {
    # tiny tiles, fused small-M step (LoadEulerIn), dwgn_small: M = 9 x 33 = 297
    "tiny": [33, 9, 2, 17, 31, 25, 12, 16, 15],
    # small M: 12 x 60 = 720
    "small": [33, 9, 60, 17, 48, 25, 12, 55, 40, 21, 30, 16],
    # large M, dwgn_kernel + euler_cast: 12 x 130 = 1560 >= 1536
    "large": [130, 129, 17, 64, 65, 2, 128, 100, 63, 31, 16, 115],
    # dwconv_stats + fused GroupNorm finalize, T > 576: 9 x 600 = 5400
    "stats": [600, 577, 513, 512, 449, 64, 65, 300, 2],
    # B <= 8 but B x T > 4096
    "long4": [1100, 1037, 512, 2],
}
# two sub-batch chains: 24 x 512 = 12,288 rows, 512 in each half, the shortest in the second
TWO_CHAINS = [100, 31, 257, 64, 448, 512, 17, 300, 65, 200, 16, 129,
              64, 385, 2, 150, 33, 512, 90, 260, 15, 128, 47, 300]


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")


@pytest.fixture(scope="module")
def pgf():
    return _prob_gen("f32")


def _path(pg):
    return pg.denoiser.hip().lens_path()


_FLOOR = {}


def _floor(sd, x0, spk, lens, u):
    """The bf16 emulation of utterance u alone (computed once per case)."""
    key = (tuple(lens), u)
    if key not in _FLOOR:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        _FLOOR[key] = emulated_solve(sd, x0[u:u + 1, :lens[u]], spk[u:u + 1], NFE)
    return _FLOOR[key]


def _check_utterances(pg, sd, x0, spk, lens, out, what, utts=None, a=None, profile=True):
    """Utterance by utterance: against the oracle alone, the HIP solve of the slice alone and (Euler) the per-frame
    profile against the bf16 floor of the utterance alone."""
    utts = list(range(len(lens))) if utts is None else list(utts)
    refs = _oracle(sd, x0, spk, lens, a, utts=utts)
    for u in utts:
        n = lens[u]
        label = f"{what} utterance {u} (len {n})"
        mine = out[u:u + 1, :n]
        _check_vs_oracle(mine, refs[u], n, label)
        alone = _solve(pg, x0[u:u + 1, :n], spk[u:u + 1], a=a)
        ea = rel_l2(mine, alone)
        print(f"{label}: ragged launch path vs the HIP solve alone rel-L2 {ea:.3e}")
        assert ea < VS_LAUNCH, (label, ea)
        if profile and a is None:
            assert_row_profile(mine, refs[u], _floor(sd, x0, spk, lens, u), label)


# ------------------------------------------------------------------------------------------------------------
# 1. which path ran
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES) + ["two_chains"])
def test_path_is_one_ragged_batch(pgb, name):
    """Every shape runs as one ragged batch on the launch path (2), never as a persistent launch."""
    pg, _ = pgb
    lens = TWO_CHAINS if name == "two_chains" else SHAPES[name]
    x0, spk = _inputs(lens)
    r0, f0 = _state(pg)
    out = _solve(pg, x0, spk, lens)
    assert _state(pg) == (r0, f0), "a persistent launch ran"
    assert _path(pg) == 2
    assert torch.isfinite(out).all()
    _check_padding_zero(out, lens)


def test_path_other_values(pgb):
    """ragged_launch 0: one utterance after another (3); a batch the persistent kernel takes: 1; equal lengths: 0."""
    pg, _ = pgb
    lens = SHAPES["tiny"]
    x0, spk = _inputs(lens)
    with knob("ragged_launch", 0, 1):
        loop = _solve(pg, x0, spk, lens)
        assert _path(pg) == 3
    one = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2
    e = rel_l2(one[0:1], loop[0:1])  # utterance 0 is the longest: the loop solved it at the same T
    print(f"lens {lens} utterance 0: ragged batch vs one utterance after another rel-L2 {e:.3e}")
    assert e < VS_LAUNCH
    r0, f0 = _state(pg)
    x1, s1 = _inputs(RAGGED[0])
    _solve(pg, x1, s1, RAGGED[0])
    assert _path(pg) == 1 and _state(pg) == (r0 + 1, f0)
    x2, s2 = _inputs([40] * 9)
    _solve(pg, x2, s2, [40] * 9)
    assert _path(pg) == 0


# ------------------------------------------------------------------------------------------------------------
# 2. parity, bf16
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "small", "large", "stats"])
def test_parity_bf16(pgb, name):
    pg, sd = pgb
    lens = SHAPES[name]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2
    again = _solve(pg, x0, spk, lens)
    assert out.shape == x0.shape and torch.equal(out, again), "two runs differ"
    _check_padding_zero(out, lens)
    _check_utterances(pg, sd, x0, spk, lens, out, f"{name} lens {lens}")


@pytest.mark.parametrize("name,knobs", [("small", {"dwgn_small": 0}), ("large", {"dwgn": 0}), ("large", {"dwgn_small": 0, "dwgn": 0})],
                         ids=["small-dwgn_small0", "large-dwgn0", "large-both0"])
def test_parity_bf16_chunk_edges(pgb, name, knobs):
    """The same shapes through dwconv_stats_kernel (+ fused finalize): lengths at and around its 64-frame chunks,
    workgroups whose chunk lies wholly behind an utterance's end."""
    pg, sd = pgb
    lens = SHAPES[name]
    x0, spk = _inputs(lens)
    with contextlib.ExitStack() as st:
        for k, v in knobs.items():
            st.enter_context(knob(k, v, 1))
        out = _solve(pg, x0, spk, lens)
        assert _path(pg) == 2
        assert torch.equal(out, _solve(pg, x0, spk, lens))
    _check_padding_zero(out, lens)
    refs = _oracle(sd, x0, spk, lens, None)
    for u, n in enumerate(lens):
        label = f"{name} {knobs} utterance {u} (len {n})"
        _check_vs_oracle(out[u:u + 1, :n], refs[u], n, label)
        assert_row_profile(out[u:u + 1, :n], refs[u], _floor(sd, x0, spk, lens, u), label)


def test_parity_long4(pgb):
    """B <= 8 but B x T > 4096: against the HIP solve of every slice alone."""
    pg, _ = pgb
    lens = SHAPES["long4"]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2
    _check_padding_zero(out, lens)
    for u, n in enumerate(lens):
        ea = rel_l2(out[u:u + 1, :n], _solve(pg, x0[u:u + 1, :n], spk[u:u + 1]))
        print(f"lens {lens} utterance {u}: ragged launch path vs the HIP solve alone rel-L2 {ea:.3e}")
        assert ea < VS_LAUNCH


def test_parity_two_chains(pgb):
    pg, sd = pgb
    lens = TWO_CHAINS
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2
    _check_padding_zero(out, lens)
    with knob("split_batch", 1, 2):
        single = _solve(pg, x0, spk, lens)
        assert _path(pg) == 2
    assert torch.equal(out, single), "split_batch 1 and 2 differ"
    shortest = min(range(len(lens)), key=lambda u: lens[u])
    _check_utterances(pg, sd, x0, spk, lens, out, "two chains", utts=sorted({0, 11, 12, 23, shortest}))


# ------------------------------------------------------------------------------------------------------------
# 3. parity, fp32 handle
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "small", "stats"])
def test_parity_f32(pgf, name):
    """fp32 < 1e-4 against the oracle alone: the tight check of the boundary logic; eager launches against the graph."""
    pg, sd = pgf
    lens = SHAPES[name]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2 and _state(pg)[0] == 0
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, None).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"f32 {name} utterance {u} (len {lens[u]})", f32=True)
    pg.denoiser.hip_graph = False
    try:
        eager = _solve(pg, x0, spk, lens)
        assert _path(pg) == 2
    finally:
        pg.denoiser.hip_graph = True
    assert torch.equal(out, eager), "use_graph 0 and 1 differ"


# ------------------------------------------------------------------------------------------------------------
# 4. RK2
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["midpoint", "heun"])
@pytest.mark.parametrize("name", ["small", "large"])
def test_rk2(pgb, name, solver):
    pg, sd = pgb
    lens, a = SHAPES[name], STAGE[solver]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens, a)
    assert _path(pg) == 2
    assert torch.equal(out, _solve(pg, x0, spk, lens, a))
    _check_padding_zero(out, lens)
    _check_utterances(pg, sd, x0, spk, lens, out, f"{solver} {name}", a=a)


# ------------------------------------------------------------------------------------------------------------
# 5. padding rows
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "large"])
def test_padding_never_influences(pgb, name):
    """NaN in every padding row of x0 gives bitwise the run with zeros there, finite on the valid rows."""
    pg, _ = pgb
    lens = SHAPES[name]
    x0, spk = _inputs(lens)
    zeros, nans = x0.clone(), x0.clone()
    for u, n in enumerate(lens):
        zeros[u, n:] = 0.0
        nans[u, n:] = float("nan")
    a = _solve(pg, zeros, spk, lens)
    b = _solve(pg, nans, spk, lens)
    assert _path(pg) == 2
    assert torch.isfinite(b).all() and torch.equal(a, b)
    for solver in ("midpoint",):
        assert torch.equal(_solve(pg, zeros, spk, lens, STAGE[solver]), _solve(pg, nans, spk, lens, STAGE[solver]))


@pytest.mark.parametrize("name,graph", [("small", 1), ("large", 1), ("small", 0), ("large", 0)])
def test_padding_never_written(pgb, name, graph):
    """Through the C call: a sentinel in the padding rows of xt is still there afterwards (Euler and midpoint)."""
    from flamed import _native as nat
    pg, _ = pgb
    h = pg.denoiser.hip()
    lens = SHAPES[name]
    B, T = len(lens), max(lens)
    x0, spk = _inputs(lens)
    h._ensure(torch.device(DEV))
    L = nat.lib()
    r = torch.arange(NFE * B, device=DEV)
    valid = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, :, None].expand(B, T, C)
    ws = torch.empty(L.flamed_den_workspace_size(h.handle, B, T), dtype=torch.uint8, device=DEV)
    cl = (ctypes.c_int * B)(*lens)
    for a in (None, STAGE["midpoint"]):
        mods = h.adaln(_ts(a)[:NFE], spk.to(DEV), (r // B).to(torch.int32), (r % B).to(torch.int32))
        x = torch.where(valid, x0, torch.full((), 12345.0)).to(DEV).contiguous()
        if a is None:
            rc = L.flamed_den_solve_lens(h.handle, nat.ptr(x), nat.ptr(mods), cl, NFE, B, T, nat.ptr(ws), ws.numel(), graph,
                                         nat.stream_ptr(torch.device(DEV)))
        else:
            rc = L.flamed_den_solve_rk2_lens(h.handle, nat.ptr(x), nat.ptr(mods), cl, NFE // 2, a, B, T, nat.ptr(ws), ws.numel(),
                                             graph, nat.stream_ptr(torch.device(DEV)))
        nat.check(rc, "flamed_den_solve_lens")
        assert h.lens_path() == 2
        x = x.cpu()
        assert torch.equal(x[~valid], torch.full_like(x[~valid], 12345.0)), "a padding row was written"
        assert torch.isfinite(x).all() and not torch.equal(x[valid], x0[valid])


# ------------------------------------------------------------------------------------------------------------
# 6. isolation
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,u", [("small", 4), ("large", 1), ("stats", 3)])
def test_isolation(pgb, name, u):
    """B, T and the longest utterance kept; every other utterance's contents and lengths changed: utterance u's rows
    are bitwise what they were."""
    pg, _ = pgb
    lens = list(SHAPES[name])
    T, longest = max(lens), lens.index(max(lens))
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    g = torch.Generator().manual_seed(99)
    x1, s1, lens1 = x0.clone(), spk.clone(), list(lens)
    for v in range(len(lens)):
        if v == u:
            continue
        x1[v] = torch.randn(T, C, generator=g)
        s1[v] = torch.randn(C, generator=g)
        if v != longest:
            lens1[v] = 2 + (lens[v] * 7 + 3 * v) % (T - 1)
    assert lens1[u] == lens[u] and max(lens1) == T and lens1 != lens
    other = _solve(pg, x1, s1, lens1)
    assert _path(pg) == 2
    assert torch.equal(out[u], other[u]), f"utterance {u} depends on its batch-mates"
    assert not torch.equal(out[longest], other[longest]) or u == longest


# ------------------------------------------------------------------------------------------------------------
# 7. the lengths are not in the graph
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "large"])
def test_lengths_not_in_graph(pgb, name):
    """Same handle, same buffers (one (B, T, nfe) key): solve(A), solve(A'), solve(A) replay the same graphs."""
    pg, _ = pgb
    lens = SHAPES[name]
    x0, spk = _inputs(lens)
    T, longest = max(lens), lens.index(max(lens))
    other = [n if u == longest else 2 + (n * 5 + u) % (T - 1) for u, n in enumerate(lens)]
    assert other != lens
    first = _solve(pg, x0, spk, lens)
    second = _solve(pg, x0, spk, other)
    third = _solve(pg, x0, spk, lens)
    assert _path(pg) == 2
    assert torch.equal(first, third)
    fresh, _ = _prob_gen("bf16")
    assert torch.equal(second, _solve(fresh, x0, spk, other))
    assert _path(fresh) == 2


# ------------------------------------------------------------------------------------------------------------
# 8. through the module
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_sample_exact_lengths_b12(pgb, solver):
    """ProbGenerator.sample(exact_lengths=True) at B = 12: fold + noise + solve against the composed oracle alone."""
    pg, sd = pgb
    lens = SHAPES["small"]
    B, T, temp = len(lens), max(lens), 0.3
    g = torch.Generator().manual_seed(sum(lens))
    cond = torch.randn(B, 6, T, 384, generator=g)
    spk = torch.randn(B, C, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    torch.manual_seed(17)
    noise = torch.randn((B, T, C))  # the draw ProbGenerator.sample makes from the global CPU RNG
    torch.manual_seed(17)
    r0, f0 = _state(pg)
    with torch.inference_mode():
        lat = pg.sample(cond.to(DEV), spk.to(DEV), mask.to(DEV), nfe=NFE, temperature=temp, solver=solver,
                        exact_lengths=True).cpu()
    assert _state(pg) == (r0, f0) and _path(pg) == 2
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = alone_oracle(sd, cond, spk, noise, lens, NFE, temp, None if solver == "euler" else STAGE[solver])
    assert lat.shape == (B, C, T)
    for u, n in enumerate(lens):
        assert torch.count_nonzero(lat[u, :, n:]) == 0
        _check_vs_oracle(lat[u, :, :n], ref[u, :, :n], n, f"sample(exact_lengths) B = 12 {solver} utterance {u} (len {n})")
