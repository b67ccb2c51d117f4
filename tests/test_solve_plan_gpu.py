"""GPU: the knob paths and cache behaviour of the denoiser's range solver (flamed-tts_amd/csrc/denoiser.hip,
den_solve_range) that no other suite runs: every replay mode of the sub-batch chains, the keys of the solve-graph
cache, the in-graph timing entry point and a re-load of the weights on the same device.  Public knobs and entry points
only; every solve runs the graph of launches (knob persist 0).

Shapes: the chains at (4, 512) with big_rows = split_min_rows = 1024, both knobs' minima -- two chains of 1,024 rows is
the smallest split the library accepts and T = 512 is dwgn's limit; the cache and re-load at (2, 37) (fused small-M
steps); the timing graph at (2, 37) (ping-pong fused steps) and (4, 400) (in-place fused steps).  nfe = 8."""
import contextlib
import ctypes
import math

import pytest
import torch

from test_denoiser_gpu import _prob_gen
from test_exact_lengths_gpu import DEV, _ts
from test_rk2_cpu import STAGE

pytestmark = pytest.mark.gpu

NFE = 8
C = 256
N_CLASSES = 9  # FLAMED_DEN_KERNEL_CLASSES (include/flamed_hip.h)
# process knob defaults (csrc/common.hpp Tune)
DEFAULTS = {"persist": 1, "big_rows": 1536, "split_min_rows": 6144, "split_batch": 2, "split_prio": 2, "split_graph": 0,
            "prio_all": 0}


@contextlib.contextmanager
def knobs(**kv):
    """Process knobs set for the block; every one back at its default afterwards."""
    from flamed import _native as nat
    L = nat.lib()
    try:
        for k, v in kv.items():
            nat.check(L.flamed_tune(k.encode(), v), "flamed_tune")
        yield
    finally:
        for k in kv:
            nat.check(L.flamed_tune(k.encode(), DEFAULTS[k]), "flamed_tune")


def _inputs(B, T):
    g = torch.Generator().manual_seed(4000 + 100 * B + T)
    x0 = 0.3 * torch.randn(B, T, C, generator=g) + torch.randn(B, T, C, generator=g)
    return x0, torch.randn(B, C, generator=g)


def _solve(pg, x0, spk, nfe=NFE, a=None, lens=None):
    h = pg.denoiser.hip()
    with torch.inference_mode():
        if a is None:
            out = h.solve(x0.to(DEV), _ts(None, nfe), spk.to(DEV), nfe, lens=lens).cpu()
        else:
            out = h.solve_rk2(x0.to(DEV), _ts(a, nfe), spk.to(DEV), nfe // 2, a, lens=lens).cpu()
    assert h.persist_status()[0] == 0, "a persistent launch ran"
    return out


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")[0]


@pytest.fixture(scope="module")
def pgo():
    """A second module with the same weights: the source of handles that have never solved."""
    return _prob_gen("bf16")[0]


# ------------------------------------------------------------------------------------------------------------
# 1. chains under every replay mode
# ------------------------------------------------------------------------------------------------------------

MODES = {"prio0": {"split_batch": 2, "split_prio": 0}, "prio1": {"split_batch": 2, "split_prio": 1},
         "prio2": {"split_batch": 2, "split_prio": 2}, "branches": {"split_batch": 2, "split_graph": 1},
         "prio_all": {"split_batch": 1, "prio_all": 1}}
_CHAIN_REF = {}


def _ws_bytes(pg):
    """What the library asks as the solve workspace of the chains' shape under the current knobs: S chain workspaces
    when the solve splits -- each with the split-K slabs that only M < 2048 rows have -- or the one of the whole batch."""
    from flamed import _native as nat
    return nat.lib().flamed_den_workspace_size(pg.denoiser.hip().handle, 4, 512)


def _chain_ref(pg, a):
    """The single-chain solve (split_batch 1) of the chains' shape, once per solver, and its workspace size."""
    if a not in _CHAIN_REF:
        x0, spk = _inputs(4, 512)
        with knobs(persist=0, big_rows=1024, split_min_rows=1024, split_batch=1):
            out = _solve(pg, x0, spk, a=a)
            _CHAIN_REF[a] = (out, _ws_bytes(pg))
        assert torch.isfinite(out).all()
    return _CHAIN_REF[a]


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
@pytest.mark.parametrize("mode", list(MODES))
def test_chains_every_replay_mode(pgb, mode, solver):
    """Two chains of 1,024 rows (or one chain on a chain stream) equal the single chain on the caller's stream bitwise."""
    a = None if solver == "euler" else STAGE[solver]
    ref, ws_one = _chain_ref(pgb, a)
    x0, spk = _inputs(4, 512)
    with knobs(persist=0, big_rows=1024, split_min_rows=1024, **MODES[mode]):
        out = _solve(pgb, x0, spk, a=a)
        again = _solve(pgb, x0, spk, a=a)  # the replay of the cached graphs
        ws = _ws_bytes(pgb)
    # the solve did split: two chain workspaces (2 x 1,024 rows, with slabs) outgrow the single chain's (2,048 rows, none)
    assert (ws > ws_one) == (MODES[mode]["split_batch"] == 2), (mode, ws, ws_one)
    assert torch.isfinite(out).all()
    assert not torch.equal(out, x0)
    assert torch.equal(out, ref), f"{mode} {solver}: max|d| {float((out - ref).abs().max()):.3e}"
    assert torch.equal(again, ref)


# ------------------------------------------------------------------------------------------------------------
# 2. cache keys
# ------------------------------------------------------------------------------------------------------------

def test_cache_keys(pgb, pgo):
    """One handle through a sequence of solves that each change one part of the graph cache's key (or none): every
    result is bitwise what a handle without a cached graph gives for the same call."""
    x0, spk = _inputs(2, 37)
    x1 = x0.flip(0).contiguous()
    mid = STAGE["midpoint"]
    calls = [("first", dict(x0=x0)), ("replay", dict(x0=x0)), ("fresh xt", dict(x0=x1, fresh=True)), ("nfe 4", dict(x0=x0, nfe=4)),
             ("rk2", dict(x0=x0, a=mid)), ("lens", dict(x0=x0, lens=[37, 20])), ("first again", dict(x0=x0))]
    with knobs(persist=0):
        h = pgb.denoiser.hip()
        held = []
        for what, kw in calls:
            kw = dict(kw)
            if kw.pop("fresh", False):  # new state / table tensors under the same (B, T, nfe), the old ones still allocated
                held.append(h._solve_bufs)
                h._solve_bufs = {}
            got = _solve(pgb, spk=spk, **kw)
            if "lens" in kw:
                assert h.lens_path() == 2
            pgo.denoiser._hip = None  # the next call creates a new DenoiserHIP: a handle with no cached graph
            want = _solve(pgo, spk=spk, **kw)
            assert torch.isfinite(got).all()
            assert torch.equal(got, want), f"{what}: max|d| {float((got - want).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------------------
# 3. the timing entry point
# ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", [(2, 37), (4, 400)])
def test_time_kernels_graph(pgb, B, T):
    from flamed import _native as nat
    L = nat.lib()
    x0, spk = _inputs(B, T)
    dev = torch.device(DEV)
    with knobs(persist=0):
        before = _solve(pgb, x0, spk)
        h = pgb.denoiser.hip()
        with torch.inference_mode():
            ts = _ts(None)
            mods = h.adaln(ts[:1], spk.to(dev), torch.zeros(B, dtype=torch.int32, device=dev),
                           torch.arange(B, dtype=torch.int32, device=dev))
            ws = nat.Workspace().get(L.flamed_den_workspace_size(h.handle, B, T), dev)
            ms = (ctypes.c_float * (N_CLASSES + 1))()
            xs = x0.to(dev).clone()
            rc = L.flamed_den_time_kernels_graph(h.handle, nat.ptr(xs), nat.ptr(mods), B, T, nat.ptr(ws), ws.numel(), 2, ms,
                                                 nat.stream_ptr(dev))
            torch.cuda.synchronize()
        nat.check(rc, "flamed_den_time_kernels_graph")
        assert rc == 0
        vals = [float(v) for v in ms]
        print(f"({B}, {T}) in-graph ms per launch of classes 0..{N_CLASSES - 1}, whole step: {vals}")
        assert all(math.isfinite(v) and v >= 0.0 for v in vals), vals
        assert vals[N_CLASSES] > 0.0
        after = _solve(pgb, x0, spk)  # dup_class is back at its default: no launch runs twice
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------------------
# 4. re-load on the same device
# ------------------------------------------------------------------------------------------------------------

def test_reload_same_device():
    """flamed_den_load again on a handle with cached graphs (load_state_dict, then hip_invalidate): the next solve
    captures afresh against the re-packed weights and gives the first result."""
    pg, sd = _prob_gen("bf16")
    x0, spk = _inputs(2, 37)
    with knobs(persist=0):
        first = _solve(pg, x0, spk)
        h = pg.denoiser.hip()
        handle = h.handle.value
        pg.load_state_dict({k[len("prob_generator."):]: v for k, v in sd.items()})
        assert h._sig is None  # the next call packs the weights again
        second = _solve(pg, x0, spk)
        pg.denoiser.hip_invalidate()
        assert h._sig is None
        third = _solve(pg, x0, spk)
    assert pg.denoiser.hip() is h and h.handle.value == handle, "the handle was replaced, not re-loaded"
    assert torch.isfinite(first).all()
    assert torch.equal(second, first) and torch.equal(third, first)
