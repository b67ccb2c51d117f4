"""GPU: the two-stage second-order solvers (midpoint a = 1/2, Heun a = 1, general a) of the denoiser solve,
flamed_den_solve_rk2 -- the persistent kernel's RK2 variants (flamed-tts_amd/csrc/persist.hip) and the graph of
launches (denoiser.hip: fp32 handles, large M, split chains, eager) -- against the formula composed from the
oracle's velocity (test_rk2_cpu.rk2_oracle).  The bars are the project's: bf16 solve rel-L2 < 6e-3 with
max|d| < 0.05, fp32 solve < 1e-4, persistent vs launch path < 4e-3.  nfe = 8 velocity evaluations throughout."""
import contextlib
import os

import pytest
import torch

from _common import rel_l2
from test_denoiser_gpu import _prob_gen
from test_rk2_cpu import STAGE, rk2_oracle, rk2_sample_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 256
NFE = 8
BF16_SOLVE, BF16_MAXABS, F32_SOLVE, VS_LAUNCH = 6e-3, 0.05, 1e-4, 4e-3


@contextlib.contextmanager
def knob(key, value, default):
    from flamed import _native as nat
    L = nat.lib()
    nat.check(L.flamed_tune(key.encode(), value), "flamed_tune")
    try:
        yield
    finally:
        nat.check(L.flamed_tune(key.encode(), default), "flamed_tune")


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")


@pytest.fixture(scope="module")
def pgf():
    return _prob_gen("f32")


def _inputs(seed, B, T, temp=0.3):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, T, C, generator=g)
    noise = torch.randn(B, T, C, generator=g)
    spk = torch.randn(B, C, generator=g)
    return noise * temp + cond, spk


def _solve(pg, x0, spk, a, nfe=NFE):
    nsteps = nfe // 2
    tb = torch.linspace(0, 1, nsteps + 1, device=DEV)[:-1]
    ts_eval = torch.stack((tb, tb + a * (1 / nsteps)), dim=1).reshape(-1)  # [t_0, t_0 + a dt, t_1, ...]
    with torch.inference_mode():
        return pg.denoiser.hip().solve_rk2(x0.to(DEV), ts_eval, spk.to(DEV), nsteps, a).cpu()


def _oracle(sd, x0, spk, a, utts=None):
    """One-utterance composed-oracle solves (equal lengths: no coupling between utterances)."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    utts = range(x0.shape[0]) if utts is None else utts
    return {u: rk2_oracle(sd, x0[u:u + 1], spk[u:u + 1], NFE, a) for u in utts}


def _runs(pg):
    if pg.denoiser.hip().handle is None:
        return 0
    runs, broken = pg.denoiser.hip().persist_info()
    assert not broken, "the handle gave up the persistent path (failed launches)"
    return runs


def _check_bf16(out, ref, what):
    e, amax = rel_l2(out, ref), float((out - ref).abs().max())
    print(f"{what}: vs composed oracle rel-L2 {e:.3e} max|d| {amax:.3e}")
    assert torch.isfinite(out).all()
    assert e < BF16_SOLVE and amax < BF16_MAXABS, what


@pytest.mark.parametrize("T", [16, 131, 257, 520])
@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_rk2_persistent_b1(pgb, solver, T):
    """One utterance on the persistent kernel's RK2 variant: T = 16 (seven row groups empty), 131 / 257 (partial
    tiles, a tile edge), 520 (two chunks per group).  The solve is one persistent launch, matches the composed oracle
    at the bf16 bar and the graph of launches at 4e-3, and is bitwise deterministic."""
    pg, sd = pgb
    a = STAGE[solver]
    x0, spk = _inputs(1000 + T, 1, T)
    r0 = _runs(pg)
    out = _solve(pg, x0, spk, a)
    assert _runs(pg) == r0 + 1, "the B = 1 RK2 solve did not take the persistent path"
    again = _solve(pg, x0, spk, a)
    assert _runs(pg) == r0 + 2
    with knob("persist", 0, 1):
        launch = _solve(pg, x0, spk, a)
    assert _runs(pg) == r0 + 2
    _check_bf16(out, _oracle(sd, x0, spk, a)[0], f"persistent {solver} B=1 T={T}")
    el = rel_l2(out, launch)
    print(f"persistent {solver} B=1 T={T}: vs launch path {el:.3e}")
    assert el < VS_LAUNCH
    assert torch.equal(out, again)


@pytest.mark.parametrize("B,T", [(2, 37), (4, 100), (3, 100), (2, 400)])
def test_rk2_persistent_multi_utterance(pgb, B, T):
    """Several utterances in one persistent launch (B = 3 padded to 4; (2, 400) two chunks per group): every
    utterance against its own one-utterance composed-oracle solve."""
    pg, sd = pgb
    x0, spk = _inputs(2000 + 10 * B + T, B, T)
    r0 = _runs(pg)
    out = _solve(pg, x0, spk, 0.5)
    assert _runs(pg) == r0 + 1, "the multi-utterance RK2 solve did not take the persistent path"
    for u, ref in _oracle(sd, x0, spk, 0.5).items():
        _check_bf16(out[u:u + 1], ref, f"persistent midpoint B={B} T={T} utterance {u}")


@pytest.mark.parametrize("solver,T", [("heun", 1100), ("midpoint", 4000)])
def test_rk2_persistent_stashed_base(pgb, solver, T):
    """From three chunks per row group on, the kernel keeps the step's base x in a thread-private global stash instead
    of registers: T = 1100 is the first such shape (138 frames per group, three chunks), T = 4000 the largest variant
    (eight chunks).  Against the graph of launches at 4e-3, bitwise deterministic, and (T = 1100) against the oracle."""
    pg, sd = pgb
    a = STAGE[solver]
    x0, spk = _inputs(6000 + T, 1, T)
    r0 = _runs(pg)
    out = _solve(pg, x0, spk, a)
    again = _solve(pg, x0, spk, a)
    assert _runs(pg) == r0 + 2, "the many-chunk RK2 solve did not take the persistent path"
    with knob("persist", 0, 1):
        launch = _solve(pg, x0, spk, a)
    el = rel_l2(out, launch)
    print(f"persistent {solver} B=1 T={T} (stashed base): vs launch path {el:.3e}")
    assert torch.isfinite(out).all() and el < VS_LAUNCH and torch.equal(out, again)
    if T == 1100:
        _check_bf16(out, _oracle(sd, x0, spk, a)[0], f"persistent {solver} B=1 T={T}")


@pytest.mark.parametrize("a", [0.5, 1.0, 2 / 3], ids=["midpoint", "heun", "ralston"])
def test_rk2_f32_graph_small(pgf, a):
    """fp32 handle (graph of launches, small M), B = 2, T = 40: the sharp check on the coefficients."""
    pg, sd = pgf
    x0, spk = _inputs(3000, 2, 40)
    out = _solve(pg, x0, spk, a)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    e = rel_l2(out, rk2_oracle(sd, x0, spk, NFE, a))
    print(f"f32 graph path a={a:.4f} B=2 T=40: vs composed oracle rel-L2 {e:.3e}")
    assert e < F32_SOLVE


def test_rk2_fp8_handle():
    """An fp8 handle never takes the persistent solve and, below its MX-fp8 row threshold, runs the bf16 kernels
    of the graph of launches: B = 2, T = 40, Heun, at the bf16 bar."""
    pg, sd = _prob_gen("fp8")
    x0, spk = _inputs(3500, 2, 40)
    out = _solve(pg, x0, spk, 1.0)
    assert _runs(pg) == 0
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    _check_bf16(out, rk2_oracle(sd, x0, spk, NFE, 1.0), "fp8 handle heun B=2 T=40")


def test_rk2_large_m_launch_path(pgb):
    """bf16 graph of launches at 1,600 rows (>= big_min_rows), the persistent knob off: utterances 0 and 3."""
    pg, sd = pgb
    x0, spk = _inputs(4000, 4, 400)
    r0 = _runs(pg)
    with knob("persist", 0, 1):
        out = _solve(pg, x0, spk, 0.5)
    assert _runs(pg) == r0
    for u, ref in _oracle(sd, x0, spk, 0.5, utts=(0, 3)).items():
        _check_bf16(out[u:u + 1], ref, f"large-M launch path midpoint (4, 400) utterance {u}")


def test_rk2_split_chains_bitwise(pgb):
    """Two sub-batch chains (split_batch 2) give bitwise the single chain, at test_cfg2_split_batch_bitwise's
    smallest shape."""
    from flamed import _native as nat
    from test_configs_gpu import SPLIT_DEFAULT
    pg, _ = pgb
    x0, spk = _inputs(90 + 24, 24, 512)
    L = nat.lib()
    nat.check(L.flamed_tune(b"split_batch", 1), "flamed_tune")
    try:
        one = _solve(pg, x0, spk, 0.5)
        nat.check(L.flamed_tune(b"split_batch", 2), "flamed_tune")
        two = _solve(pg, x0, spk, 0.5)
    finally:
        nat.check(L.flamed_tune(b"split_batch", SPLIT_DEFAULT), "flamed_tune")
    assert torch.isfinite(one).all() and torch.equal(two, one)


def test_rk2_eager_vs_graph(pgf):
    """hip_graph False (plain launches) against the replayed graph: bitwise, B = 1, T = 40, fp32."""
    pg, _ = pgf
    x0, spk = _inputs(5000, 1, 40)
    graph = _solve(pg, x0, spk, 0.5)
    keep = pg.denoiser.hip_graph
    pg.denoiser.hip_graph = False
    try:
        eager = _solve(pg, x0, spk, 0.5)
    finally:
        pg.denoiser.hip_graph = keep
    assert keep and torch.isfinite(graph).all() and torch.equal(eager, graph)


def test_rk2_sample_ragged(pgb):
    """ProbGenerator.sample(solver="midpoint") on the masked ragged batch of test_sample_ragged_profile's smallest
    case (lengths 100 / 77 / 55 / 31 padded to 100)."""
    pg, sd = pgb
    lens = [100, 77, 55, 31]
    B, T, temp = len(lens), max(lens), 0.3
    g = torch.Generator().manual_seed(sum(lens))
    cond = torch.randn(B, 6, T, 384, generator=g)
    spk = torch.randn(B, C, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    torch.manual_seed(17)
    noise = torch.randn((B, T, C))  # the draw ProbGenerator.sample makes from the global CPU RNG
    torch.manual_seed(17)
    with torch.inference_mode():
        lat = pg.sample(cond.to(DEV), spk.to(DEV), mask.to(DEV), nfe=NFE, temperature=temp, solver="midpoint").cpu()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = rk2_sample_oracle(sd, cond, spk, mask, NFE, temp, noise, 0.5)
    assert lat.shape == (B, C, T)
    _check_bf16(lat, ref, f"ProbGenerator.sample midpoint, lens {lens}")
