"""GPU: exact lengths -- every utterance of a padded ragged batch solved (flamed_den_solve_lens / _rk2_lens) and folded
(flamed_cond_fold_exact) over its own frames only.  The reference of every check is the utterance ALONE: the oracle on
[:len_u] with a mask of ones, and the HIP solve of the slice.  2..8 utterances on a bf16 handle run as one launch of
the persistent kernel's exact-lengths variants (flamed-tts_amd/csrc/persist_rag.hip); everything else solves one
utterance after another on the launch path.

The bars are the project's (tests/test_rk2_gpu.py): bf16 solve rel-L2 < 6e-3 with max|d| < 0.05 against the oracle
(an utterance of <= 2 frames: the 2e-2 of test_denoiser_gpu.test_velocity_path_boundaries_bf16 -- GroupNorm over two
frames amplifies operand rounding), fp32 < 1e-4, persistent vs alone / launch path < 4e-3, condition fold 1e-5 (f32) and
8e-3 (bf16).  nfe = 8 velocity evaluations throughout."""
import os
import warnings

import pytest
import torch

from _common import orc, rel_l2
from test_denoiser_gpu import _prob_gen
from test_exact_lengths_cpu import alone_oracle
from test_rk2_cpu import STAGE, rk2_oracle
from test_rk2_gpu import BF16_MAXABS, BF16_SOLVE, F32_SOLVE, VS_LAUNCH, knob

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 256
NFE = 8
SHORT = 2e-2  # bf16 vs the oracle for an utterance of <= 2 frames
RAGGED = [[100, 77, 55, 31],      # the table of the design note
          [130, 129, 17, 64],     # one frame of padding, a tile edge, one more than the 16-frame tile
          [40, 33, 9, 2],         # shorter than the 15-frame halo, the minimum length, empty row groups
          [520, 300],             # B = 2, three chunks per group
          [64, 50, 33],           # B = 3 run as 4 (an idle utterance)
          [64, 61, 48, 33, 17, 16, 15, 9]]


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")


@pytest.fixture(scope="module")
def pgf():
    return _prob_gen("f32")


def _inputs(lens, temp=0.3):
    B, T = len(lens), max(lens)
    g = torch.Generator().manual_seed(7000 + sum(lens))
    cond = torch.randn(B, T, C, generator=g)
    noise = torch.randn(B, T, C, generator=g)
    spk = torch.randn(B, C, generator=g)
    return noise * temp + cond, spk


def _ts(a, nfe=NFE):
    if a is None:
        return torch.linspace(0, 1, nfe + 1, device=DEV)
    nsteps = nfe // 2
    tb = torch.linspace(0, 1, nsteps + 1, device=DEV)[:-1]
    return torch.stack((tb, tb + a * (1 / nsteps)), dim=1).reshape(-1)  # [t_0, t_0 + a dt, t_1, ...]


def _solve(pg, x0, spk, lens=None, a=None):
    h = pg.denoiser.hip()
    with torch.inference_mode():
        if a is None:
            return h.solve(x0.to(DEV), _ts(None), spk.to(DEV), NFE, lens=lens).cpu()
        return h.solve_rk2(x0.to(DEV), _ts(a), spk.to(DEV), NFE // 2, a, lens=lens).cpu()


def _state(pg):
    """(persistent launches, failed launches) of the handle; the handle must not have given the path up."""
    h = pg.denoiser.hip()
    if h.handle is None:
        return 0, 0
    runs, broken = h.persist_info()  # waits for the last launch
    assert not broken, "the handle gave up the persistent path (failed launches)"
    assert h.settle(block=True) == 0, "a persistent launch failed and was re-run"  # (synchronises the device)
    torch.cuda.synchronize()
    return runs, h.persist_status()[1]


_ORACLE = {}


def _oracle(sd, x0, spk, lens, a, utts=None):
    """Utterance u alone: the oracle's solve of x0[u, :len_u] (computed once per case and solver)."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    out = {}
    for u in range(len(lens)) if utts is None else utts:
        key = (tuple(lens), a, u)
        if key not in _ORACLE:
            xu, su = x0[u:u + 1, :lens[u]], spk[u:u + 1]
            _ORACLE[key] = orc.euler_solve(sd, xu, su, NFE) if a is None else rk2_oracle(sd, xu, su, NFE, a)
        out[u] = _ORACLE[key]
    return out


def _check_vs_oracle(out, ref, n, what, f32=False):
    e, amax = rel_l2(out, ref), float((out - ref).abs().max())
    print(f"{what}: vs the oracle alone rel-L2 {e:.3e} max|d| {amax:.3e}")
    assert torch.isfinite(out).all(), what
    if f32:
        assert e < F32_SOLVE, what
    elif n <= 2:
        assert e < SHORT, what
    else:
        assert e < BF16_SOLVE and amax < BF16_MAXABS, what


def _check_padding_zero(out, lens):
    for u, n in enumerate(lens):
        assert torch.count_nonzero(out[u, n:]) == 0, f"utterance {u}: padding rows not exactly 0"


@pytest.mark.parametrize("lens", RAGGED, ids=lambda v: "-".join(map(str, v)))
def test_ragged_persistent_euler(pgb, lens):
    """One persistent launch per solve, no failure; every utterance against the HIP solve of its slice alone (4e-3)
    and against the oracle alone; padding rows exactly 0; bitwise deterministic over two runs."""
    pg, sd = pgb
    x0, spk = _inputs(lens)
    r0, f0 = _state(pg)
    out = _solve(pg, x0, spk, lens)
    r1, f1 = _state(pg)
    assert (r1, f1) == (r0 + 1, f0), "the ragged solve was not exactly one persistent launch without a failure"
    again = _solve(pg, x0, spk, lens)
    assert _state(pg) == (r0 + 2, f0)
    assert out.shape == x0.shape and torch.equal(out, again)
    _check_padding_zero(out, lens)
    refs = _oracle(sd, x0, spk, lens, None)
    for u, n in enumerate(lens):
        alone = _solve(pg, x0[u:u + 1, :n], spk[u:u + 1])
        ea = rel_l2(out[u:u + 1, :n], alone)
        print(f"lens {lens} utterance {u} (len {n}): ragged launch vs the HIP solve alone rel-L2 {ea:.3e}")
        _check_vs_oracle(out[u:u + 1, :n], refs[u], n, f"lens {lens} utterance {u} (len {n})")
        assert ea < VS_LAUNCH, (lens, u, ea)


def test_padding_is_never_read(pgb):
    """NaN in every padding row of x0 gives bitwise the output of the run with zeros there: finite on the valid rows,
    no failed launch, no re-run."""
    pg, _ = pgb
    lens = RAGGED[0]
    x0, spk = _inputs(lens)
    zeros, nans = x0.clone(), x0.clone()
    for u, n in enumerate(lens):
        zeros[u, n:] = 0.0
        nans[u, n:] = float("nan")
    r0, f0 = _state(pg)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a re-run announces itself with a warning
        a = _solve(pg, zeros, spk, lens)
        b = _solve(pg, nans, spk, lens)
        assert _state(pg) == (r0 + 2, f0)
    assert torch.isfinite(b).all() and torch.equal(a, b)
    _check_padding_zero(b, lens)


def test_all_lengths_equal_is_the_dense_solve(pgb):
    pg, _ = pgb
    x0, spk = _inputs([100, 100, 100, 100])
    r0, f0 = _state(pg)
    dense = _solve(pg, x0, spk)
    exact = _solve(pg, x0, spk, [100] * 4)
    assert _state(pg) == (r0 + 2, f0)
    assert torch.isfinite(dense).all() and torch.equal(dense, exact)
    for a in (0.5, 1.0):
        assert torch.equal(_solve(pg, x0, spk, a=a), _solve(pg, x0, spk, [100] * 4, a=a))


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_ragged_persistent_rk2(pgb, solver):
    pg, sd = pgb
    lens, a = RAGGED[0], STAGE[solver]
    x0, spk = _inputs(lens)
    r0, f0 = _state(pg)
    out = _solve(pg, x0, spk, lens, a)
    assert _state(pg) == (r0 + 1, f0), "the ragged RK2 solve was not exactly one persistent launch without a failure"
    assert torch.equal(out, _solve(pg, x0, spk, lens, a))
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, a).items():
        n = lens[u]
        alone = _solve(pg, x0[u:u + 1, :n], spk[u:u + 1], a=a)
        ea = rel_l2(out[u:u + 1, :n], alone)
        print(f"{solver} lens {lens} utterance {u}: ragged launch vs the HIP solve alone rel-L2 {ea:.3e}")
        _check_vs_oracle(out[u:u + 1, :n], ref, n, f"{solver} lens {lens} utterance {u}")
        assert ea < VS_LAUNCH


def test_fallback_f32_handle(pgf):
    """An fp32 handle never takes the persistent solve: one utterance after another on the launch path."""
    pg, sd = pgf
    lens = RAGGED[2]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _state(pg)[0] == 0
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, None).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"f32 handle lens {lens} utterance {u}", f32=True)
    a = STAGE["midpoint"]
    out = _solve(pg, x0, spk, lens, a)
    for u, ref in _oracle(sd, x0, spk, lens, a).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"f32 handle midpoint lens {lens} utterance {u}", f32=True)


def test_fallback_persist_knob_off(pgb):
    pg, sd = pgb
    lens = RAGGED[2]
    x0, spk = _inputs(lens)
    r0, f0 = _state(pg)
    with knob("persist", 0, 1):
        out = _solve(pg, x0, spk, lens)
    assert _state(pg) == (r0, f0), "a persistent launch ran with the knob off"
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, None).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"persist 0 lens {lens} utterance {u}")
    ep = rel_l2(_solve(pg, x0, spk, lens)[0:1], out[0:1])
    print(f"lens {lens} utterance 0: ragged persistent launch vs the launch-path fallback rel-L2 {ep:.3e}")
    assert ep < VS_LAUNCH


def test_fallback_fp8_handle():
    pg, sd = _prob_gen("fp8")
    lens = RAGGED[2]
    x0, spk = _inputs(lens)
    out = _solve(pg, x0, spk, lens)
    assert _state(pg)[0] == 0
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, None).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"fp8 handle lens {lens} utterance {u}")


def test_fallback_more_than_eight_utterances(pgb):
    """B = 12 cannot run as one persistent launch: no multi-utterance launch is claimed, and utterance 0, the
    shortest and the longest match the oracle alone."""
    pg, sd = pgb
    lens = [33, 9, 60, 17, 48, 25, 12, 55, 40, 21, 30, 16]
    x0, spk = _inputs(lens)
    r0, f0 = _state(pg)
    out = _solve(pg, x0, spk, lens)
    assert _state(pg) == (r0, f0), "B = 12 claimed a persistent launch"
    _check_padding_zero(out, lens)
    for u, ref in _oracle(sd, x0, spk, lens, None, utts=(0, 1, 2)).items():
        _check_vs_oracle(out[u:u + 1, :lens[u]], ref, lens[u], f"B = 12 utterance {u} (len {lens[u]})")


@pytest.mark.parametrize("lens", [[48, 33], [17, 2]], ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("mode,tol", [("f32", 1e-5), ("bf16", 8e-3)])
def test_cond_fold_exact(pgf, mode, tol, lens):
    pg, sd = pgf
    B, T = len(lens), max(lens)
    cond = torch.randn(B, 6, T, 384, generator=torch.Generator().manual_seed(sum(lens)))
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    pg.cond_hip_dtype = mode
    try:
        with torch.inference_mode():
            cf = pg.fold_condition(cond.to(DEV), mask.to(DEV), exact=True).cpu()
    finally:
        pg.cond_hip_dtype = "f32"
    assert cf.shape == (B, T, C)
    for u, n in enumerate(lens):
        assert torch.count_nonzero(cf[u, n:]) == 0
        e = rel_l2(cf[u:u + 1, :n], orc.cond_fold(sd, cond[u:u + 1, :, :n], torch.ones(1, n, 1, dtype=torch.bool)))
        print(f"cond fold exact {mode} lens {lens} utterance {u}: vs the oracle alone rel-L2 {e:.3e}")
        assert e < tol


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_sample_exact_lengths(pgb, solver):
    """ProbGenerator.sample(exact_lengths=True): fold + noise + solve, against the composed oracle alone."""
    pg, sd = pgb
    lens = RAGGED[0]
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
    assert _state(pg) == (r0 + 1, f0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = alone_oracle(sd, cond, spk, noise, lens, NFE, temp, None if solver == "euler" else STAGE[solver])
    assert lat.shape == (B, C, T)
    for u, n in enumerate(lens):
        assert torch.count_nonzero(lat[u, :, n:]) == 0
        _check_vs_oracle(lat[u, :, :n], ref[u, :, :n], n, f"sample(exact_lengths) {solver} utterance {u} (len {n})")
