"""CPU calibration of the per-frame error profile (tests/_rowprofile.py).

  * the emulation with round = identity is the pinned oracle, bitwise (it cannot drift from it);
  * the floor is a property of the arithmetic, not of the input: the bf16 emulation on a second input seed stays
    inside 2 x the first seed's floor, also at small T where GroupNorm over few frames amplifies rounding;
  * seven planted single-site bugs on top of the bf16 emulation are each rejected with a row max of at least
    2 x the bar (4 x the floor) -- while most of them pass the global rel-L2 bar the GPU tests used alone.
"""
import pytest
import torch

from _common import orc, rel_l2, seeded
from _rowprofile import (assert_row_profile, bf16_round, emulated_forward, emulated_solve, row_errors, row_profile)

C = 256
BF16_VEL, BF16_SOLVE = 8e-3, 6e-3  # the global bars of the GPU tests (tests/test_denoiser_gpu.py)


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    return seeded("prob_generator")


def _solve_inputs(seed, B, T, temp=0.3):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, T, C, generator=g)
    noise = torch.randn(B, T, C, generator=g)
    spk = torch.randn(B, C, generator=g)
    return noise * temp + cond, spk


def _vel_inputs(seed, B, T):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, C, generator=g), torch.randn(B, C, generator=g)


def test_row_errors_definition():
    ref = torch.zeros(2, 3, 4)
    ref[..., 0] = 2.0                     # every frame norm 2 -> global RMS frame norm 2
    out = ref.clone()
    out[1, 2, 1] = 1.0                    # one frame off by 1
    e = row_errors(out, ref)
    assert e.dtype == torch.float64 and e.shape == (6,)
    assert torch.equal(e, torch.tensor([0, 0, 0, 0, 0, 0.5], dtype=torch.float64))


@pytest.mark.parametrize("per_frame_t", [False, True])
def test_identity_emulation_is_the_oracle_velocity(sd, per_frame_t):
    x, c = _vel_inputs(3, 3, 70)
    t = torch.rand(3, 70, generator=torch.Generator().manual_seed(4)) if per_frame_t else torch.tensor([[0.4]])
    assert torch.equal(emulated_forward(sd, x, t, c, round=None), orc.denoiser_forward(sd, x, t, c))
    seen = []
    emulated_forward(sd, x, t, c, round=None, mutate=lambda s, v, ctx: (seen.append((s, ctx["block"])), v)[1])
    assert seen == [("dw", 0), ("dw", 1), ("dw", 2), ("dw", 3), ("dw", 4), ("conv_out", 4)]


def test_identity_emulation_is_the_oracle_solve(sd):
    x0, spk = _solve_inputs(5, 1, 131)
    assert torch.equal(emulated_solve(sd, x0, spk, 4, round=None), orc.euler_solve(sd, x0, spk, 4))
    # a mutate hook that changes nothing changes nothing
    assert torch.equal(emulated_solve(sd, x0, spk, 4, round=None, mutate=lambda s, v, ctx: v),
                       orc.euler_solve(sd, x0, spk, 4))


@pytest.mark.parametrize("B,T,nfe", [(1, 400, 8), (3, 70, 0), (1, 17, 0), (2, 2, 0)])
def test_floor_holds_under_another_seed(sd, B, T, nfe):
    """nfe 0: one velocity.  The bar comes from seed 1's emulation against seed 1's oracle result; seed 2's
    emulation must pass it against seed 2's oracle result."""
    runs = []
    for seed in (1000 + T, 2000 + T):
        if nfe:
            x0, spk = _solve_inputs(seed, B, T)
            runs.append((emulated_solve(sd, x0, spk, nfe), orc.euler_solve(sd, x0, spk, nfe)))
        else:
            x, c = _vel_inputs(seed, B, T)
            t = torch.tensor([[0.35]])
            runs.append((emulated_forward(sd, x, t, c), orc.denoiser_forward(sd, x, t, c)))
    (f1, r1), (f2, r2) = runs
    assert_row_profile(f2, r2, f1, f"floor self-check B={B} T={T} nfe={nfe}", floor_ref=r1)


# ------------------------------------------------------------------------------------------------------------
# planted bugs: one site each, on top of the bf16 emulation
# ------------------------------------------------------------------------------------------------------------

def _lose_tap(y, ctx, frame, tap):
    """Depthwise output frame `frame` without the product of tap `tap` (k = 31: tap j reads frame + j)."""
    y = y.clone()
    y[:, :, frame] -= ctx["w"][:, 0, 15 + tap] * ctx["x"][:, :, frame + tap]
    return y


def bug_a(site, v, ctx):
    """depthwise tap -15 lost on frame 200 in ResBlock 2 only"""
    return _lose_tap(v, ctx, 200, -15) if site == "dw" and ctx["block"] == 2 else v


def bug_b(site, v, ctx):
    """depthwise tap -15 lost on frames 50, 100, ..., 350 in every block"""
    if site != "dw":
        return v
    for f in range(50, 400, 50):
        v = _lose_tap(v, ctx, f, -15)
    return v


def bug_c(site, v, ctx):
    """the last frame reads one stale row past T through tap +1 (the stale row: the conv input's own frame 0,
    a row of ordinary magnitude left behind where the zero padding should be), every block"""
    if site != "dw":
        return v
    v = v.clone()
    v[:, :, -1] += ctx["w"][:, 0, 16] * ctx["x"][:, :, 0]
    return v


def bug_d(site, v, ctx):
    """frame 0 of utterance 5 reads the last frame of utterance 4 through tap -1, block 0 only (a batch leak)"""
    if site != "dw" or ctx["block"] != 0:
        return v
    v = v.clone()
    v[5, :, 0] += ctx["w"][:, 0, 14] * ctx["x"][4, :, -1]
    return v


def bug_e(site, v, ctx):
    """conv_out tap -1 lost at frame 200"""
    if site != "conv_out":
        return v
    v = v.clone()
    v[:, :, 200] -= ctx["x"][:, :, 199] @ ctx["w"][:, :, 0].t()
    return v


def bug_f(site, v, ctx):
    """hidden columns 32..63 x frames 48..63 of ResBlock 1's depthwise output shifted by one frame"""
    if site != "dw" or ctx["block"] != 1:
        return v
    o = v.clone()
    o[:, 32:64, 48:64] = v[:, 32:64, 47:63]
    return o


def bug_g(site, v, ctx):
    """frame 200 skips the last Euler update"""
    if site != "euler" or ctx["step"] != ctx["nfe"] - 1:
        return v
    v = v.clone()
    v[:, 200] = ctx["prev"][:, 200]
    return v


@pytest.fixture(scope="module")
def solve_case(sd):
    x0, spk = _solve_inputs(1, 1, 400)
    return x0, spk, orc.euler_solve(sd, x0, spk, 8), emulated_solve(sd, x0, spk, 8)


@pytest.fixture(scope="module")
def vel_case(sd):
    x, c = _vel_inputs(6, 6, 100)
    t = torch.tensor([[0.35]])
    return x, t, c, orc.denoiser_forward(sd, x, t, c), emulated_forward(sd, x, t, c)


def _check_bug(name, bug, out, ref, floor, glob_bar, where):
    emax, fmax, arg, _ = row_profile(out, ref, floor)
    g = rel_l2(out, ref)
    print(f"planted bug ({name}) {bug.__doc__}: row max {emax:.3e} = {emax / fmax:.1f}x floor {fmax:.3e} at {arg}; "
          f"global rel-L2 {g:.3e} (floor {rel_l2(floor, ref):.3e}, global bar {glob_bar:g}: "
          f"{'passes' if g < glob_bar else 'fails'})")
    with pytest.raises(AssertionError, match="bf16 floor"):
        assert_row_profile(out, ref, floor, f"bug ({name})")
    assert emax >= 4 * fmax, f"bug ({name}) stands only {emax / fmax:.1f}x above the floor"
    assert arg in where, (arg, where)


@pytest.mark.parametrize("name,bug,frames", [
    ("a", bug_a, range(169, 232)), ("b", bug_b, range(19, 382)), ("c", bug_c, range(368, 400)),
    ("e", bug_e, range(169, 232)), ("f", bug_f, range(17, 95)), ("g", bug_g, [200])])
def test_planted_bug_rejected_solve(sd, solve_case, name, bug, frames):
    """(a) (b) (c) (e) (f) (g) on the (1, 400) 8-step solve.  The worst frame lies where the bug was planted (within
    31 frames, two depthwise reaches, of it)."""
    x0, spk, ref, floor = solve_case
    out = emulated_solve(sd, x0, spk, 8, mutate=bug)
    _check_bug(name, bug, out, ref, floor, BF16_SOLVE, [(0, f) for f in frames])


def test_planted_bug_rejected_velocity(sd, vel_case):
    """(d) on one velocity at (6, 100)."""
    x, t, c, ref, floor = vel_case
    out = emulated_forward(sd, x, t, c, mutate=bug_d)
    _check_bug("d", bug_d, out, ref, floor, BF16_VEL, [(5, f) for f in range(0, 31)])


def test_clean_emulation_passes_and_x16_rounds_more(sd, vel_case):
    """The floor passes its own bar trivially (ratio 1); the x16 option only adds rounding points."""
    x, t, c, ref, floor = vel_case
    assert assert_row_profile(floor, ref, floor, "floor vs itself") == 1.0
    f16 = emulated_forward(sd, x, t, c, x16=True)
    assert not torch.equal(f16, floor)
    assert rel_l2(f16, ref) < BF16_VEL
    assert torch.equal(bf16_round(torch.tensor([1.00390625, 1.01171875])), torch.tensor([1.0, 1.015625]))  # ties to even
