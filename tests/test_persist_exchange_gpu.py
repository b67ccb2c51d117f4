"""GPU: the persistent solve's Euler boundary exchange (flamed-tts_amd/csrc/persist.hip).  conv_out's two boundary
rows per workgroup (Y0 of its last frame, Y2 of its first, 8 channels each) travel to the same-slot workgroups of the
two neighbouring row groups as {tag, fp32} granules, tag = the launch's evaluation number; the reader sweeps the 16
granules it needs until their tags match, and the launch's reset prologue zeroes every tag.  The row statistics of the
mlp.0 / conv_out epilogues are combined after the MFMA loop from loads issued before it (one chunk per group).

The bars are test_persist_gpu.py's, imported: the launch-path bar (rel-L2 < 4e-3 against the graph of launches: same
bf16 operands, other fp32 order) and the oracle bar (rel-L2 < BF16_SOLVE against the fp32 oracle, each frame within
the bf16-emulation profile).  Seeded inputs as there, nfe 8 unless stated.
"""
import warnings

import pytest
import torch

from _common import orc, rel_l2
from _rowprofile import assert_row_profile, solve_floor
from test_persist_gpu import BF16_SOLVE, PERSIST_DEFAULT, _inputs, _runs, _solve, knob, pgb  # noqa: F401
from test_rk2_gpu import _solve as _solve_rk2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VS_LAUNCH = 4e-3  # test_persist_gpu.py: `el < 4e-3`
NFE = 8


def _persistent(pg, x0, spk, nfe=NFE, runs=1):
    r0 = _runs(pg)
    out = _solve(pg, x0, spk, nfe)
    assert _runs(pg) == r0 + runs, "the solve did not take the persistent path"
    assert torch.isfinite(out).all()
    return out


@pytest.mark.parametrize("part", [0, 2])
@pytest.mark.parametrize("T", [16, 17, 40, 131, 400])
def test_boundary_exchange_one_utterance(pgb, T, part):
    """One utterance under both row partitions (part = persist_opt bit 2 flipped).  T = 16: one tile, seven groups
    empty (no neighbour at all); 17: one row in a second tile; 40: three tiles spread over eight groups, so the
    nearest non-empty neighbours are not adjacent groups; 131: ragged last tile; 400: the headline shape."""
    pg, sd = pgb
    x0, spk = _inputs(900 + T, 1, T)
    with knob("persist_opt", PERSIST_DEFAULT ^ part, PERSIST_DEFAULT):
        out = _persistent(pg, x0, spk)
    with knob("persist", 0, 1):
        launch = _solve(pg, x0, spk, NFE)
    el = rel_l2(out, launch)
    print(f"boundary exchange T={T} part={part}: vs launch path {el:.3e}")
    assert el < VS_LAUNCH
    if T == 131:
        ref = orc.euler_solve(sd, x0, spk, NFE)
        e = rel_l2(out, ref)
        print(f"boundary exchange T={T} part={part}: vs oracle {e:.3e}")
        assert e < BF16_SOLVE
        assert_row_profile(out, ref, solve_floor(sd, x0, spk, NFE), f"boundary exchange T={T} part={part}")


EDGES = [(2, 37, 2), (4, 100, 4), (8, 64, 8), (3, 100, 4)]


@pytest.mark.parametrize("B,T,Bp", EDGES, ids=["2x37", "4x100", "8x64", "3x100-padded"])
def test_utterance_edges_alone_bitwise(pgb, B, T, Bp):
    """Every utterance of the batch equals, bitwise, the B = 1 persistent solve of that utterance alone, and the
    padded batch (3, 100) equals the first three utterances of the unpadded (4, 100) one.

    The solo solve runs in the row partition the utterance has inside the batch (flamed_tune persist_as = the batch
    size: the utterance owns 8 / B row groups, the other groups idle).  In the default solo partition (all 8 groups)
    the comparison is not bitwise, before the granule exchange or after it: the GroupNorm statistics are Chan-combined
    per row group, (4, 100) splits 100 frames as 48 + 52 and a solo solve as 6 x 16 + 4, so the sums round differently
    (measured on MI355X, identical with the previous kernel: utterance 0 of (4, 100) max|d| 5.13e-3, rel-L2 8.13e-4;
    of (8, 64) 5.71e-3, 8.39e-4 -- the size of the persistent-vs-launch-path difference; only (2, 37), three one-tile
    groups either way, is equal there).  Those figures are printed, not asserted."""
    pg, _ = pgb
    xp, spkp = _inputs(950 + 10 * Bp + T, Bp, T)
    x0, spk = xp[:B].clone(), spkp[:B].clone()
    out = _persistent(pg, x0, spk)
    if B != Bp:
        assert torch.equal(out, _persistent(pg, xp, spkp)[:B])
    for u in range(B):
        with knob("persist_as", Bp, 0):
            alone = _persistent(pg, x0[u:u + 1], spk[u:u + 1])
        assert torch.equal(out[u:u + 1], alone), f"utterance {u} of ({B}, {T})"
    wide = _persistent(pg, x0[:1], spk[:1])  # the default solo partition, for the record
    print(f"utterance 0 of ({B}, {T}) vs alone over all 8 row groups: max|d| {float((out[:1] - wide).abs().max()):.3e} "
          f"rel-L2 {rel_l2(out[:1], wide):.3e}")


@pytest.mark.parametrize("B,T,Bp", EDGES, ids=["2x37", "4x100", "8x64", "3x100-padded"])
def test_utterance_edges_do_not_leak(pgb, B, T, Bp):
    """Nothing crosses an utterance edge: utterance u of the batch is bitwise the same whatever the other utterances
    hold (the same row partition on both sides, so the comparison is exact by construction)."""
    pg, _ = pgb
    x0, spk = _inputs(950 + 10 * Bp + T, Bp, T)
    x0, spk = x0[:B].clone(), spk[:B].clone()
    out = _persistent(pg, x0, spk)
    x1, spk1 = _inputs(1950 + 10 * Bp + T, B, T)
    for u in {0, B // 2, B - 1}:
        x1u, spk1u = x1.clone(), spk1.clone()
        x1u[u], spk1u[u] = x0[u], spk[u]
        assert torch.equal(_persistent(pg, x1u, spk1u)[u], out[u]), f"utterance {u} of ({B}, {T})"


def test_exchange_two_chunks_euler(pgb):
    """(1, 1000): two 64-frame chunks per group (the multi-chunk kernel variant reads the boundary rows of both)."""
    pg, _ = pgb
    x0, spk = _inputs(971, 1, 1000)
    out = _persistent(pg, x0, spk)
    with knob("persist", 0, 1):
        launch = _solve(pg, x0, spk, NFE)
    el = rel_l2(out, launch)
    print(f"boundary exchange (1, 1000): vs launch path {el:.3e}")
    assert el < VS_LAUNCH


@pytest.mark.parametrize("B,T", [(1, 131), (2, 37)])
@pytest.mark.parametrize("a", [0.5, 1.0], ids=["midpoint", "heun"])
def test_exchange_rk2(pgb, a, B, T):
    """The two-stage solvers exchange twice per step (one tag per velocity evaluation): against the graph path's RK2."""
    pg, _ = pgb
    x0, spk = _inputs(980 + 10 * B + T, B, T)
    r0 = _runs(pg)
    out = _solve_rk2(pg, x0, spk, a, NFE)
    assert _runs(pg) == r0 + 1, "the RK2 solve did not take the persistent path"
    with knob("persist", 0, 1):
        launch = _solve_rk2(pg, x0, spk, a, NFE)
    assert _runs(pg) == r0 + 1
    el = rel_l2(out, launch)
    print(f"boundary exchange RK2 a={a} ({B}, {T}): vs launch path {el:.3e}")
    assert torch.isfinite(out).all() and el < VS_LAUNCH


def test_stale_tags(pgb):
    """Tags of an earlier launch never match: on one handle A, B, A at the same nfe (the same tag sequence each
    time), then a captured graph of the solve replayed three times with the input changed in between, each result
    bitwise that input's solve on a fresh handle."""
    from flamed.models.synthesizer.prob_generator import DenoiserHIP
    pg, _ = pgb
    T = 131
    (xa, spk), (xb, _) = _inputs(991, 1, T), _inputs(992, 1, T)
    ts = torch.linspace(0, 1, NFE + 1, device=DEV)
    sd_ = spk.to(DEV)
    with torch.inference_mode():
        fresh = [DenoiserHIP(pg.denoiser, "bf16") for _ in range(2)]
        ref = [f.solve(x.to(DEV), ts, sd_, NFE).clone() for f, x in zip(fresh, (xa, xb))]
        assert all(f.settle() == 0 for f in fresh)
        h = DenoiserHIP(pg.denoiser, "bf16")
        for k in (0, 1, 0):
            assert torch.equal(h.solve((xa, xb)[k].to(DEV), ts, sd_, NFE), ref[k]), f"eager solve of input {k}"
        assert h.settle() == 0
        xd = xa.to(DEV).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            h.solve(xd, ts, sd_, NFE)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        r0 = h.persist_info()[0]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = h.solve(xd, ts, sd_, NFE)
        assert h.persist_info()[0] == r0 + 1, "the captured solve did not take the persistent path"
        for k in (1, 0, 1):
            xd.copy_((xa, xb)[k].to(DEV))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, ref[k]), f"replay with input {k}"
    assert h.persist_fails() == 0


def test_abandon_path(pgb):
    """A launch abandoned at step 3 (flamed_tune persist_inject: every workgroup leaves before that step's first
    hand-off, some of them still short of the previous step's boundary rows) returns, is counted once, and the
    wrapper's re-run equals the launch path.  Nothing here waits for a poll to time out."""
    from flamed.models.synthesizer.prob_generator import DenoiserHIP
    pg, _ = pgb
    h = DenoiserHIP(pg.denoiser, "bf16")
    x0, spk = _inputs(995, 1, 131)
    ts = torch.linspace(0, 1, NFE + 1, device=DEV)
    with torch.inference_mode():
        with warnings.catch_warnings(record=True) as wl:
            warnings.simplefilter("always")
            with knob("persist_inject", 3, -1):
                out = h.solve(x0.to(DEV), ts, spk.to(DEV), NFE)
            assert h.settle() == 1 and not h._pending
        assert any("persistent solve failed" in str(w.message) for w in wl)
        assert h.persist_fails() == 1 and h.persist_info() == (1, False)
        with knob("persist", 0, 1):
            ref = pg.denoiser.hip().solve(x0.to(DEV), ts, spk.to(DEV), NFE)
    assert torch.isfinite(out).all() and torch.equal(out, ref)
