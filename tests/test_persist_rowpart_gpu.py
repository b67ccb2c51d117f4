"""GPU: the persistent solve's tile-major LayerNorm row partials (flamed-tts_amd/csrc/persist.hip store_partials_t /
row_stats / load_row_partials, persist.hpp xpart_off: [group][16-row tile][slot][row in tile], one 128-B line per wave
store) against the row-major image they replace, which persist_opt bit 2097152 still selects.

Where a partial lies never changes the arithmetic or its order, so every comparison between the two layouts is bitwise:
at T = 16 (most row groups empty; with equal shares the depthwise halo spans seven groups), 131 (partial tiles) and 400,
under both row partitions and in combination with the hand-off variants (counter-form GroupNorm exchange, the drain
behind the weight DMA with four issuing waves, the deferred seals off); with several chunks (the LDS-table readers),
several utterances, a padded batch, exact lengths and a Heun solve, up to five and six chunks per group.  The new default itself is held to the existing bars
against the fp32 oracle (so a wrong baseline cannot pass for agreement), is deterministic, splits into parts exactly,
and still fails loudly: persist_inject poisons x with NaN, counts one failure, and the next solve recovers.
nfe = 8 unless said.
"""
import pytest
import torch

from _common import rel_l2
from _rowprofile import assert_row_profile, solve_floor
from test_denoiser_gpu import _prob_gen
from test_persist_gpu import BF16_SOLVE, DEV, PERSIST_DEFAULT, _inputs, _oracle, _runs, _solve, knob
from test_rk2_cpu import STAGE

pytestmark = pytest.mark.gpu
ROW_MAJOR = 2097152  # persist_opt: row-major row partials (the layout before xpart_off)
NFE = 8


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")


def _pair(pg, x0, spk, base, solve=None):
    """The same solve under persist_opt `base` (tile-major) and `base | ROW_MAJOR`; both must take the persistent path."""
    solve = solve or (lambda: _solve(pg, x0, spk, NFE))
    r0 = _runs(pg)
    with knob("persist_opt", base, PERSIST_DEFAULT):
        a = solve()
    with knob("persist_opt", base | ROW_MAJOR, PERSIST_DEFAULT):
        b = solve()
    assert _runs(pg) == r0 + 2, "a solve did not take the persistent path"
    return a, b


@pytest.mark.parametrize("part", [0, 2])
@pytest.mark.parametrize("extra", [0, 512, 4096 | 1, 65536], ids=["default", "gn-counter", "dma-first-4w", "no-dseal"])
@pytest.mark.parametrize("T", [16, 131, 400])
def test_layouts_bitwise(pgb, T, extra, part):
    pg, _ = pgb
    x0, spk = _inputs(31, 1, T)
    a, b = _pair(pg, x0, spk, PERSIST_DEFAULT ^ part ^ extra)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,T", [(1, 600), (2, 100), (4, 100), (3, 64), (1, 2400), (1, 3000)])
def test_layouts_bitwise_chunks_and_utterances(pgb, B, T):
    """Two chunks per group, two and four utterances (groups of 48 and 52 rows), a batch of three padded to four, five
    and six chunks per group (several row_stats trips per thread)."""
    pg, _ = pgb
    x0, spk = _inputs(32, B, T)
    a, b = _pair(pg, x0, spk, PERSIST_DEFAULT)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_layouts_bitwise_exact_lengths(pgb):
    pg, _ = pgb
    lens = [100, 61, 37, 16]
    x0, spk = _inputs(33, 4, 100)
    ts = torch.linspace(0, 1, NFE + 1, device=DEV)

    def solve():
        with torch.inference_mode():
            return pg.denoiser.hip().solve(x0.to(DEV), ts, spk.to(DEV), NFE, lens=lens).cpu()

    a, b = _pair(pg, x0, spk, PERSIST_DEFAULT, solve)
    for u, n in enumerate(lens):
        assert torch.isfinite(a[u, :n]).all()
    assert torch.equal(a, b)


def test_layouts_bitwise_heun(pgb):
    pg, _ = pgb
    x0, spk = _inputs(34, 1, 131)
    a_, nsteps = STAGE["heun"], NFE // 2
    tb = torch.linspace(0, 1, nsteps + 1, device=DEV)[:-1]
    ts = torch.stack((tb, tb + a_ * (1 / nsteps)), dim=1).reshape(-1)

    def solve():
        with torch.inference_mode():
            return pg.denoiser.hip().solve_rk2(x0.to(DEV), ts, spk.to(DEV), nsteps, a_).cpu()

    a, b = _pair(pg, x0, spk, PERSIST_DEFAULT, solve)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_default_deterministic(pgb):
    pg, _ = pgb
    x0, spk = _inputs(35, 1, 400)
    r0 = _runs(pg)
    a = _solve(pg, x0, spk, NFE)
    b = _solve(pg, x0, spk, NFE)
    assert _runs(pg) == r0 + 2
    assert torch.equal(a, b)


def test_default_parts_equal_whole(pgb):
    """[0, G) + [G, nfe) equals the whole solve (T = 300, nfe = 32): a launch that starts at step G on the partial
    buffers the first one left."""
    from flamed import _native as nat
    pg, _ = pgb
    hip = pg.denoiser.hip()
    L = nat.lib()
    x0, spk = _inputs(36, 1, 300)
    nfe = 32
    whole = _solve(pg, x0, spk, nfe)
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    with torch.inference_mode():
        G = L.flamed_den_solve_chunk(hip.handle, nfe)
        r = torch.arange(nfe, device=DEV)
        mods = hip.adaln(ts[:nfe], spk.to(DEV), r.to(torch.int32), torch.zeros(nfe, dtype=torch.int32, device=DEV))
        x = x0.to(DEV).contiguous()
        ws = nat.Workspace().get(L.flamed_den_workspace_size(hip.handle, 1, 300), DEV)
        runs0 = _runs(pg)
        for s0, s1 in ((0, G), (G, nfe)):
            nat.check(L.flamed_den_solve_part(hip.handle, nat.ptr(x), nat.ptr(mods), nfe, 1, 300, nat.ptr(ws), ws.numel(),
                                              1, s0, s1, nat.stream_ptr(DEV)), "flamed_den_solve_part")
        torch.cuda.synchronize()
    assert _runs(pg) == runs0 + 2
    assert torch.equal(x.cpu(), whole)


def test_failure_then_recovers(pgb):
    """The give-up path under the default layout: a launch that abandons at step 3 leaves NaN and counts
    one failure, and the next solve on the same handle is persistent and equal to one on a handle that never failed."""
    from flamed.models.synthesizer.prob_generator import DenoiserHIP
    pg, _ = pgb
    h = DenoiserHIP(pg.denoiser, "bf16")
    h.check_persist = False
    x0, spk = _inputs(37, 1, 131)
    ts = torch.linspace(0, 1, NFE + 1, device=DEV)
    with torch.inference_mode():
        with knob("persist_inject", 3, -1):
            bad = h.solve(x0.to(DEV), ts, spk.to(DEV), NFE)
        assert torch.isnan(bad).all()
        good = h.solve(x0.to(DEV), ts, spk.to(DEV), NFE)
        ref = pg.denoiser.hip().solve(x0.to(DEV), ts, spk.to(DEV), NFE)
    runs, broken = h.persist_info()
    assert h.persist_fails() == 1 and not broken and runs == 2
    assert torch.equal(good, ref)


@pytest.mark.parametrize("T", [131, 400])
def test_default_vs_oracle(pgb, T):
    pg, sd = pgb
    x0, spk = _inputs(38 + T, 1, T)
    r0 = _runs(pg)
    out = _solve(pg, x0, spk, NFE)
    assert _runs(pg) == r0 + 1
    ref = _oracle(sd, x0, spk, NFE)
    e = rel_l2(out, ref)
    print(f"tile-major partials T={T} {NFE} steps: vs oracle rel-L2 {e:.3e}")
    assert torch.isfinite(out).all()
    assert e < BF16_SOLVE
    assert_row_profile(out, ref, solve_floor(sd, x0, spk, NFE), f"tile-major partials T={T}")
