"""GPU: the persistent solve's group hand-off arrival words (flamed-tts_amd/csrc/persist.hpp arrive_image; persist.hip
signal / wait_ge): four words per row group, one per eight slots and each on a 128-B line of its own (the default),
against the single word per group that persist_opt 4194304 still selects.

Where an arrival is counted never changes what is computed, so every comparison is bitwise: the smallest eligible
length (most groups hold two rows), one chunk with a one-row second tile, two chunks, one group per utterance at B = 2
and B = 8, a batch of three padded to four, a Heun solve and an exact-lengths solve; then, on one handle, the same
solve three times (the launch's own reset of the enlarged counter block) and a two-chunk solve followed by the
smallest one (words of shards that the second launch's short groups still use).  Every solve must take the
persistent path and none may fail.  nfe = 4, bf16.
"""
import pytest
import torch

from test_denoiser_gpu import _prob_gen
from test_persist_gpu import DEV, PERSIST_DEFAULT, _inputs, knob
from test_rk2_cpu import STAGE

pytestmark = pytest.mark.gpu
ONE_WORD = 4194304
NFE = 4


@pytest.fixture(scope="module")
def pgb():
    return _prob_gen("bf16")


def _euler(pg, x0, spk, lens=None):
    ts = torch.linspace(0, 1, NFE + 1, device=DEV)
    with torch.inference_mode():
        return pg.denoiser.hip().solve(x0.to(DEV), ts, spk.to(DEV), NFE, lens=lens).cpu()


def _heun(pg, x0, spk):
    a, nsteps = STAGE["heun"], NFE // 2
    tb = torch.linspace(0, 1, nsteps + 1, device=DEV)[:-1]
    ts = torch.stack((tb, tb + a * (1 / nsteps)), dim=1).reshape(-1)
    with torch.inference_mode():
        return pg.denoiser.hip().solve_rk2(x0.to(DEV), ts, spk.to(DEV), nsteps, a).cpu()


def _under(pg, bits, solves):
    """The results of `solves` (callables) under persist_opt default | bits; each must be one more persistent launch,
    and the handle must have counted no failed launch."""
    hip = pg.denoiser.hip()
    out = []
    with knob("persist_opt", PERSIST_DEFAULT | bits, PERSIST_DEFAULT):
        for f in solves:
            r0 = hip.persist_status()[0] if hip.handle is not None else 0
            out.append(f())
            assert hip.persist_status()[0] == r0 + 1, "a solve did not take the persistent path"
    assert hip.persist_fails() == 0
    return out


CASES = {
    "T16": (1, 16, None, _euler),
    "T130": (1, 130, None, _euler),
    "T513": (1, 513, None, _euler),
    "B2-T64": (2, 64, None, _euler),
    "B8-T16": (8, 16, None, _euler),
    "B3-T40-padded": (3, 40, None, _euler),
    "heun-T130": (1, 130, None, _heun),
    "lens-B2-T64": (2, 64, [64, 17], _euler),
}


@pytest.mark.parametrize("case", list(CASES))
def test_shards_bitwise(pgb, case):
    pg, _ = pgb
    B, T, lens, fn = CASES[case]
    x0, spk = _inputs(200 + 7 * B + T, B, T)
    solve = (lambda: fn(pg, x0, spk, lens)) if lens else (lambda: fn(pg, x0, spk))
    (ref,) = _under(pg, ONE_WORD, [solve])
    (out,) = _under(pg, 0, [solve])
    valid = ref if lens is None else torch.cat([ref[u, :n] for u, n in enumerate(lens)])
    assert torch.isfinite(valid).all()
    assert torch.equal(out, ref)


def test_same_handle_reset_and_stale_words(pgb):
    pg, _ = pgb
    xa, sa = _inputs(301, 1, 130)
    xb, sb = _inputs(302, 1, 513)
    xc, sc = _inputs(303, 1, 16)
    solves = [lambda: _euler(pg, xa, sa)] * 3 + [lambda: _euler(pg, xb, sb), lambda: _euler(pg, xc, sc)]
    ref = _under(pg, ONE_WORD, solves)
    out = _under(pg, 0, solves)
    for r, o in zip(ref, out):
        assert torch.isfinite(r).all()
        assert torch.equal(o, r)
    assert torch.equal(out[0], out[1]) and torch.equal(out[1], out[2])
