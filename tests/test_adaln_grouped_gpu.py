"""GPU: the AdaLN table built with grouped GEMM launches (flamed-tts_amd/csrc/gemm.hpp gemm_group_kernel; flamed_den_adaln:
the time MLP's first layer with the speaker projection, and the NB + 1 LayerNorm-fold GEMMs of each kind, one launch
per family) against one launch per GEMM, which flamed_tune adaln_grouped 0 still selects.

A grouped launch runs each problem's own tile code in its own K order, so the whole table -- modulation vectors and
fold columns -- is bitwise the same: one row; rows that reuse times and speakers in permuted order; one row past the
32-row tile; the 128 rows of a full solve; and an fp32 handle, which has no fold tables.
"""
import pytest
import torch

from test_denoiser_gpu import _prob_gen
from test_persist_gpu import DEV, knob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pgs():
    return {"bf16": _prob_gen("bf16")[0], "f32": _prob_gen("f32")[0]}


def _table(pg, grouped, t, spk, tidx, sidx):
    """The table written into a NaN-filled tensor of its own (returned on the GPU, so both tables of a comparison stay
    allocated): an element that no launch writes is NaN, never the other call's value in a reused block."""
    from flamed import _native as nat
    hip = pg.denoiser.hip()
    hip._ensure(torch.device(DEV))
    ms = nat.lib().flamed_den_mods_stride(hip.handle)
    out = torch.full((tidx.numel(), ms), float("nan"), dtype=torch.float32, device=DEV)
    with knob("adaln_grouped", grouped, 1), torch.inference_mode():
        res = hip.adaln(t, spk, tidx, sidx, out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype,n_t,n_spk,R", [("bf16", 1, 1, 1), ("bf16", 3, 2, 6), ("bf16", 33, 1, 33),
                                               ("bf16", 128, 1, 128), ("f32", 3, 2, 6)])
def test_grouped_table_bitwise(pgs, dtype, n_t, n_spk, R):
    pg = pgs[dtype]
    g = torch.Generator().manual_seed(100 * n_t + R)
    t = torch.rand(n_t, generator=g).to(DEV)
    spk = torch.randn(n_spk, 256, generator=g).to(DEV)
    perm = torch.randperm(R, generator=g)  # row r takes time perm[r] % n_t and speaker perm[r] // n_t % n_spk
    tidx = (perm % n_t).to(torch.int32).to(DEV)
    sidx = (perm // n_t % n_spk).to(torch.int32).to(DEV)
    a = _table(pg, 0, t, spk, tidx, sidx)
    b = _table(pg, 1, t, spk, tidx, sidx)
    assert a.data_ptr() != b.data_ptr()
    assert a.shape[0] == R and torch.isfinite(a).all() and torch.isfinite(b).all()
    if dtype == "bf16":  # the fold columns exist and were written
        from flamed import _native as nat
        ms = nat.lib().flamed_den_mods_stride(pg.denoiser.hip().handle)
        H, NB = pg.denoiser.model_channels, pg.denoiser.num_res_blocks
        ms0 = (6 * NB + 5) * H  # modulation vectors; behind them [wa, wb] of every mlp.0 and of conv_out
        assert a.shape[1] == ms == ms0 + NB * 2 * H + 6 * pg.denoiser.out_channels
        assert a[:, ms0:].abs().sum() > 0
    assert torch.equal(a, b)
