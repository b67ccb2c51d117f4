"""GPU parity: HIP denoiser (SimpleMLPAdaLN.forward) and Euler solve vs the oracle and the
reference-generated golden vectors.

Tolerances (rel-L2 = ||a-b|| / ||b||):
  * f32 mode (exact fp32 MFMA, different summation order): velocity <= 2e-5, 4-step solve <= 1e-4
  * bf16 mode (bf16 GEMM operands, fp32 accumulate/residual/norms): velocity <= 8e-3 (~2x the measured
    3.7e-3 .. 3.9e-3), short solves <= 6e-3 (SURVEY.md §8(c) allows 2e-2; the reference itself under
    CPU bf16 autocast drifts to 8.5e-3 velocity rel-L2).  128/256-step solves: test_configs_gpu.py.
  * bf16 mode, per frame: no frame further from the oracle than 2x the worst frame of a bf16 emulation of the
    oracle on the same input (_rowprofile.assert_row_profile) -- the global norm above divides an error confined
    to a few frames (a tile, chunk or utterance edge) by sqrt(frames).
"""
import numpy as np
import pytest
import torch
import yaml

from _common import golden, seeded, t32, rel_l2, orc, PKG
from _rowprofile import assert_row_profile, emulated_prob_sample, solve_floor, velocity_floor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16_VEL = 8e-3
BF16_SOLVE = 6e-3


def _prob_gen(dtype):
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    import os
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    sd = seeded("prob_generator")
    pg.load_state_dict({k[len("prob_generator."):]: v for k, v in sd.items()})
    pg.denoiser.hip_dtype = dtype
    return pg.to(DEV), sd


@pytest.fixture(scope="module")
def pg_f32():
    return _prob_gen("f32")


@pytest.fixture(scope="module")
def pg_bf16():
    return _prob_gen("bf16")


def _vel(pg, x, t, c):
    with torch.inference_mode():
        return pg.denoiser(t32(x).to(DEV), t32(t).to(DEV), t32(c).to(DEV)).cpu()


@pytest.mark.parametrize("mode,tol", [("f32", 2e-5), ("bf16", BF16_VEL)])
def test_velocity_golden(mode, tol, pg_f32, pg_bf16):
    pg, _ = pg_f32 if mode == "f32" else pg_bf16
    g = golden("den_full")
    assert rel_l2(_vel(pg, g["x"], g["t1"], g["c"]), g["v1"]) < tol          # sampling t (1,1)
    assert rel_l2(_vel(pg, g["xB"], g["tB"], g["cB"]), g["vB"]) < tol        # training t (B,T)
    assert rel_l2(_vel(pg, g["xB"], g["t_mid"], g["cB"]), g["vB1"]) < tol    # batched, padded-free


@pytest.mark.parametrize("B,T", [(1, 33), (3, 70), (2, 130), (2, 1), (1, 2), (2, 5), (1, 31)])
def test_velocity_ragged_shapes_f32(B, T, pg_f32):
    pg, sd = pg_f32
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, T, 256, generator=g)
    c = torch.randn(B, 256, generator=g)
    t = torch.tensor([[0.4]])
    ref = orc.denoiser_forward(sd, x, t, c)
    assert rel_l2(_vel(pg, x, t, c), ref) < 2e-5


@pytest.mark.parametrize("mode,tol", [("f32", 1e-4), ("bf16", BF16_SOLVE)])
def test_prob_sample_golden(mode, tol, pg_f32, pg_bf16):
    pg, sd = pg_f32 if mode == "f32" else pg_bf16
    g = golden("prob_sample")
    lens = t32(g["lens"])
    T = g["cond"].shape[2]
    mask = ~(torch.arange(T)[None, :] >= lens[:, None]).unsqueeze(-1)
    torch.manual_seed(int(g["rng_seed"]))
    with torch.inference_mode():
        lat = pg.sample(t32(g["cond"]).to(DEV), t32(g["spk"]).to(DEV), mask.to(DEV), nfe=int(g["nfe"]),
                        temperature=float(g["temperature"])).cpu()
    assert lat.shape == g["latents"].shape
    assert rel_l2(lat, g["latents"]) < tol
    if mode == "bf16":  # per-frame profile (padded frames included); the f32 bar already resolves single frames
        torch.manual_seed(int(g["rng_seed"]))
        noise = torch.randn((lat.shape[0], T, lat.shape[1]))  # the draw ProbGenerator.sample makes (prob_generator.py:440)
        floor = emulated_prob_sample(sd, t32(g["cond"]), t32(g["spk"]), mask, int(g["nfe"]), float(g["temperature"]), noise)
        assert_row_profile(lat.transpose(1, 2), t32(g["latents"]).transpose(1, 2), floor, "prob_sample golden bf16")


def test_solve_graph_equals_eager_and_oracle(pg_f32):
    pg, sd = pg_f32
    hip = pg.denoiser.hip()
    g = torch.Generator().manual_seed(9)
    B, T, nfe = 2, 100, 6
    x0 = torch.randn(B, T, 256, generator=g)
    spk = torch.randn(B, 256, generator=g)
    ts = torch.linspace(0, 1, nfe + 1)
    with torch.inference_mode():
        pg.denoiser.hip_graph = True
        a = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
        b2 = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()  # graph replay
        pg.denoiser.hip_graph = False
        e = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
        pg.denoiser.hip_graph = True
    assert torch.equal(a, b2) and torch.equal(a, e)
    ref = orc.euler_solve(sd, x0, spk, nfe)
    assert rel_l2(a, ref) < 1e-4


def test_unsupported_dims_fall_back_to_torch():
    """Dims the library does not specialise (H = 64) keep the module on its torch ops on ROCm (with a
    warning), equal to the same module on CPU; the HIP library is never asked to run them."""
    from flamed.models.synthesizer.prob_generator import SimpleMLPAdaLN
    den = SimpleMLPAdaLN(16, 64, 16, 32, 2, 31, 1, 15, 1, None).eval()
    g = torch.Generator().manual_seed(2)
    x, t, c = torch.randn(1, 8, 16, generator=g), torch.rand(1, 1, generator=g), torch.randn(1, 32, generator=g)
    with torch.inference_mode():
        ref = den(x, t, c)
        den = den.to(DEV)
        with pytest.warns(UserWarning, match="does not specialise"):
            from flamed import _native as nat
            nat._supported.clear()
            v = den(x.to(DEV), t.to(DEV), c.to(DEV))
    assert den._hip is None
    assert rel_l2(v.cpu(), ref) < 1e-5


@pytest.mark.parametrize("target,mx", [(512, 2), (1024, 4)])
def test_split_k_solve_bf16(target, mx, pg_bf16):
    """Small-M split-K (write-through slab hand-off, last arriver reduces) gives the unsplit result
    up to fp32 summation order, and stays within the bf16 tolerance of the oracle."""
    from flamed import _native as nat
    pg, sd = pg_bf16
    hip = pg.denoiser.hip()
    g = torch.Generator().manual_seed(11)
    B, T, nfe = 1, 200, 4
    x0 = torch.randn(B, T, 256, generator=g)
    spk = torch.randn(B, 256, generator=g)
    ts = torch.linspace(0, 1, nfe + 1)
    L = nat.lib()
    with torch.inference_mode():
        base = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
        try:
            nat.check(L.flamed_tune(b"persist", 0), "tune")  # the graph-of-launches path is under test
            nat.check(L.flamed_tune(b"splitk_target", target), "tune")
            nat.check(L.flamed_tune(b"splitk_max", mx), "tune")
            pg.denoiser.hip_graph = False
            a = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
            pg.denoiser.hip_graph = True
            b = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
            c = hip.solve(x0.to(DEV), ts.to(DEV), spk.to(DEV), nfe).cpu()
        finally:
            nat.check(L.flamed_tune(b"splitk_target", 1), "tune")
            nat.check(L.flamed_tune(b"splitk_max", 4), "tune")
            nat.check(L.flamed_tune(b"persist", 1), "tune")
    assert torch.equal(a, b) and torch.equal(b, c)  # deterministic reduction, graph == eager
    assert rel_l2(a, base) < 5e-3  # bf16 re-rounding of U after a different fp32 summation order
    ref = orc.euler_solve(sd, x0, spk, nfe)
    assert rel_l2(a, ref) < BF16_SOLVE
    assert_row_profile(a, ref, solve_floor(sd, x0, spk, nfe), f"split-K target {target} max {mx}")


@pytest.mark.parametrize("per_frame_t", [False, True])
def test_velocity_large_m_bf16(per_frame_t, pg_bf16):
    """Large-M bf16 path (B*T >= 8192 rows): LN/GN/cast passes to bf16 rows + 128x128 LDS-DMA GEMM tiles
    with XCD-aware placement, vs the oracle (bf16 tolerance); also the fused register-staged path
    (flamed_tune big 0) on the same input."""
    from flamed import _native as nat
    pg, sd = pg_bf16
    g = torch.Generator().manual_seed(21)
    B, T = 17, 500
    x = torch.randn(B, T, 256, generator=g)
    c = torch.randn(B, 256, generator=g)
    t = torch.rand(B, T, generator=g) if per_frame_t else torch.tensor([[0.6]])
    ref = orc.denoiser_forward(sd, x, t, c)
    L = nat.lib()
    v_big = _vel(pg, x, t, c)
    try:
        nat.check(L.flamed_tune(b"big", 0), "tune")
        v_fused = _vel(pg, x, t, c)
    finally:
        nat.check(L.flamed_tune(b"big", 1), "tune")
    assert rel_l2(v_big, ref) < BF16_VEL
    assert rel_l2(v_fused, ref) < BF16_VEL
    floor = velocity_floor(sd, x, t, c)
    assert_row_profile(v_big, ref, floor, f"large-M 128x128 per_frame_t={per_frame_t}")
    assert_row_profile(v_fused, ref, floor, f"large-M fused (big 0) per_frame_t={per_frame_t}")


@pytest.mark.parametrize("knobs,B,T", [
    ({"dma": 0, "bn32": 0}, 1, 200), ({"dma": 1, "bn32": 0}, 1, 200), ({"dma": 2, "bn32": 0}, 1, 200),
    ({"dma": 0, "bn32": 1}, 1, 200), ({"dma": 2, "bn32": 1}, 1, 200), ({"dma": 1, "bn32": 1}, 3, 1000),
    ({"big_ns": 3}, 17, 500), ({"big": 1, "dw_tc": 128}, 17, 500),
    ({"dw_cg": 16}, 2, 300), ({"dw_cg32": 0}, 1, 131), ({"dma_ns": 8}, 1, 400), ({"dma_ns": 4, "dma": 2}, 1, 250),
    ({"lnfold": 0}, 1, 400), ({"lnfold": 0}, 17, 500), ({"lnfold": 0, "big": 0}, 5, 400),
    ({"g8p_rows": 0}, 41, 400), ({"x16": 1}, 41, 400), ({"x16": 1, "lnfold": 0}, 41, 400), ({"x16": 1}, 5, 400),
    ({"dwgn": 0}, 41, 400), ({"dwgn": 0, "x16": 1}, 41, 400), ({"dwgn": 1}, 30, 64), ({"dwgn": 1}, 12, 130),
    ({"dwgn": 1}, 4, 512), ({"dwgn": 1}, 4, 513), ({"dwgn": 1, "x16": 1}, 7, 333),
    ({"dwgn_small": 0}, 1, 400), ({"dwgn_small": 0}, 2, 300), ({"dwgn_small": 1}, 1, 577), ({"dwgn_small": 1}, 1, 449),
    ({"dwgn_small": 1}, 3, 130), ({"dwgn_small": 1}, 1, 64), ({"dwgn_small": 1, "lnfold": 0}, 1, 250),
])
def test_velocity_tuning_paths_bf16(knobs, B, T, pg_bf16):
    """Every GEMM main-loop / tile / pipeline variant behind flamed_tune computes the same velocity (vs the
    oracle, bf16 tolerance): register-staged vs LDS-DMA, 32- vs 64-wide small tiles, mid-M, large-M ring
    depth, depthwise T-chunk, the 256 x 256 8-phase tiles (B*T = 16,400) vs the 128 x 128 ring, and the
    large-M bf16 residual stream (x16), and the whole-utterance depthwise conv + GroupNorm kernel (dwgn:
    1, 2, 3 and 8 frame chunks; T = 513 falls back to the chunked conv + GroupNorm pass) and its small-M
    form (one workgroup per utterance x 8 channels, RPT = 1..9; T = 577 falls back)."""
    from flamed import _native as nat
    pg, sd = pg_bf16
    g = torch.Generator().manual_seed(B * 7 + T)
    x = torch.randn(B, T, 256, generator=g)
    c = torch.randn(B, 256, generator=g)
    t = torch.tensor([[0.35]])
    ref = orc.denoiser_forward(sd, x, t, c)
    L = nat.lib()
    defaults = {"dma": 1, "bn32": 1, "big": 1, "big_ns": 2, "dw_tc": 64, "dw_cg": 32, "dw_cg32": 1536, "dma_ns": 3, "lnfold": 1,
                "g8p_rows": 12800, "x16": 0, "dwgn": 1, "dwgn_small": 1}
    try:
        for k, v in knobs.items():
            nat.check(L.flamed_tune(k.encode(), v), "tune")
        v_hip = _vel(pg, x, t, c)
    finally:
        for k in knobs:
            nat.check(L.flamed_tune(k.encode(), defaults[k]), "tune")
    assert rel_l2(v_hip, ref) < BF16_VEL
    # x16 cases (all on the large-M path, where the knob acts): the floor rounds the residual stream and the
    # depthwise output too
    floor = velocity_floor(sd, x, t, c, x16=bool(knobs.get("x16")))
    assert_row_profile(v_hip, ref, floor, f"tuning {knobs} B={B} T={T}")


@pytest.mark.parametrize("B,T,per_frame_t", [(1, 400, False), (2, 300, True), (17, 500, False), (4, 400, False)])
def test_lnfold_error_budget(B, T, per_frame_t, pg_bf16):
    """The LayerNorm fold (mlp.0 / conv_out on bf16 x*alpha with rstd (acc - mean wa) + wb in the epilogue)
    keeps the bf16 velocity error at the level of the A-loader LayerNorm path: at most 1.5x its rel-L2
    (+1e-3) against the fp32 oracle, small-M (DMA), per-frame-t and large-M (128x128) paths."""
    from flamed import _native as nat
    pg, sd = pg_bf16
    g = torch.Generator().manual_seed(B * 5 + T)
    x = torch.randn(B, T, 256, generator=g)
    c = torch.randn(B, 256, generator=g)
    t = torch.rand(B, T, generator=g) if per_frame_t else torch.tensor([[0.55]])
    ref = orc.denoiser_forward(sd, x, t, c)
    L = nat.lib()
    nat.check(L.flamed_tune(b"fold_rows", 0), "tune")  # fold on the large-M path too (default from 6144 rows)
    try:
        e_fold = rel_l2(_vel(pg, x, t, c), ref)
    finally:
        nat.check(L.flamed_tune(b"fold_rows", 6144), "tune")
    try:
        nat.check(L.flamed_tune(b"lnfold", 0), "tune")
        e_ln = rel_l2(_vel(pg, x, t, c), ref)
    finally:
        nat.check(L.flamed_tune(b"lnfold", 1), "tune")
    print(f"bf16 velocity rel-L2: lnfold {e_fold:.3e}, A-loader LN {e_ln:.3e}")
    assert e_fold < 1.5 * e_ln + 1e-3


def test_single_value_groupnorm_raises(pg_f32):
    """B*T == 1 leaves one value per GroupNorm(H, H) group: the reference's F.group_norm raises ValueError
    (prob_generator.py:89); the HIP path raises the same error for velocity() and solve()."""
    pg, sd = pg_f32
    x, c, t = torch.randn(1, 1, 256), torch.randn(1, 256), torch.tensor([[0.4]])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        orc.denoiser_forward(sd, x, t, c)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _vel(pg, x, t, c)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        pg.denoiser.hip().solve(x.to(DEV), torch.linspace(0, 1, 5, device=DEV), c.to(DEV), 4)


@pytest.mark.parametrize("B,T", [(2, 1), (1, 2), (1, 17), (1, 319), (1, 320), (2, 160), (1, 1535), (1, 1536),
                                 (3, 512), (4, 1536), (1, 6144)])
def test_velocity_path_boundaries_bf16(B, T, pg_bf16):
    """bf16 velocity at the row counts where the dispatch changes path: T shorter than the depthwise
    halo, 32x32 -> 32x64 tiles (320 rows), small-M -> large-M 128x128 path (1536 rows), LayerNorm fold on
    the large-M path (6144 rows), single- and multi-utterance tiles."""
    pg, sd = pg_bf16
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, T, 256, generator=g)
    c = torch.randn(B, 256, generator=g)
    t = torch.tensor([[0.3]])
    ref = orc.denoiser_forward(sd, x, t, c)
    v = _vel(pg, x, t, c)
    e = rel_l2(v, ref)
    print(f"B={B} T={T} bf16 velocity rel-L2 {e:.3e}")
    # T <= 2: GroupNorm(H, H) over <= 2 frames per channel amplifies the bf16 rounding of the GEMM
    # operands (measured 1.2e-2 at B=1, T=2); SURVEY.md §8(c)'s bf16 bar 2e-2 applies there
    assert e < (BF16_VEL if T > 2 else 2e-2)
    assert_row_profile(v, ref, velocity_floor(sd, x, t, c), f"path boundary B={B} T={T}")  # the floor adapts at T <= 2


@pytest.mark.parametrize("mode,tol", [("f32", 1e-5), ("bf16", 8e-3)])
def test_cond_fold_golden(mode, tol, pg_f32):
    """HIP condition fold (QuantizerEncoding + ConditionDownSampler, prob_generator.py:167-205, 368-381)
    vs the reference's own output on padded lengths (golden prob_sample.cond_fold, lens 48/33)."""
    pg, _ = pg_f32
    g = golden("prob_sample")
    lens = t32(g["lens"])
    T = g["cond"].shape[2]
    mask = ~(torch.arange(T)[None, :] >= lens[:, None]).unsqueeze(-1)
    pg.cond_hip_dtype = mode
    try:
        with torch.inference_mode():
            cf = pg.fold_condition(t32(g["cond"]).to(DEV), mask.to(DEV)).cpu()
    finally:
        pg.cond_hip_dtype = "f32"
    e = rel_l2(cf, g["cond_fold"])
    print(f"cond fold {mode} rel-L2 {e:.3e}")
    assert cf.shape == g["cond_fold"].shape and e < tol


@pytest.mark.parametrize("B,T", [(1, 400), (3, 257)])
def test_cond_fold_vs_oracle(B, T, pg_f32):
    pg, sd = pg_f32
    gen = torch.Generator().manual_seed(B * 31 + T)
    cond = torch.randn(B, 6, T, 384, generator=gen)
    lens = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lens[0] = T
    mask = ~(torch.arange(T)[None, :] >= lens[:, None]).unsqueeze(-1)
    with torch.inference_mode():
        cf = pg.fold_condition(cond.to(DEV), mask.to(DEV)).cpu()
    e = rel_l2(cf, orc.cond_fold(sd, cond, mask))
    print(f"cond fold B={B} T={T} f32 rel-L2 {e:.3e}")
    assert e < 1e-5


@pytest.mark.parametrize("B,T,nfe", [(1, 400, 128), (3, 37, 8), (2, 1, 4), (1, 50, 7)])
def test_fused_euler_solve_bitwise(B, T, nfe, pg_bf16):
    """Small-M solve graphs compute the conv_out tap combine + Euler update (prob_generator.py:238-245,
    445) inside the next step's proj_in loader (flamed_tune fuse_euler, 25 launches per step).  Same fp32
    operation order as the combine kernel, so the solve is bitwise equal to the unfused graph and to the
    eager solve; nfe = 7 has an odd graph chunk and takes the unfused path."""
    from flamed import _native as nat
    pg, _ = pg_bf16
    hip = pg.denoiser.hip()
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(B, T, 256, generator=g).to(DEV)
    spk = torch.randn(B, 256, generator=g).to(DEV)
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    L = nat.lib()
    outs = []
    nat.check(L.flamed_tune(b"persist", 0), "tune")  # the graph-of-launches path is under test
    try:
        with torch.inference_mode():
            for fuse, graph in ((1, True), (0, True), (1, False)):
                nat.check(L.flamed_tune(b"fuse_euler", fuse), "tune")
                pg.denoiser.hip_graph = graph
                outs.append(hip.solve(x0, ts, spk, nfe).cpu())
    finally:
        nat.check(L.flamed_tune(b"fuse_euler", 1), "tune")
        nat.check(L.flamed_tune(b"persist", 1), "tune")
        pg.denoiser.hip_graph = True
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_solve_in_parts_equals_whole(pg_bf16):
    """flamed_den_solve_part: the graph-chunked solve run as [0, G) then [G, nfe) (as a caller overlapping
    later AdaLN rows would) is bitwise the whole flamed_den_solve."""
    from flamed import _native as nat
    pg, _ = pg_bf16
    hip = pg.denoiser.hip()
    L = nat.lib()
    g = torch.Generator().manual_seed(41)
    B, T, nfe = 1, 400, 32
    x0 = torch.randn(B, T, 256, generator=g).to(DEV)
    spk = torch.randn(B, 256, generator=g).to(DEV)
    ts = torch.linspace(0, 1, nfe + 1, device=DEV)
    with torch.inference_mode():
        whole = hip.solve(x0, ts, spk, nfe).cpu()
        G = L.flamed_den_solve_chunk(hip.handle, nfe)
        assert 0 < G < nfe and nfe % G == 0
        r = torch.arange(nfe * B, device=DEV)
        mods = hip.adaln(ts[:nfe], spk, (r // B).to(torch.int32), (r % B).to(torch.int32))
        x = x0.clone()
        ws = nat.Workspace().get(L.flamed_den_workspace_size(hip.handle, B, T), DEV)
        for s0, s1 in ((0, G), (G, nfe)):
            nat.check(L.flamed_den_solve_part(hip.handle, nat.ptr(x), nat.ptr(mods), nfe, B, T, nat.ptr(ws), ws.numel(),
                                              1, s0, s1, nat.stream_ptr(DEV)), "flamed_den_solve_part")
        assert L.flamed_den_solve_part(hip.handle, nat.ptr(x), nat.ptr(mods), nfe, B, T, nat.ptr(ws), ws.numel(),
                                       1, 1, nfe, nat.stream_ptr(DEV)) == 1001  # off a chunk boundary
        torch.cuda.synchronize()
    assert torch.equal(x.cpu(), whole)


_launch_refs = {}


def _launch_ref(sd, B, T):
    """Inputs, oracle velocity and bf16-emulation floor of one shape, computed once for the cases that share it."""
    if (B, T) not in _launch_refs:
        g = torch.Generator().manual_seed(B * 1009 + T)
        x = torch.randn(B, T, 256, generator=g)
        c = torch.randn(B, 256, generator=g)
        t = torch.tensor([[0.45]])
        _launch_refs[(B, T)] = (x, t, c, orc.denoiser_forward(sd, x, t, c), velocity_floor(sd, x, t, c))
    return _launch_refs[(B, T)]


@pytest.mark.parametrize("knobs,B,T", [
    ({}, 5, 333), ({}, 3, 513), ({}, 13, 100), ({}, 16, 100), ({"g8p_rows": 0}, 46, 250), ({"g8p_rows": 11500}, 46, 250),
    ({}, 2, 130), ({}, 1, 319), ({}, 1, 9)])
def test_launch_edge_profiles(knobs, B, T, pg_bf16):
    """The per-frame profile of one bf16 velocity where tile edges fall inside utterances and utterance edges
    inside tiles.  (5, 333): 1,665 rows, 128 x 128 tiles, whole-utterance depthwise + GroupNorm kernel; (3, 513):
    dwgn falls back to the chunked pass; (13, 100): 1,300 rows stay under the large-M threshold (1,536), so it is
    the small-M tiles that span utterance edges there -- (16, 100), 1,600 rows, is the shape where a 128-row tile
    spans two or three utterances; (46, 250): 11,500 rows, the smallest count the 256 x 256 8-phase dispatch accepts
    (180 tiles; a 256-row tile spans two utterances; subset floor) -- g8p_rows 0 switches the 8-phase tiles OFF
    (launch_big: g8 > 0), so that case is the 128 x 128 ring at this size and g8p_rows 11500 is the 8-phase one;
    (2, 130) and (1, 319): small-M tiles, dwgn_small; (1, 9): under one tile and under the depthwise halo (the
    persistent solve takes no T < 16)."""
    from flamed import _native as nat
    pg, sd = pg_bf16
    x, t, c, ref, floor = _launch_ref(sd, B, T)
    L = nat.lib()
    try:
        for k, v in knobs.items():
            nat.check(L.flamed_tune(k.encode(), v), "tune")
        v_hip = _vel(pg, x, t, c)
    finally:
        for k in knobs:
            nat.check(L.flamed_tune(k.encode(), {"g8p_rows": 12800}[k]), "tune")
    e = rel_l2(v_hip, ref)
    print(f"launch edge {knobs} B={B} T={T}: velocity rel-L2 {e:.3e}")
    assert e < BF16_VEL
    assert_row_profile(v_hip, ref, floor, f"launch edge {knobs} B={B} T={T}")
