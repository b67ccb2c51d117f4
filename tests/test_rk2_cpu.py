"""Second-order ODE solvers (midpoint, Heun) of the denoiser solve, CPU side: the C entry point's declaration,
binding, export and host-side argument checks; the custom op; ProbGenerator.sample(solver=...) on the module's
torch ops against the two-stage formula composed from the oracle's velocity; the solvers' order of accuracy; and
the synthesize.py flag.

The formula (include/flamed_hip.h, flamed_den_solve_rk2), nfe velocity evaluations = nfe / 2 steps of dt = 2 / nfe:
    y      = x + (a dt) v(x, t_i)
    x_next = x + c1 (y - x) + (c2 dt) v(y, t_i + a dt),   c1 = (2a - 1) / (2 a^2),  c2 = 1 / (2a)
with a = 1/2 (midpoint) or 1 (Heun)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from _common import PKG, orc, rel_l2, seeded

TOL = 2e-5  # module vs oracle, as tests/test_modules_cpu.py
C = 256
STAGE = {"midpoint": 0.5, "heun": 1.0}


def rk2_oracle(sd, x, spk, nfe, a):
    """The two-stage solve from x (B, T, C), composed from the oracle's velocity (fp32, Python-float coefficients)."""
    nsteps = nfe // 2
    ts = torch.linspace(0, 1, nsteps + 1)
    dt = 1 / nsteps
    c1, c2 = (2 * a - 1) / (2 * a * a), 1 / (2 * a)
    for i in range(nsteps):
        y = x + (a * dt) * orc.denoiser_forward(sd, x, ts[i].reshape(1, 1), spk)
        v = orc.denoiser_forward(sd, y, (ts[i] + a * dt).reshape(1, 1), spk)
        x = x + c1 * (y - x) + (c2 * dt) * v
    return x


def rk2_sample_oracle(sd, cond, spk, mask, nfe, temperature, noise, a):
    x = noise * temperature + orc.cond_fold(sd, cond, mask)
    return rk2_oracle(sd, x, spk, nfe, a).transpose(1, -1)


@pytest.fixture(scope="module")
def pg_sd():
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    sd = seeded("prob_generator")
    pg.load_state_dict({k[len("prob_generator."):]: v for k, v in sd.items()})
    return pg, sd


def test_header_binding_export_and_validation():
    from flamed import _native as nat
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "flamed_hip.h")).read()
    assert "FLAMED_API int flamed_den_solve_rk2(" in hdr
    assert "flamed_den_solve_rk2" in nat.SIGNATURES
    L = nat.lib()
    fn = L.flamed_den_solve_rk2  # AttributeError if the library does not export it
    assert fn.argtypes[4] is ctypes.c_double and len(fn.argtypes) == 11
    one = ctypes.c_void_p(256)  # non-null stand-ins: the scalar checks come before any pointer is touched

    def err(h, x, m, nsteps, a, ws):
        rc = fn(h, x, m, nsteps, a, 1, 16, ws, 1 << 20, 1, None)
        return rc, (L.flamed_last_error() or b"").decode()

    for nsteps in (0, -3):
        rc, msg = err(one, one, one, nsteps, 0.5, one)
        assert rc == 1001 and "nsteps" in msg, (rc, msg)
    for a in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        rc, msg = err(one, one, one, 4, a, one)
        assert rc == 1001 and "stage parameter" in msg, (a, rc, msg)
    for k in range(4):
        p = [one] * 4
        p[k] = None
        rc, msg = err(p[0], p[1], p[2], 4, 0.5, p[3])
        assert rc == 1001 and "null" in msg, (k, rc, msg)


def test_op_registered_with_fake_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops
    assert "den_solve_rk2" in ops.OPS
    schema = torch.ops.flamed_hip.den_solve_rk2.default._schema
    assert str(schema).startswith("flamed_hip::den_solve_rk2(") and "float a" in str(schema), str(schema)
    assert [a.name for a in schema.arguments] == ["oid", "xt", "ts_eval", "spk", "nsteps", "a"]
    # den_solve's schema is as it was
    assert [a.name for a in torch.ops.flamed_hip.den_solve.default._schema.arguments] == ["oid", "xt", "ts", "spk", "nfe"]
    with FakeTensorMode():
        s = torch.ops.flamed_hip.den_solve_rk2(1, torch.empty(2, 50, C), torch.empty(8), torch.empty(2, C), 4, 0.5)
        assert s.shape == (2, 50, C) and s.dtype == torch.float32


def _sample_inputs(B=2, T=24, short=17, seed=5):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, 6, T, 384, generator=g)
    spk = torch.randn(B, C, generator=g)
    lens = torch.tensor([T] + [short] * (B - 1))
    mask = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(-1)
    return cond, spk, mask


@pytest.mark.parametrize("solver", ["midpoint", "heun"])
def test_sample_cpu_vs_composed_oracle(pg_sd, solver):
    pg, sd = pg_sd
    cond, spk, mask = _sample_inputs()
    torch.manual_seed(11)
    noise = torch.randn((2, 24, C))  # the draw ProbGenerator.sample makes from the global CPU RNG
    torch.manual_seed(11)
    with torch.inference_mode():
        lat = pg.sample(cond, spk, mask, nfe=4, temperature=0.3, solver=solver)
    ref = rk2_sample_oracle(sd, cond, spk, mask, 4, 0.3, noise, STAGE[solver])
    e = rel_l2(lat, ref)
    print(f"ProbGenerator.sample CPU {solver} nfe=4 vs composed oracle: rel-L2 {e:.3e}")
    assert lat.shape == (2, C, 24) and e < TOL
    # and it is not the Euler trajectory
    assert rel_l2(lat, orc.prob_sample(sd, cond, spk, mask, nfe=4, temperature=0.3, noise=noise)) > 1e-3


def test_sample_euler_default_and_errors(pg_sd):
    pg, _ = pg_sd
    cond, spk, mask = _sample_inputs()
    with torch.inference_mode():
        torch.manual_seed(3)
        a = pg.sample(cond, spk, mask, nfe=4, temperature=0.3)
        torch.manual_seed(3)
        b = pg.sample(cond, spk, mask, nfe=4, temperature=0.3, solver="euler")
    assert torch.equal(a, b)
    for solver in ("midpoint", "heun"):
        with pytest.raises(ValueError, match="even"):
            pg.sample(cond, spk, mask, nfe=5, solver=solver)
    with pytest.raises(ValueError, match="unknown solver"):
        pg.sample(cond, spk, mask, nfe=4, solver="rk4")


def test_order_of_accuracy(pg_sd):
    """B = 1, T = 16, fp32 torch ops; the reference is midpoint at 64 evaluations.  A second-order solver quarters
    its error when the evaluations double and a first-order one halves it: midpoint and Heun at 16 evaluations are
    at least 4x closer than Euler at 16, err(8) / err(16) >= 3 for them and < 3 for Euler.  A wrong stage time or
    coefficient drops a solver to first order and fails this."""
    pg, _ = pg_sd
    cond, spk, mask = _sample_inputs(B=1, T=16, seed=9)

    def run(solver, nfe):
        torch.manual_seed(21)
        with torch.inference_mode():
            return pg.sample(cond, spk, mask, nfe=nfe, temperature=0.3, solver=solver)

    ref = run("midpoint", 64)
    err = {(s, n): rel_l2(run(s, n), ref) for s in ("euler", "midpoint", "heun") for n in (8, 16)}
    print("order of accuracy, rel-L2 vs midpoint-64: " +
          ", ".join(f"{s} {err[s, 8]:.2e} -> {err[s, 16]:.2e}" for s in ("euler", "midpoint", "heun")))
    for s in ("midpoint", "heun"):
        assert err[s, 16] <= err["euler", 16] / 4, (s, err)
        assert err[s, 8] / err[s, 16] >= 3, (s, err)
    assert err["euler", 8] / err["euler", 16] < 3, err


def _prompts(d):
    from flamed.utils.audio import write_wav
    os.makedirs(d, exist_ok=True)
    write_wav(os.path.join(d, "p0.wav"), np.random.default_rng(0).normal(0, 0.1, 4000).astype(np.float32))


def test_cli_flag_and_namespace_default(tmp_path):
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed.utils.random_ckpt import write
    p = syn.build_arg_parser()
    base = ["--ckpt-path", "c", "--cfg-path", "g"]
    assert p.parse_args(base).solver_denoiser == "euler"
    assert p.parse_args(base + ["--solver-denoiser", "heun"]).solver_denoiser == "heun"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--solver-denoiser", "rk4"])
    paths = write(str(tmp_path / "ck"))
    _prompts(tmp_path / "pr")
    ns = dict(ckpt_path=paths["ckpt"], cfg_path=paths["cfg"], text="hello world.", prompt_list=["p0.wav"],
              prompt_dir=str(tmp_path / "pr"), metadata_file=None, output_dir=str(tmp_path / "out"), weights_only=True,
              nsteps_durgen=4, nsteps_denoiser=4, temp_durgen=0.3, temp_denoiser=0.3, device="cpu", skip_existing=True,
              batch_size=4, codec_ckpt_dir=str(tmp_path / "ck"))
    assert syn.main(argparse.Namespace(**ns)) > 0  # a hand-built Namespace without the field: Euler, the old name
    assert os.listdir(tmp_path / "out") == ["p0-4-4-0.3-0.3.wav"]
    assert syn.main(argparse.Namespace(**ns, solver_denoiser="midpoint")) > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["p0-4-4-0.3-0.3-midpoint.wav", "p0-4-4-0.3-0.3.wav"]
