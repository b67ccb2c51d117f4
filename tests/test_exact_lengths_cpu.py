"""Exact lengths, CPU side: every utterance of a padded ragged batch folded and solved over its own frames only, so
it gets what it would get alone at T = len_u from noise[u, :len_u] of the same (B, T, C) draw, with exactly 0 behind
it.  The three C entry points' declaration, binding, export and host-side argument checks; the custom ops;
ProbGenerator.sample(exact_lengths=True) on the module's torch ops against the oracle run alone per utterance; the
errors; the synthesize.py flag; and the pass-through of Flamed.sample_batch."""
import argparse
import ctypes
import os
import sys

import pytest
import torch
import yaml

from _common import PKG, orc, rel_l2, seeded
from test_rk2_cpu import STAGE, _prompts, rk2_oracle

TOL = 2e-5  # module vs oracle, as tests/test_modules_cpu.py
C = 256
LENS = [24, 17]


@pytest.fixture(scope="module")
def pg_sd():
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    sd = seeded("prob_generator")
    pg.load_state_dict({k[len("prob_generator."):]: v for k, v in sd.items()})
    return pg, sd


def _inputs(lens, seed=5):
    B, T = len(lens), max(lens)
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, 6, T, 384, generator=g)
    spk = torch.randn(B, C, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    return cond, spk, mask


def alone_oracle(sd, cond, spk, noise, lens, nfe, temperature, a=None):
    """The definition: utterance u alone at T = len_u, a mask of ones, noise[u, :len_u]; (B, C, T), 0 behind len_u."""
    T = cond.shape[2]
    out = torch.zeros(len(lens), C, T)
    for u, n in enumerate(lens):
        cu, su, ones = cond[u:u + 1, :, :n], spk[u:u + 1], torch.ones(1, n, 1, dtype=torch.bool)
        if a is None:
            lat = orc.prob_sample(sd, cu, su, ones, nfe=nfe, temperature=temperature, noise=noise[u:u + 1, :n])
        else:
            x0 = noise[u:u + 1, :n] * temperature + orc.cond_fold(sd, cu, ones)
            lat = rk2_oracle(sd, x0, su, nfe, a).transpose(1, -1)
        out[u, :, :n] = lat[0]
    return out


def test_header_binding_export_and_validation():
    from flamed import _native as nat
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "flamed_hip.h")).read()
    integ = open(os.path.join(os.path.dirname(PKG), "INTEGRATION.md")).read()
    for name in ("flamed_den_solve_lens", "flamed_den_solve_rk2_lens", "flamed_cond_fold_exact"):
        assert f"FLAMED_API int {name}(" in hdr and name in nat.SIGNATURES and name in integ, name
    L = nat.lib()
    euler, rk2, fold = L.flamed_den_solve_lens, L.flamed_den_solve_rk2_lens, L.flamed_cond_fold_exact  # exported
    assert len(euler.argtypes) == 11 and len(rk2.argtypes) == 12 and rk2.argtypes[5] is ctypes.c_double
    assert fold.argtypes == L.flamed_cond_fold.argtypes
    one = ctypes.c_void_p(256)  # non-null stand-ins: every check below comes before any pointer is touched
    B, T = 2, 16

    def lens_of(*v):
        return (ctypes.c_int * len(v))(*v)

    def err(fn, *args):
        rc = fn(*args)
        return rc, (L.flamed_last_error() or b"").decode()

    good = lens_of(16, 9)
    for k in range(5):  # handle, state, table, lengths, workspace
        p = [one, one, one, good, one]
        p[k] = None
        rc, msg = err(euler, p[0], p[1], p[2], p[3], 4, B, T, p[4], 1 << 20, 1, None)
        assert rc == 1001 and "null" in msg, (k, rc, msg)
        rc, msg = err(rk2, p[0], p[1], p[2], p[3], 2, 0.5, B, T, p[4], 1 << 20, 1, None)
        assert rc == 1001 and "null" in msg, (k, rc, msg)
    for bad in ((16, 1), (16, 0), (17, 9), (-3, 9)):  # 2 <= len <= T
        rc, msg = err(euler, one, one, one, lens_of(*bad), 4, B, T, one, 1 << 20, 1, None)
        assert rc == 1001 and "length" in msg, (bad, rc, msg)
        rc, msg = err(rk2, one, one, one, lens_of(*bad), 2, 0.5, B, T, one, 1 << 20, 1, None)
        assert rc == 1001 and "length" in msg, (bad, rc, msg)
    # the flamed_den_solve_rk2 checks, unchanged
    for nsteps in (0, -3):
        rc, msg = err(rk2, one, one, one, good, nsteps, 0.5, B, T, one, 1 << 20, 1, None)
        assert rc == 1001 and "nsteps" in msg, (rc, msg)
    for a in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        rc, msg = err(rk2, one, one, one, good, 2, a, B, T, one, 1 << 20, 1, None)
        assert rc == 1001 and "stage parameter" in msg, (a, rc, msg)
    for k in range(5):  # handle, cond, mask, out, workspace
        p = [one] * 5
        p[k] = None
        rc, msg = err(fold, p[0], p[1], p[2], B, T, p[3], p[4], 1 << 20, None)
        assert rc == 1001 and "flamed_cond_fold_exact" in msg, (k, rc, msg)


def test_ops_registered_with_fake_shapes():
    import types
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops
    for name in ("den_solve_lens", "den_solve_rk2_lens", "cond_fold_exact"):
        assert name in ops.OPS
    names = lambda op: [a.name for a in op.default._schema.arguments]
    assert names(torch.ops.flamed_hip.den_solve_lens) == ["oid", "xt", "ts", "spk", "nfe", "lens"]
    assert names(torch.ops.flamed_hip.den_solve_rk2_lens) == ["oid", "xt", "ts_eval", "spk", "nsteps", "a", "lens"]
    assert names(torch.ops.flamed_hip.cond_fold_exact) == ["oid", "cond", "mask"]
    assert "Int[] lens" in str(torch.ops.flamed_hip.den_solve_lens.default._schema)  # a list of ints (SymInt[])
    # the existing schemas are as they were
    assert names(torch.ops.flamed_hip.den_solve) == ["oid", "xt", "ts", "spk", "nfe"]
    assert names(torch.ops.flamed_hip.den_solve_rk2) == ["oid", "xt", "ts_eval", "spk", "nsteps", "a"]
    assert names(torch.ops.flamed_hip.cond_fold) == ["oid", "cond", "mask"]

    class Owner:
        pg = types.SimpleNamespace(target_dim=C)

    own = Owner()
    oid = ops.register(own)
    with FakeTensorMode():
        s = torch.ops.flamed_hip.den_solve_lens(1, torch.empty(2, 50, C), torch.empty(9), torch.empty(2, C), 8, [50, 31])
        assert s.shape == (2, 50, C) and s.dtype == torch.float32
        s = torch.ops.flamed_hip.den_solve_rk2_lens(1, torch.empty(2, 50, C), torch.empty(8), torch.empty(2, C), 4, 0.5, [50, 31])
        assert s.shape == (2, 50, C) and s.dtype == torch.float32
        c = torch.ops.flamed_hip.cond_fold_exact(oid, torch.empty(2, 6, 50, 384), torch.empty(2, 50, 1, dtype=torch.bool))
        assert c.shape == (2, 50, C) and c.dtype == torch.float32


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_sample_exact_cpu_vs_oracle_alone(pg_sd, solver):
    """lens 24 / 17 on the torch ops: each utterance against the oracle run on it alone (2e-5), the padding frames
    exactly 0, and utterance 1 far from what the default padded call gives it (the coupling this mode removes)."""
    pg, sd = pg_sd
    cond, spk, mask = _inputs(LENS)
    torch.manual_seed(11)
    noise = torch.randn((2, 24, C))  # the draw ProbGenerator.sample makes from the global CPU RNG
    with torch.inference_mode():
        torch.manual_seed(11)
        lat = pg.sample(cond, spk, mask, nfe=4, temperature=0.3, solver=solver, exact_lengths=True)
        torch.manual_seed(11)
        padded = pg.sample(cond, spk, mask, nfe=4, temperature=0.3, solver=solver)
    ref = alone_oracle(sd, cond, spk, noise, LENS, 4, 0.3, None if solver == "euler" else STAGE[solver])
    assert lat.shape == (2, C, 24)
    for u, n in enumerate(LENS):
        e = rel_l2(lat[u, :, :n], ref[u, :, :n])
        print(f"sample(exact_lengths=True) CPU {solver} utterance {u} (len {n}) vs oracle alone: rel-L2 {e:.3e}")
        assert e < TOL
        assert torch.count_nonzero(lat[u, :, n:]) == 0
    d = rel_l2(lat[1, :, :17], padded[1, :, :17])
    print(f"utterance 1: exact vs default padded call rel-L2 {d:.3e}")
    assert d > 1e-2


def test_fold_condition_exact_cpu(pg_sd):
    pg, sd = pg_sd
    cond, _, mask = _inputs(LENS)
    with torch.inference_mode():
        cf = pg.fold_condition(cond, mask, exact=True)
    assert cf.shape == (2, 24, C) and torch.count_nonzero(cf[1, 17:]) == 0
    for u, n in enumerate(LENS):
        ref = orc.cond_fold(sd, cond[u:u + 1, :, :n], torch.ones(1, n, 1, dtype=torch.bool))
        assert rel_l2(cf[u:u + 1, :n], ref) < TOL


def test_default_unchanged_and_errors(pg_sd):
    pg, _ = pg_sd
    cond, spk, mask = _inputs(LENS)
    with torch.inference_mode():
        torch.manual_seed(3)
        a = pg.sample(cond, spk, mask, nfe=4, temperature=0.3)
        torch.manual_seed(3)
        b = pg.sample(cond, spk, mask, nfe=4, temperature=0.3, exact_lengths=False)
        assert torch.equal(a, b)
        assert torch.equal(pg.fold_condition(cond, mask), pg.fold_condition(cond, mask, exact=False))
        hole = mask.clone()
        hole[1, 5] = False  # not a prefix mask
        with pytest.raises(ValueError, match="prefix mask"):
            pg.sample(cond, spk, hole, nfe=4, exact_lengths=True)
        pg.sample(cond, spk, hole, nfe=4)  # the default takes any mask, as before
        one = (torch.arange(24)[None, :] < torch.tensor([24, 1])[:, None]).unsqueeze(-1)
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            pg.sample(cond, spk, one, nfe=4, exact_lengths=True)


def test_cli_flag_namespace_default_and_names(tmp_path):
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed.utils.random_ckpt import write
    p = syn.build_arg_parser()
    base = ["--ckpt-path", "c", "--cfg-path", "g"]
    assert p.parse_args(base).exact_lengths is False
    assert p.parse_args(base + ["--exact-lengths", "true"]).exact_lengths is True
    assert p.parse_args(base + ["--exact-lengths", "False"]).exact_lengths is False
    paths = write(str(tmp_path / "ck"))
    _prompts(tmp_path / "pr")
    ns = dict(ckpt_path=paths["ckpt"], cfg_path=paths["cfg"], text="hello world.", prompt_list=["p0.wav"],
              prompt_dir=str(tmp_path / "pr"), metadata_file=None, output_dir=str(tmp_path / "out"), weights_only=True,
              nsteps_durgen=4, nsteps_denoiser=4, temp_durgen=0.3, temp_denoiser=0.3, device="cpu", skip_existing=True,
              batch_size=4, codec_ckpt_dir=str(tmp_path / "ck"))
    assert syn.main(argparse.Namespace(**ns)) > 0  # a hand-built Namespace without the field: off, the old name
    assert os.listdir(tmp_path / "out") == ["p0-4-4-0.3-0.3.wav"]
    assert syn.main(argparse.Namespace(**ns, exact_lengths=True)) > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["p0-4-4-0.3-0.3-exact.wav", "p0-4-4-0.3-0.3.wav"]
    assert syn.main(argparse.Namespace(**ns, exact_lengths=True, solver_denoiser="heun")) > 0
    assert "p0-4-4-0.3-0.3-heun-exact.wav" in os.listdir(tmp_path / "out")
    # metadata mode: the target directory carries the suffix
    meta = tmp_path / "meta.txt"
    meta.write_text("a.wav|p0.wav|hello world.\nb.wav|p0.wav|a much longer line of text to say.\n")
    ns2 = dict(ns, text=None, prompt_list=None, metadata_file=str(meta), output_dir=str(tmp_path / "out2"))
    assert syn.main(argparse.Namespace(**ns2, exact_lengths=True)) > 0
    assert os.listdir(tmp_path / "out2") == ["nfe4-temp0.3-exact"]
    assert sorted(os.listdir(tmp_path / "out2" / "nfe4-temp0.3-exact")) == ["a.wav", "b.wav"]


def test_sample_batch_passes_the_flag_through(monkeypatch):
    """Flamed.sample_batch(exact_lengths=...) reaches ProbGenerator.sample (the end-to-end fixture's ragged batch of
    two): the latents are 0 on the padding frames, the longest utterance is unchanged, the short one is not."""
    from _common import golden, t32
    from _flamed_common import build_flamed
    torch.set_num_threads(8)
    m, _ = build_flamed("cpu")
    g = golden("flamed_sample")
    seen = []
    real = m.prob_generator.sample

    def spy(*args, **kw):
        seen.append(kw.get("exact_lengths"))
        return real(*args, **kw)

    monkeypatch.setattr(m.prob_generator, "sample", spy)
    kw = dict(phonemes=t32(g["phonemes"]), src_lens=t32(g["src_lens"]), prompts=t32(g["prompts"]), timbres=t32(g["timbres"]),
              temp_durgen=0.3, temp_denoiser=0.3, nsteps_durgen=4, nsteps_denoiser=4)
    with torch.inference_mode():
        torch.manual_seed(int(g["rng_seed"]))
        exact = m.sample_batch(**kw, exact_lengths=True)
        torch.manual_seed(int(g["rng_seed"]))
        padded = m.sample_batch(**kw)
    assert seen == [True, False]
    pad = exact["tgt_mask"]  # True = padding frame
    lens = (~pad).sum(dim=1).tolist()
    assert min(lens) < max(lens) == pad.shape[1], lens
    lat, ref = exact["latents"].transpose(1, 2), padded["latents"].transpose(1, 2)  # (B, T, C)
    assert torch.count_nonzero(lat[pad]) == 0 and torch.count_nonzero(ref[pad]) > 0
    for u, n in enumerate(lens):
        d = rel_l2(lat[u, :n], ref[u, :n])
        assert d < TOL if n == max(lens) else d > 1e-2, (u, n, d)
