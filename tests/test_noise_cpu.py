"""Keyed noise, CPU side (tests/_noiseoracle.py states the definition; the oracle there does not import
flamed/utils/noise.py): the Philox and seed known answers, the numpy back end against the oracle, the bitwise prefix /
batch-independence properties, the moments, the opt-in (seeds=None is the parent's draw, bit for bit), the C entry
points' host-side validation, and `synthesize.py --noise utterance` on --device cpu."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _common import PKG
import _noiseoracle as no

from flamed.utils import noise as fn

SEEDS = [0, 1, 20251205, 2**63 + 12345]


def test_philox_known_answers():
    for ctr, key, out in no.KNOWN:
        assert tuple(int(v) for v in no.philox(*ctr, *key)[0]) == out
    # the product's numpy Philox takes (block, stream, seed): counter word 3 is 0 by definition, so the first answer
    assert tuple(int(v) for v in fn.philox4x32_10(np.zeros(1, dtype=np.uint64), 0, 0)[0]) == no.KNOWN[0][2]


def test_utterance_seed_against_pure_python():
    for seed in (0, 1, 2**64 - 1):
        for index in (0, 1, 10**6):
            z = (seed + 0x9E3779B97F4A7C15 * (index + 1)) & no.M64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & no.M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & no.M64
            z ^= z >> 31
            assert fn.utterance_seed(seed, index) == z == no.utterance_seed(seed, index)
            assert 0 <= z < 2**64
    assert fn.utterance_seeds(7, [2, 0]) == [fn.utterance_seed(7, 2), fn.utterance_seed(7, 0)]
    assert len({fn.utterance_seed(7, i) for i in range(1000)}) == 1000


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_cpu_backend_against_the_oracle(stream):
    """Integer words exact; normals within 1e-5 max abs of the fp64 oracle (numpy fp32 sits 1.33e-6 from it)."""
    worst = 0.0
    for seed in SEEDS + [2**64 - 1]:
        assert np.array_equal(fn.philox4x32_10(np.arange(300, dtype=np.uint64), stream, seed),
                              no.block_words(seed, stream, 300))
        got = fn.keyed_normal([seed], None, 37, 33, stream)  # 1221 elements: not a multiple of 4
        assert got.dtype == torch.float32 and got.shape == (1, 37, 33)
        d = float(np.abs(got.numpy().reshape(-1).astype(np.float64) - no.normals(seed, stream, 37 * 33)).max())
        worst = max(worst, d)
    print(f"stream {stream}: CPU back end vs the fp64 oracle max abs {worst:.3e}")
    assert worst <= 1e-5
    # the block index above 2^32 (the high counter word)
    big = np.array([2**32 - 1, 2**32, 2**40 + 5], dtype=np.uint64)
    ref = no.philox([int(b) % 2**32 for b in big], [int(b) >> 32 for b in big], stream, 0, 5, 0)
    assert np.array_equal(fn.philox4x32_10(big, stream, 5), ref)


def test_prefix_and_batch_independence_bitwise():
    seeds, lens = [11, 2**64 - 3, 12], [7, 2, 5]
    full = fn.keyed_normal(seeds, lens, 7, 256, 0)
    for u, n in enumerate(lens):
        alone = fn.keyed_normal([seeds[u]], None, n, 256, 0)
        assert torch.equal(full[u:u + 1, :n], alone), u
        assert torch.count_nonzero(full[u, n:]) == 0
        assert torch.equal(fn.keyed_normal([seeds[u]], None, 7, 256, 0)[:, :n], alone)  # a prefix is a prefix
    assert not torch.equal(full[0, :2], full[2, :2])                       # two seeds differ
    assert not torch.equal(full[0], fn.keyed_normal(seeds[:1], None, 7, 256, 1)[0])  # two streams differ
    # the state: cond + temperature n, 0 behind the length, and the same bits in and out of a batch
    cond = torch.randn(3, 7, 256, generator=torch.Generator().manual_seed(3))
    x = fn.noise_state(cond, seeds, lens, 0.3, 0)
    for u, n in enumerate(lens):
        assert torch.equal(x[u:u + 1, :n], fn.noise_state(cond[u:u + 1, :n].contiguous(), [seeds[u]], None, 0.3, 0))
        assert torch.count_nonzero(x[u, n:]) == 0
    ref = no.state(cond.numpy(), seeds, lens, 0.3, 0)
    assert float(np.abs(x.numpy() - ref).max()) <= 1e-5 * 0.3 + 2.0 ** -23 * float(np.abs(ref).max())
    pv = fn.noise_state(None, seeds, [5, 3, 1], 0.3, 2, shape=(3, 5, 1))
    assert pv.shape == (3, 5, 1) and torch.count_nonzero(pv[1, 3:]) == 0
    assert torch.equal(pv[1, :3], fn.noise_state(None, seeds[1:2], None, 0.3, 2, shape=(1, 3, 1))[0])


@pytest.mark.parametrize("seed", SEEDS)
def test_moments(seed):
    """102 400 normals: four standard errors (the oracle itself gives at most 0.0042, 0.0075, 0.056)."""
    z = fn.keyed_normal([seed], None, 400, 256, 0).double().reshape(-1)
    m, v, k = float(z.mean()), float(z.var(unbiased=False)), float((z ** 4).mean())
    print(f"seed {seed}: mean {m:.4f} var {v:.4f} E z^4 {k:.4f} max |z| {float(z.abs().max()):.3f}")
    assert abs(m) < 0.0125 and abs(v - 1) < 0.0177 and abs(k - 3) < 0.122
    assert float(z.abs().max()) <= 5.77


def _prob_gen():
    import yaml
    from flamed.models.synthesizer.prob_generator import ProbGenerator
    from flamed.utils.seeded_init import randomize_module
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prob.yaml")))
    pg = ProbGenerator(cfg).eval()
    randomize_module(pg, 7)
    return pg


def test_opt_in_prob_generator():
    """seeds=None: the parent's draw (torch.randn((B, T, C)) from the global CPU RNG), bitwise, consuming the RNG
    identically.  With seeds the global RNG is untouched and an utterance does not depend on its batch."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    pg = _prob_gen()
    g = torch.Generator().manual_seed(5)
    lens, B, T = [9, 6], 2, 9
    cond, spk = torch.randn(B, 6, T, 384, generator=g), torch.randn(B, 256, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    with torch.inference_mode():
        torch.manual_seed(3)
        a = pg.sample(cond, spk, mask, nfe=2, temperature=0.3)
        after = torch.get_rng_state()
        torch.manual_seed(3)
        noise = torch.randn((B, T, 256))
        assert torch.equal(after, torch.get_rng_state())
        x0 = noise * 0.3 + pg.fold_condition(cond, mask)
        ts = torch.linspace(0, 1, 3)
        assert torch.equal(a, pg._euler_torch(x0, ts, spk, 2).transpose(1, -1))
        assert torch.equal(a, pg.sample(cond, spk, mask, nfe=2, temperature=0.3, seeds=None)) is False  # the RNG moved on
        torch.manual_seed(3)
        assert torch.equal(a, pg.sample(cond, spk, mask, nfe=2, temperature=0.3, seeds=None))
        st = torch.get_rng_state()
        for solver in ("euler", "midpoint"):
            both = pg.sample(cond, spk, mask, nfe=2, temperature=0.3, solver=solver, exact_lengths=True, seeds=[4, 9])
            padded = pg.sample(cond, spk, mask, nfe=2, temperature=0.3, solver=solver, seeds=[4, 9])
            assert padded.shape == both.shape == (B, 256, T)
            for u, n in enumerate(lens):
                alone = pg.sample(cond[u:u + 1, :, :n], spk[u:u + 1], mask[u:u + 1, :n], nfe=2, temperature=0.3,
                                  solver=solver, exact_lengths=True, seeds=[[4, 9][u]])
                assert torch.equal(both[u:u + 1, :, :n], alone), (solver, u)  # CPU exact path: each alone, so bitwise
                assert torch.count_nonzero(both[u, :, n:]) == 0
        assert torch.equal(st, torch.get_rng_state())
        with pytest.raises(ValueError):
            pg.sample(cond, spk, mask, nfe=2, seeds=[1])


def test_opt_in_pva():
    import yaml
    from flamed.models.synthesizer.pva import PVA
    from flamed.utils.seeded_init import randomize_module
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "prior.yaml")))
    pva = PVA(cfg["variance_adaptor"]).eval()
    randomize_module(pva, 7)
    g = torch.Generator().manual_seed(1)
    B, L, lens = 2, 7, [7, 4]
    H = pva.duration_generator.input_size
    x = torch.randn(B, L, H, generator=g)
    mask = ~(torch.arange(L)[None, :] < torch.tensor(lens)[:, None])
    with torch.inference_mode():
        torch.manual_seed(8)
        d0, s0 = pva.flow(x, mask, 2, 0.3)
        after = torch.get_rng_state()
        torch.manual_seed(8)
        torch.randn((B, L)), torch.randn((B, L))
        assert torch.equal(after, torch.get_rng_state())
        torch.manual_seed(8)
        d1, s1 = pva.flow(x, mask, 2, 0.3, seeds=None)
        assert torch.equal(d0, d1) and torch.equal(s0, s1)
        st = torch.get_rng_state()
        d, s = pva.flow(x, mask, 2, 0.3, exact=True, seeds=[21, 22])
        assert torch.equal(st, torch.get_rng_state())
        assert not torch.equal(d, s)
        for u, n in enumerate(lens):
            da, sa = pva.flow(x[u:u + 1, :n], mask[u:u + 1, :n], 2, 0.3, exact=True, seeds=[[21, 22][u]])
            assert torch.equal(d[u, :n], da[0]) and torch.equal(s[u, :n], sa[0])
            assert torch.count_nonzero(d[u, n:]) == 0 and torch.count_nonzero(s[u, n:]) == 0
        dp, _ = pva.flow(x, mask, 2, 0.0, seeds=[21, 22])  # padded mode takes seeds too
        assert dp.shape == (B, L)


def test_c_abi_validation_without_a_gpu():
    """Declared, bound, mapped; bad arguments give 1001 and a message before any HIP call (no GPU here)."""
    from flamed import _native as nat
    root = os.path.dirname(PKG)
    hdr = open(os.path.join(root, "include", "flamed_hip.h")).read()
    diag = open(os.path.join(root, "include", "flamed_diag.h")).read()
    assert "FLAMED_API int flamed_noise_state(" in hdr and "flamed_noise_state" in nat.SIGNATURES
    assert "flamed_noise_state" in open(os.path.join(root, "INTEGRATION.md")).read()
    assert "FLAMED_API int flamed_noise_bits(" in diag.split("---- libflamed_hip.so diagnostics ----")[1]
    assert "flamed_noise_bits" in nat.HIP_DIAG_SIGNATURES
    L = nat.lib()
    one = ctypes.c_void_p(64)  # never dereferenced: validation comes first
    seeds = (ctypes.c_ulonglong * 2)(1, 2)

    def call(cond, sd, lens, stream, B, T, C, x):
        la = None if lens is None else (ctypes.c_int * len(lens))(*lens)
        rc = L.flamed_noise_state(cond, sd, la, stream, 0.3, B, T, C, x, None)
        return rc, L.flamed_last_error().decode()

    for args in ((None, seeds, None, 0, 0, 4, 4, one), (None, seeds, None, 0, 2, 0, 4, one), (None, seeds, None, 0, 2, 4, 0, one),
                 (None, seeds, [4, 0], 0, 2, 4, 4, one), (None, seeds, [5, 1], 0, 2, 4, 4, one), (None, seeds, None, 0, 2, 4, 4, None),
                 (None, None, None, 0, 2, 4, 4, one), (None, seeds, None, -1, 2, 4, 4, one)):
        rc, msg = call(*args)
        assert rc == 1001 and "flamed_noise_state" in msg, (args, rc, msg)
    assert L.flamed_noise_bits(0, 0, 0, 0, one, None) == 1001 and L.flamed_noise_bits(0, 0, 0, 4, None, None) == 1001
    for bad in (dict(seeds=[1]), dict(seeds=[1, 2**64]), dict(seeds=[1, -1]), dict(seeds=[1, 2], lens=[3, 9])):
        kw = dict(seeds=[1, 2], lens=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            fn.noise_state(torch.zeros(2, 4, 4), kw["seeds"], kw["lens"], 0.3, 0)


def test_op_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops  # noqa: F401
    assert str(torch.ops.flamed_hip.noise_state.default._schema).startswith("flamed_hip::noise_state(")
    with FakeTensorMode():
        x = torch.ops.flamed_hip.noise_state(torch.empty(3, 7, 256), [1, -2, 3], [7, 2, 5], 0.3, 0, 3, 7, 256, torch.device("cpu"))
        assert x.shape == (3, 7, 256) and x.dtype == torch.float32
        y = torch.ops.flamed_hip.noise_state(None, [1], None, 0.3, 1, 1, 5, 1, torch.device("cpu"))
        assert y.shape == (1, 5, 1)


def test_cli_noise_utterance(tmp_path):
    """`--noise utterance --seed 7 --exact-lengths true --exact-prior true` on --device cpu with the seeded random
    checkpoint: a three-line metadata file at --batch-size 1 and 3, at 2 with the lines of the batches in another
    order, and one line re-run alone through --skip-existing.

    The bar.  The CPU exact paths are NOT bitwise across batch shapes: the prior text encoder runs the padded batch on
    torch ops (masked attention), whose GEMMs block differently at B = 1 and B = 3.  So across batch sizes this test
    uses the bar of the existing exact CPU test of the CLI (tests/test_prior_exact_cpu.py::
    test_cli_flag_suffix_and_batch_independent_files): every file holds the same number of samples in every run -- here
    at duration temperature 0.3, which that test could only ask at temperature 0 because the global draw of a batch of
    two is not the draw of a batch of one.  The largest sample difference is printed.  Where the batch shape is the
    same -- a line re-run alone against the --batch-size 1 run -- the file is BITWISE the same.

    The reordering is applied to the batches, not to the file: a line's seed is utterance_seed(S, its index among the
    file's non-empty lines) by definition, so moving a line inside the FILE gives it another seed and another waveform
    on purpose.  What must not matter is where in a batch (and in which batch) the line is synthesized, so the batches
    are permuted after the indices are taken, which is what sharding over GPUs does."""
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed.utils.audio import write_wav
    from flamed.utils.random_ckpt import write
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    paths = write(str(tmp_path / "ck"))
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "pr")
    for i in range(2):
        write_wav(str(tmp_path / "pr" / f"p{i}.wav"), rng.normal(0, 0.1, 4000 + 2400 * i).astype(np.float32))
    meta = tmp_path / "meta.txt"
    meta.write_text("u0.wav|p0.wav|hello world.\n\nu1.wav|p1.wav|good morning to you all.\nu2.wav|p0.wav|a third one.\n")
    parser = syn.build_arg_parser()
    assert parser.parse_args(["--ckpt-path", "c", "--cfg-path", "g"]).noise == "global"
    assert syn._solver_suffix("heun", True, True, 7) == "-heun-exact-xprior-seed7" and syn._solver_suffix("euler") == ""

    def run(name, batch, *extra):
        args = parser.parse_args([
            "--ckpt-path", paths["ckpt"], "--cfg-path", paths["cfg"], "--codec-ckpt-dir", str(tmp_path / "ck"),
            "--metadata-file", str(meta), "--prompt-dir", str(tmp_path / "pr"), "--output-dir", str(tmp_path / name),
            "--device", "cpu", "--nsteps-durgen", "4", "--nsteps-denoiser", "2", "--exact-lengths", "true",
            "--exact-prior", "true", "--batch-size", str(batch), *extra])
        assert syn.main(args) is not None
        d = tmp_path / name / "nfe2-temp0.3-exact-xprior-seed7"
        return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}

    keyed = ("--noise", "utterance", "--seed", "7")
    orig, seen = syn.Flamed.sample_batch, []

    def spy(self, **kw):  # synthesis itself (model construction draws its initial weights) leaves the global RNG alone
        state = torch.get_rng_state()
        out = orig(self, **kw)
        seen.append((kw["seeds"], torch.equal(state, torch.get_rng_state())))
        return out

    syn.Flamed.sample_batch = spy
    try:
        one = run("b1", 1, *keyed)
    finally:
        syn.Flamed.sample_batch = orig
    assert [s for s, _ in seen] == [[no.utterance_seed(7, i)] for i in range(3)] and all(ok for _, ok in seen)
    assert sorted(one) == ["u0.wav", "u1.wav", "u2.wav"]
    assert len({len(v) for v in one.values()}) > 1 and one["u0.wav"] != one["u2.wav"]

    def same_counts(name, got):
        assert sorted(got) == sorted(one), name
        for f in sorted(one):
            assert len(got[f]) == len(one[f]), (name, f, len(got[f]), len(one[f]))
            x, y = (np.frombuffer(v[44:], dtype="<i2").astype(np.int64) for v in (got[f], one[f]))
            print(f"{name} {f}: {len(x)} samples, max |d| vs --batch-size 1 {int(np.abs(x - y).max())} of 32767")

    same_counts("batch 3", run("b3", 3, *keyed))
    chunked = syn.chunked
    syn.chunked = lambda seq, size: chunked(list(seq)[::-1], size)
    try:
        same_counts("batch 2 reversed", run("b2r", 2, *keyed))
    finally:
        syn.chunked = chunked
    os.remove(tmp_path / "b1" / "nfe2-temp0.3-exact-xprior-seed7" / "u1.wav")
    assert run("b1", 3, *keyed, "--skip-existing", "true") == one  # only u1 is synthesized again, alone: bitwise
    # another seed is another waveform; the mode needs a seed
    meta.write_text("u0.wav|p0.wav|hello world.\n")
    other = parser.parse_args([
        "--ckpt-path", paths["ckpt"], "--cfg-path", paths["cfg"], "--codec-ckpt-dir", str(tmp_path / "ck"),
        "--metadata-file", str(meta), "--prompt-dir", str(tmp_path / "pr"), "--output-dir", str(tmp_path / "s8"),
        "--device", "cpu", "--nsteps-durgen", "4", "--nsteps-denoiser", "2", "--exact-lengths", "true",
        "--exact-prior", "true", "--noise", "utterance", "--seed", "8"])
    syn.main(other)
    assert open(tmp_path / "s8" / "nfe2-temp0.3-exact-xprior-seed8" / "u0.wav", "rb").read() != one["u0.wav"]
    other.seed = None
    with pytest.raises(ValueError, match="--noise utterance needs --seed"):
        syn.main(other)
