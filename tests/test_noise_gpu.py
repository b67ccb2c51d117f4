"""GPU: keyed noise (flamed_noise_state / flamed_noise_bits, flamed-tts_amd/csrc/noise.hip) against the test oracle of
tests/_noiseoracle.py -- the raw Philox words bit-exact, the state within
    |x - (cond + temp n)| <= 1e-5 |temp| + 2^-23 |x|
of the fp64 oracle (1e-5: fp32 log / sqrt / sincos against fp64, numpy's fp32 sits 1.33e-6 away; 2^-23 |x|: the one
rounding of the fmaf) -- the bitwise properties (a batch row is the call alone, a prefix is a prefix, padding is 0, the
vector and the scalar path agree), torch.library.opcheck, and the two stages that take seeds:
ProbGenerator.sample(seeds=) and Flamed.sample_batch(seeds=) with exact lengths, where an utterance then depends on
nothing but its own inputs and its seed."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _common import rel_l2
import _noiseoracle as no

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = [0, 1, 2**64 - 1, 0x0123456789ABCDEF]


def _hip(cond, seeds, lens, temp, stream, shape=None, out=None):
    from flamed.utils.noise import hip_noise_state
    x = hip_noise_state(cond, seeds, lens, temp, stream, shape=shape, device=DEV, out=out)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("first", [0, 4 * (2**32 - 2)], ids=["first0", "first-high-word"])
def test_noise_bits_bit_exact(first):
    """n = 1024 raw words; with first = 4 (2^32 - 2) the block index crosses 2^32 inside the range."""
    from flamed import _native as nat
    L = nat.lib()
    out = torch.empty(1024, dtype=torch.int32, device=DEV)
    for seed in SEEDS:
        for stream in (0, 1, 2):
            nat.check(L.flamed_noise_bits(seed, stream, first, 1024, nat.ptr(out), nat.stream_ptr(torch.device(DEV))),
                      "flamed_noise_bits")
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, no.words(seed, stream, first, 1024)), (hex(seed), stream)


CASES = [((3, 7, 256), [7, 2, 5]), ((1, 1, 4), None), ((2, 13, 1), [13, 6]), ((70, 3, 8), None)]


@pytest.mark.parametrize("shape,lens", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("mode", ["cond", "nocond", "inplace"])
def test_noise_state_vs_fp64_oracle(shape, lens, mode):
    """(2, 13, 1) takes the scalar path, (70, 3, 8) crosses the 64-utterance chunk (and has random lengths)."""
    B, T, C = shape
    g = torch.Generator().manual_seed(B * 1000 + T)
    if lens is None and B == 70:
        lens = [int(v) for v in torch.randint(1, T + 1, (B,), generator=g)]
    seeds = [no.utterance_seed(99, u) for u in range(B)]
    temp = 0.3
    cond = None if mode == "nocond" else torch.randn(B, T, C, generator=g)
    dc = None if cond is None else cond.to(DEV)
    x = _hip(dc, seeds, lens, temp, 0, shape=shape, out=dc if mode == "inplace" else None)
    if mode == "inplace":
        assert x.data_ptr() == dc.data_ptr()
    elif cond is not None:
        assert torch.equal(dc.cpu(), cond)  # the input is left alone
    ref = no.state(None if cond is None else cond.numpy(), seeds, lens, temp, 0, shape=shape)
    got = x.cpu().numpy().astype(np.float64)
    dev = np.abs(got - ref)
    bound = 1e-5 * abs(temp) + 2.0 ** -23 * np.abs(got)
    print(f"{shape} {mode}: largest deviation {dev.max():.3e} (largest excess over the bound {float((dev - bound).max()):.3e})")
    assert np.all(dev <= bound)
    if lens is not None:
        for u, n in enumerate(lens):
            assert np.count_nonzero(got[u, n:]) == 0, u


def test_bitwise_properties():
    seeds, lens, temp = [5, 2**64 - 9, 77], [7, 2, 5], 0.3
    cond = torch.randn(3, 7, 256, generator=torch.Generator().manual_seed(1)).to(DEV)
    x = _hip(cond, seeds, lens, temp, 0)
    assert torch.equal(x, _hip(cond, seeds, lens, temp, 0))  # two calls are equal
    for u, n in enumerate(lens):
        alone = _hip(cond[u:u + 1, :n].contiguous(), [seeds[u]], None, temp, 0)
        assert torch.equal(x[u:u + 1, :n], alone), u                     # a batch row is the call alone
        assert torch.count_nonzero(x[u, n:]) == 0                        # padding is exactly 0
    long = _hip(None, [seeds[0]], None, temp, 0, shape=(1, 9, 256))
    assert torch.equal(long[:, :4], _hip(None, [seeds[0]], None, temp, 0, shape=(1, 4, 256)))  # a prefix is a prefix
    assert torch.equal(long[:, :4], _hip(None, [seeds[0]], [4], temp, 0, shape=(1, 9, 256))[:, :4])
    assert not torch.equal(x[0, :2], x[2, :2])
    assert not torch.equal(long, _hip(None, [seeds[0]], None, temp, 1, shape=(1, 9, 256)))
    # the vector path (C = 4) and the scalar path (C = 1, odd length) on the same elements of one utterance
    c4 = torch.randn(1, 5, 4, generator=torch.Generator().manual_seed(2))
    v = _hip(c4.to(DEV), [seeds[1]], [3], temp, 2)
    s = _hip(c4.reshape(1, 20, 1)[:, :19].contiguous().to(DEV), [seeds[1]], [12], temp, 2)
    assert torch.equal(v.reshape(-1)[:19], s.reshape(-1)) and torch.count_nonzero(s[0, 12:]) == 0
    # a misaligned view of an aligned buffer takes the scalar path too
    buf = torch.zeros(1 + 7 * 256, device=DEV)
    o = buf[1:].view(1, 7, 256)
    _hip(None, [seeds[0]], None, temp, 0, shape=(1, 7, 256), out=o)
    assert torch.equal(o, long[:, :7]) and float(buf[0]) == 0.0


def test_opcheck():
    from flamed import ops  # noqa: F401
    cond = torch.randn(3, 7, 256, device=DEV)
    for args in ((cond, [1, -2, 3], [7, 2, 5], 0.3, 0, 3, 7, 256, torch.device(DEV)),
                 (None, [4, 5], None, 0.5, 1, 2, 13, 1, torch.device(DEV))):
        torch.library.opcheck(torch.ops.flamed_hip.noise_state.default, args)
    a = torch.ops.flamed_hip.noise_state(None, [-1], None, 1.0, 0, 1, 2, 4, torch.device(DEV))  # -1 is seed 2^64 - 1
    assert torch.equal(a, _hip(None, [2**64 - 1], None, 1.0, 0, shape=(1, 2, 4)))


@pytest.fixture(scope="module")
def pgb():
    from test_denoiser_gpu import _prob_gen
    return _prob_gen("bf16")


@pytest.mark.parametrize("solver", ["euler", "midpoint"])
def test_sample_with_seeds_exact_lengths(pgb, solver):
    """ProbGenerator.sample(seeds=, exact_lengths=True), bf16 handle, lens (100, 37, 64), nfe 8: every utterance against
    the same call made alone with its seed (VS_LAUNCH of tests/test_exact_lengths_gpu.py) and against the oracle alone
    started from THIS file's oracle noise (that file's bf16 bars); the initial state bitwise in and out of the batch;
    the global RNG untouched."""
    from flamed.utils.noise import noise_state
    from test_exact_lengths_cpu import alone_oracle
    from test_exact_lengths_gpu import NFE, _check_vs_oracle
    from test_rk2_cpu import STAGE
    from test_rk2_gpu import VS_LAUNCH
    pg, sd = pgb
    lens, C, temp = [100, 37, 64], 256, 0.3
    B, T = len(lens), max(lens)
    seeds = [no.utterance_seed(20251205, u) for u in range(B)]
    g = torch.Generator().manual_seed(sum(lens))
    cond = torch.randn(B, 6, T, 384, generator=g)
    spk = torch.randn(B, C, generator=g)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    dc, ds, dm = cond.to(DEV), spk.to(DEV), mask.to(DEV)
    state = torch.get_rng_state()
    with torch.inference_mode():
        lat = pg.sample(dc, ds, dm, nfe=NFE, temperature=temp, solver=solver, exact_lengths=True, seeds=seeds)
        folded = pg.fold_condition(dc, dm, exact=True)
        x0 = noise_state(folded, seeds, lens, temp, 0)
        for u, n in enumerate(lens):
            alone = pg.sample(dc[u:u + 1, :, :n], ds[u:u + 1], dm[u:u + 1, :n], nfe=NFE, temperature=temp, solver=solver,
                              exact_lengths=True, seeds=[seeds[u]])
            e = rel_l2(lat[u:u + 1, :, :n].cpu(), alone.cpu())
            print(f"{solver} utterance {u} (len {n}): in the batch vs alone rel-L2 {e:.3e}")
            assert e < VS_LAUNCH, (u, e)
            assert torch.equal(x0[u:u + 1, :n], noise_state(folded[u:u + 1, :n].contiguous(), [seeds[u]], None, temp, 0))
            assert torch.count_nonzero(x0[u, n:]) == 0 and torch.count_nonzero(lat[u, :, n:]) == 0
    assert torch.equal(state, torch.get_rng_state())
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    noise = torch.zeros(B, T, C)
    for u, n in enumerate(lens):
        noise[u, :n] = torch.from_numpy(no.normals(seeds[u], 0, n * C)).float().reshape(n, C)
    ref = alone_oracle(sd, cond, spk, noise, lens, NFE, temp, None if solver == "euler" else STAGE[solver])
    lat = lat.cpu()
    for u, n in enumerate(lens):
        _check_vs_oracle(lat[u, :, :n], ref[u, :, :n], n, f"sample(seeds) {solver} utterance {u} (len {n})")


E2E_NOISE_SEED = 4


def test_sample_batch_with_seeds_is_batch_independent():
    """Flamed.sample_batch(seeds=, exact_lengths=True, exact_prior=True) on the small fixture model of
    tests/test_prior_exact_gpu.py::test_sample_batch_exact_prior_end_to_end: the batch [A, B, C] against [C, A] and [B]
    run separately with the same per-utterance seeds utterance_seed(4, index) -- equal frame counts (tgt_mask), latents
    within VS_LAUNCH, the global RNG untouched.

    Seed 4 was picked on the CPU path (the oracle's flow of every utterance alone, from the oracle noise of streams 1
    and 2, tests/_priorexact.flow_alone): no position of the six log-duration vectors lies within 1e-4 of a .5 rounding
    boundary (near_and_flips counts 0; the closest is 5.2e-3 away), so a last-bit difference between two batch shapes
    cannot flip a frame count.  The check runs again here (it is the cheap part of the oracle)."""
    import _priorexact as px
    from _common import orc
    from _flamed_common import build_flamed
    from test_prior_exact_gpu import E2E_NFE, e2e_inputs
    from test_rk2_gpu import VS_LAUNCH
    m, _ = build_flamed(DEV, "bf16")
    phonemes, src, prompts, timbres = e2e_inputs()
    B, L = phonemes.shape
    seeds = [no.utterance_seed(E2E_NOISE_SEED, u) for u in range(B)]
    sd = {"prior_generator." + k: v.detach().float().cpu() for k, v in m.prior_generator.state_dict().items()}
    lens = src.tolist()
    dn, sn = torch.zeros(B, L), torch.zeros(B, L)
    for u, n in enumerate(lens):
        dn[u, :n] = torch.from_numpy(no.normals(seeds[u], 1, n)).float()
        sn[u, :n] = torch.from_numpy(no.normals(seeds[u], 2, n)).float()
    with torch.inference_mode():
        enc = orc.prior_encoder(sd, phonemes, orc.mask_from_lengths(src, L))
    flow = px.flow_alone(sd, enc, lens, dn, sn, E2E_NFE, 0.3)
    assert sum(px.near_and_flips(r, r)[0] for f in flow for r in f) == 0
    tgt = [t for _, t in px.lr_alone(enc, [f[0] for f in flow], [f[1] for f in flow], lens)]

    def run(idx):
        i = torch.tensor(idx)
        return m.sample_batch(phonemes=phonemes[i], src_lens=src[i], prompts=prompts[i], timbres=timbres[i], temp_durgen=0.3,
                              temp_denoiser=0.3, nsteps_durgen=E2E_NFE, nsteps_denoiser=8, exact_lengths=True,
                              exact_prior=True, seeds=[seeds[u] for u in idx])

    state = torch.get_rng_state()
    full, ca, b = run([0, 1, 2]), run([2, 0]), run([1])
    assert torch.equal(state, torch.get_rng_state())
    counts = (~full["tgt_mask"]).sum(-1).tolist()
    assert counts == tgt, (counts, tgt)  # ... and they are the oracle's frame counts of every utterance alone
    for out, idx in ((ca, [2, 0]), (b, [1])):
        assert (~out["tgt_mask"]).sum(-1).tolist() == [counts[u] for u in idx]
        for k, u in enumerate(idx):
            n = counts[u]
            e = rel_l2(out["latents"][k, :, :n].cpu(), full["latents"][u, :, :n].cpu())
            print(f"utterance {u} ({n} frames): batch {idx} vs batch [0, 1, 2] latents rel-L2 {e:.3e}")
            assert e < VS_LAUNCH, (idx, u, e)
            assert torch.count_nonzero(out["latents"][k, :, n:]) == 0
    # other seeds, other durations and latents
    other = m.sample_batch(phonemes=phonemes, src_lens=src, prompts=prompts, timbres=timbres, temp_durgen=0.3,
                           temp_denoiser=0.3, nsteps_durgen=E2E_NFE, nsteps_denoiser=8, exact_lengths=True, exact_prior=True,
                           seeds=[s ^ 1 for s in seeds])
    assert other["latents"].shape != full["latents"].shape or not torch.equal(other["latents"], full["latents"])
