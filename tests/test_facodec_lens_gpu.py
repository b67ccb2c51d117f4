"""GPU: the HIP FaCodec decode with exact lengths (flamed_fac_decode_lens through FACodecDecoder.inference(x, spk, lens))
against each utterance decoded alone by the oracle; tests/_faclens.py has the definition, the bars and the shapes.
f32 and bf16 handles, calm weights.  test_facodec_lens_cpu.py::test_calibration_* shows what these tests see of a decode
that runs over the padded batch and trims: 41-91 x the bf16 bar in the last ~14 frames of every shorter utterance.

Measured HIP / floor worst-window ratios (bf16, bar 1.4) and f32 worst windows (bar 2e-5) are recorded in DESIGN.md
"Exact lengths"."""
import pytest
import torch

from _common import golden, t32
from _faclens import HOP, SHAPES, alone, case, check_batch, inputs, make_decoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["f32", "bf16"]
PAD_SHAPES = [(3, 13, (13, 7, 2)), (2, 32, (32, 19))]


@pytest.fixture(scope="module")
def decs():
    return {m: make_decoder(m, DEV) for m in MODES}


def _run(dec, lat, spk, lens=None):
    with torch.inference_mode():
        return dec.inference(lat.to(DEV), spk.to(DEV), lens).cpu()


@pytest.mark.parametrize("B,T,lens", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_parity_each_utterance_alone(decs, mode, B, T, lens):
    lat, spk, refs = case(B, T, lens)
    wav = _run(decs[mode], lat, spk, list(lens))
    assert wav.shape == (B, 1, HOP * T)
    check_batch(mode, wav, lens, refs, f"lens {B}x{T} {'/'.join(map(str, lens))}")


@pytest.mark.parametrize("B,T,lens", PAD_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_padding_is_never_read(decs, mode, B, T, lens):
    """0, 100 x randn, NaN and inf behind every end: the four outputs are bitwise equal, as whole tensors."""
    lat, spk, _ = case(B, T, lens)
    noise = 100 * torch.randn(lat.shape, generator=torch.Generator().manual_seed(3))
    outs = []
    for fill in (torch.zeros_like(lat), noise, torch.full_like(lat, float("nan")), torch.full_like(lat, float("inf"))):
        x = lat.clone()
        for u, n in enumerate(lens):
            x[u, :, n:] = fill[u, :, n:]
        outs.append(_run(decs[mode], x, spk, list(lens)))
    assert torch.isfinite(outs[0]).all()
    for k in (1, 2, 3):
        assert torch.equal(outs[0], outs[k]), f"padding fill {k} changed the output"


@pytest.mark.parametrize("B,T,lens", PAD_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_neighbours(decs, mode, B, T, lens):
    """Utterance 1 replaced -- latents, speaker row and length: the other utterances are bitwise unchanged."""
    lat, spk, _ = case(B, T, lens)
    lat2, spk2 = inputs(B, T, seed=1)
    latb, spkb, lensb = lat.clone(), spk.clone(), list(lens)
    latb[1], spkb[1], lensb[1] = lat2[1], spk2[1], lens[1] + 4
    a, b = _run(decs[mode], lat, spk, list(lens)), _run(decs[mode], latb, spkb, lensb)
    assert not torch.equal(a[1], b[1])
    assert torch.count_nonzero(b[1, :, HOP * lensb[1]:]) == 0 and torch.count_nonzero(b[1, :, HOP * lens[1]:HOP * lensb[1]]) > 0
    for u in range(B):
        if u != 1:
            assert torch.equal(a[u], b[u]), f"utterance {u} changed with its neighbour"


@pytest.mark.parametrize("B,T,lens", PAD_SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_dense_identity(decs, mode, B, T, lens):
    """lens = [T] * B is the dense call bitwise, graph on and off; the dense call is the same before and after a
    ragged call on the same handle."""
    d = decs[mode]
    lat, spk, _ = case(B, T, lens)
    try:
        for graph in (True, False):
            d.hip_graph = graph
            before = _run(d, lat, spk)
            assert torch.equal(_run(d, lat, spk, [T] * B), before), f"graph={graph}"
            ragged = _run(d, lat, spk, list(lens))
            assert not torch.equal(ragged, before)
            assert torch.equal(_run(d, lat, spk), before), f"graph={graph}: dense call moved after a ragged one"
            assert torch.equal(_run(d, lat, spk, torch.tensor([T] * B)), before)
    finally:
        d.hip_graph = True


@pytest.mark.parametrize("mode", MODES)
def test_graph_replay_and_stale_state(decs, mode):
    """One handle, graph on then off: dense (3, 41) -> (3, 13, 13/7/2) -> (3, 13, 5/13/9) -> dense (3, 13) ->
    (3, 13, 13/7/2).  The last equals the second bitwise (a replay sees its own call's lengths; rows past an end keep
    whatever an earlier, larger or denser decode left there and are never read); the third meets the bars for its
    own lengths."""
    d = decs[mode]
    lat, spk, _ = case(3, 13, (13, 7, 2))
    big = inputs(3, 41, seed=2)
    lens3 = (5, 13, 9)
    _, _, refs3 = case(3, 13, lens3)
    try:
        for graph in (True, False):
            d.hip_graph = graph
            _run(d, big[0], big[1])
            second = _run(d, lat, spk, [13, 7, 2])
            third = _run(d, lat, spk, list(lens3))
            _run(d, lat, spk)
            last = _run(d, lat, spk, [13, 7, 2])
            assert torch.equal(second, last), f"graph={graph}"
            check_batch(mode, third, lens3, refs3, f"sequence graph={graph} 3x13 5/13/9")
    finally:
        d.hip_graph = True


@pytest.mark.parametrize("mode", MODES)
def test_graph_recaptured_after_tune(decs, mode):
    """A knob the captured launches bake in (small_stages, read by launch_gemm) changes between calls of one shape and
    goes back: graph on == graph off bitwise under the new knob, and both calls equal their first results once it is
    restored.  This checks only that results do not move.  It cannot tell a re-capture from the replay of a graph
    captured under the old knob: the stage count changes no bit of a GEMM's result (same K order), so the test passes
    on a library whose graph keys lack the tune epoch too."""
    from test_persist_gpu import knob
    d = decs[mode]
    B, T, lens = 2, 13, [13, 7]
    lat, spk = inputs(B, T)
    try:
        d.hip_graph = True
        first = _run(d, lat, spk), _run(d, lat, spk, lens)
        with knob("small_stages", 5, 3):
            on = _run(d, lat, spk), _run(d, lat, spk, lens)
            d.hip_graph = False
            off = _run(d, lat, spk), _run(d, lat, spk, lens)
            d.hip_graph = True
        for k, what in enumerate(("dense", "ragged")):
            assert torch.equal(on[k], off[k]), f"{what}: graph on differs from graph off under the new knob"
        again = _run(d, lat, spk), _run(d, lat, spk, lens)
        for k, what in enumerate(("dense", "ragged")):
            assert torch.equal(again[k], first[k]), f"{what}: moved after the knob was restored"
    finally:
        d.hip_graph = True


@pytest.mark.parametrize("mode", MODES)
def test_determinism(decs, mode):
    lat, spk, _ = case(4, 9, (9, 1, 5, 8))
    assert torch.equal(_run(decs[mode], lat, spk, [9, 1, 5, 8]), _run(decs[mode], lat, spk, [9, 1, 5, 8]))


def test_opcheck_fac_decode_lens(decs):
    d = decs["f32"]
    lat, spk = inputs(3, 13)
    x, s = lat.to(DEV), spk.to(DEV)
    with torch.inference_mode():
        d.inference(x, s, [13, 7, 2])  # creates the owner
    torch.library.opcheck(torch.ops.flamed_hip.fac_decode_lens.default, (d._hip.oid, x, s, [13, 7, 2]),
                          test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("mode", MODES)
def test_sample_batch_exact_lengths_decodes_each_alone(decs, mode):
    """Flamed.sample_batch(exact_lengths=True) on the device, the end-to-end fixture's ragged batch: every waveform
    up to wav_lens meets the mode's bars against the oracle decode of that utterance's own latents alone; 0 after."""
    from _flamed_common import build_flamed
    m, _ = build_flamed(DEV, mode)
    g = golden("flamed_sample")
    with torch.inference_mode():
        torch.manual_seed(int(g["rng_seed"]))
        out = m.sample_batch(phonemes=t32(g["phonemes"]), src_lens=t32(g["src_lens"]), prompts=t32(g["prompts"]),
                             timbres=t32(g["timbres"]), codec_decoder=decs[mode], temp_durgen=0.3, temp_denoiser=0.3,
                             nsteps_durgen=4, nsteps_denoiser=4, exact_lengths=True)
    lens = (~out["tgt_mask"]).sum(dim=1).tolist()
    assert min(lens) < max(lens) == out["tgt_mask"].shape[1], lens
    assert out["wav_lens"].tolist() == [HOP * n for n in lens]
    refs = alone(out["latents"].float().cpu(), t32(g["timbres"]).float(), lens)
    check_batch(mode, out["wav"].cpu(), lens, refs, f"sample_batch {mode}")
