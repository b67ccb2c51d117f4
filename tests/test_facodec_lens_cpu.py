"""FaCodec decode with exact lengths, CPU side (tests/_faclens.py has the definition and the bars).

1. calibration: what a decode of the padded batch does to the shorter utterances (the evidence that the parity
   tests of this file and of test_facodec_lens_gpu.py discriminate: decode-and-trim misses the bf16 bar 41-91 x on these inputs);
2. FACodecDecoder.inference(x, spk, lens) on the torch ops against the oracle alone; 3. the ValueErrors;
4. flamed_fac_decode_lens: declared, bound, exported, its host-side argument checks; 5. the custom op;
6. Flamed.sample_batch(exact_lengths=True) hands the lengths to the decoder; 7. synthesize.py trims the files."""
import argparse
import ctypes
import os
import sys
import types

import pytest
import torch

from _common import PKG, golden, orc, t32
from _codecprofile import FACTOR_DEC, W_DEC, window_errors
from _faclens import HOP, alone, calm_sd, case, check_batch, inputs, make_decoder

CAL_SHAPES = [(3, 13, (13, 7, 2)), (2, 32, (32, 19)), (4, 9, (9, 1, 5, 8))]


@pytest.fixture(scope="module")
def dec():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return make_decoder("f32", "cpu")


def _rms(x):
    return float(torch.as_tensor(x, dtype=torch.float64).pow(2).mean().sqrt())


@pytest.mark.parametrize("B,T,lens", CAL_SHAPES)
def test_calibration_padded_decode_misses_the_bars(B, T, lens):
    """The oracle's dense decode of latents zeroed past the lengths (what exact_lengths delivers), cut at each
    utterance's end, against the utterance decoded alone: its worst window is >= 10 x the bf16 bar (1.4 x the
    emulation's worst window) for every utterance shorter than T, and what it puts behind the end is not silence."""
    lat, spk, refs = case(B, T, lens)
    z = lat.clone()
    for u, n in enumerate(lens):
        z[u, :, n:] = 0
    padded = orc.facodec_decode(calm_sd(), z, spk)
    for u, n in enumerate(lens):
        if n == T:
            continue
        ref, floor = refs[u]
        got = padded[u:u + 1, :, :HOP * n]
        worst = float(window_errors(got, ref, W_DEC).max())
        fl = float(window_errors(floor, ref, W_DEC).max())
        pad_rms, utt_rms = _rms(padded[u, :, HOP * n:]), _rms(got)
        print(f"calibration {B}x{T} len {n}: padded-decode worst window {worst:.2e} = {worst / fl:.0f} x the floor "
              f"({worst / (FACTOR_DEC * fl):.0f} x the bar); padding RMS {pad_rms:.2e}, utterance RMS {utt_rms:.2e}")
        assert worst >= 10 * FACTOR_DEC * fl
        assert pad_rms >= 0.5 * utt_rms


@pytest.mark.parametrize("B,T,lens", CAL_SHAPES)
def test_inference_lens_torch_ops_vs_oracle_alone(dec, B, T, lens):
    lat, spk, refs = case(B, T, lens)
    poisoned = lat.clone()
    for u, n in enumerate(lens):
        poisoned[u, :, n:] = float("nan")
    with torch.inference_mode():
        wav = dec.inference(lat, spk, lens)
        wav_nan = dec.inference(poisoned, spk, torch.tensor(lens))
    assert wav.shape == (B, 1, HOP * T)
    check_batch("f32", wav, lens, refs, f"torch ops {B}x{T}")
    assert torch.equal(wav, wav_nan)  # nothing stored in the padding reaches the output


def test_inference_dense_lens_is_the_plain_call(dec):
    lat, spk = inputs(3, 13)
    with torch.inference_mode():
        assert torch.equal(dec.inference(lat, spk, [13] * 3), dec.inference(lat, spk))
        assert torch.equal(dec.inference(lat, spk, lens=None), dec.inference(lat, spk))


def test_inference_lens_validation(dec):
    lat, spk = inputs(3, 13)
    for bad in ([13, 7], [13, 7, 2, 2], [13, 0, 2], [13, 14, 2], [13, -1, 2], torch.tensor([13.0, 7.0, 2.0]), [13, 7.5, 2],
                torch.tensor([[13, 7, 2]]), 7):
        with pytest.raises(ValueError):
            dec.inference(lat, spk, bad)
    from flamed.models.facodec.facodec import FacDecoderHIP
    owner = FacDecoderHIP(dec, "f32")
    with pytest.raises(ValueError):  # before the library or a device is touched
        owner.decode(lat, spk, lens=[13, 7, 0])


def test_header_binding_export_and_validation():
    from flamed import _native as nat
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "flamed_hip.h")).read()
    integ = open(os.path.join(os.path.dirname(PKG), "INTEGRATION.md")).read()
    name = "flamed_fac_decode_lens"
    assert f"FLAMED_API int {name}(" in hdr and name in nat.SIGNATURES and name in integ
    L = nat.lib()
    fn = L.flamed_fac_decode_lens  # exported
    assert len(fn.argtypes) == 11 and len(L.flamed_fac_decode.argtypes) == 10
    one = ctypes.c_void_p(256)  # non-null stand-ins: every check below comes before any pointer is touched
    B, T = 2, 16

    def lens_of(*v):
        return (ctypes.c_int * len(v))(*v)

    def err(*args):
        rc = fn(*args)
        return rc, (L.flamed_last_error() or b"").decode()

    good = lens_of(16, 9)
    for k in range(6):  # handle, latents, speaker, lengths, wav, workspace
        p = [one, one, one, good, one, one]
        p[k] = None
        rc, msg = err(p[0], p[1], p[2], B, T, p[3], p[4], p[5], 1 << 20, 1, None)
        assert rc == 1001 and "null" in msg, (k, rc, msg)
    for bad in ((16, 0), (17, 9), (-3, 9), (16, 1 << 30)):  # 1 <= len <= T
        rc, msg = err(one, one, one, B, T, lens_of(*bad), one, one, 1 << 20, 1, None)
        assert rc == 1001 and "length" in msg, (bad, rc, msg)
    for dims in ((0, 16), (2, 0), (-1, 16)):
        rc, msg = err(one, one, one, dims[0], dims[1], good, one, one, 1 << 20, 1, None)
        assert rc == 1001, (dims, rc, msg)


def test_op_registered_with_fake_shape():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops
    assert "fac_decode_lens" in ops.OPS
    op = torch.ops.flamed_hip.fac_decode_lens
    assert [a.name for a in op.default._schema.arguments] == ["oid", "x", "spk", "lens"]
    assert "Int[] lens" in str(op.default._schema)
    assert [a.name for a in torch.ops.flamed_hip.fac_decode.default._schema.arguments] == ["oid", "x", "spk"]  # as it was

    class Owner:
        dec = types.SimpleNamespace(hop_length=HOP)

    own = Owner()
    oid = ops.register(own)
    with FakeTensorMode():
        w = op(oid, torch.empty(3, 256, 13), torch.empty(3, 256), [13, 7, 2])
        assert w.shape == (3, 1, HOP * 13) and w.dtype == torch.float32


def test_sample_batch_hands_the_lengths_to_the_decoder():
    """The end-to-end fixture's ragged batch of two on CPU: with the flag wav_lens = 200 len, every waveform is the
    decoder run alone on that utterance's own latents (f32 bars against the oracle) and exactly 0 behind its end;
    without it no wav_lens, and wav is codec_decoder.inference(latents, timbres) bitwise."""
    from _flamed_common import build_flamed
    torch.set_num_threads(8)
    m, _ = build_flamed("cpu")
    cdec = make_decoder("f32", "cpu")
    g = golden("flamed_sample")
    kw = dict(phonemes=t32(g["phonemes"]), src_lens=t32(g["src_lens"]), prompts=t32(g["prompts"]), timbres=t32(g["timbres"]),
              codec_decoder=cdec, temp_durgen=0.3, temp_denoiser=0.3, nsteps_durgen=4, nsteps_denoiser=4)
    with torch.inference_mode():
        torch.manual_seed(int(g["rng_seed"]))
        exact = m.sample_batch(**kw, exact_lengths=True)
        torch.manual_seed(int(g["rng_seed"]))
        padded = m.sample_batch(**kw)
        again = cdec.inference(padded["latents"], kw["timbres"])
    lens = (~exact["tgt_mask"]).sum(dim=1).tolist()
    T = exact["tgt_mask"].shape[1]
    assert min(lens) < max(lens) == T, lens
    assert exact["wav_lens"].tolist() == [HOP * n for n in lens]
    assert exact["wav"].shape == (len(lens), 1, HOP * T)
    check_batch("f32", exact["wav"], lens, alone(exact["latents"], kw["timbres"], lens), "sample_batch CPU")
    assert "wav_lens" not in padded
    assert torch.equal(padded["wav"], again)
    u = lens.index(min(lens))  # the flag moved the short utterance's waveform
    assert not torch.equal(exact["wav"][u], padded["wav"][u])


def test_synthesize_metadata_mode_trims_each_file(tmp_path, monkeypatch):
    """Two lines of different length in one batch: with --exact-lengths true the two files hold their own wav_lens
    samples; without it both hold the batch's padded length, as before."""
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed import Flamed
    from flamed.utils.audio import load_wav
    from flamed.utils.random_ckpt import write
    from test_rk2_cpu import _prompts
    paths = write(str(tmp_path / "ck"))
    _prompts(tmp_path / "pr")
    meta = tmp_path / "meta.txt"
    meta.write_text("a.wav|p0.wav|hello world.\nb.wav|p0.wav|a much longer line of text to say.\n")
    ns = dict(ckpt_path=paths["ckpt"], cfg_path=paths["cfg"], text=None, prompt_list=None, prompt_dir=str(tmp_path / "pr"),
              metadata_file=str(meta), output_dir=str(tmp_path / "out"), weights_only=True, nsteps_durgen=4,
              nsteps_denoiser=4, temp_durgen=0.3, temp_denoiser=0.3, device="cpu", skip_existing=True, batch_size=4,
              codec_ckpt_dir=str(tmp_path / "ck"))
    seen = []
    real = Flamed.sample_batch

    def spy(self, *a, **kw):
        out = real(self, *a, **kw)
        seen.append((out["wav_lens"].tolist() if "wav_lens" in out else None, out["wav"].shape[-1]))
        return out

    monkeypatch.setattr(Flamed, "sample_batch", spy)
    assert syn.main(argparse.Namespace(**ns, exact_lengths=True)) > 0
    assert syn.main(argparse.Namespace(**ns)) > 0
    (wl, _), (none, padded_n) = seen
    assert none is None and len(wl) == 2 and wl[0] != wl[1] and max(wl) <= padded_n
    count = lambda d, f: len(load_wav(str(tmp_path / "out" / d / f), 16000))
    assert [count("nfe4-temp0.3-exact", f) for f in ("a.wav", "b.wav")] == wl
    assert [count("nfe4-temp0.3", f) for f in ("a.wav", "b.wav")] == [padded_n, padded_n]
