"""Exact lengths in the prompt stage without a GPU: the definition on torch ops (a loop over the utterances, each alone)
against the oracle alone, the calibration of the GPU bars against the bug they have to see (the dense padded batch), the
host length arithmetic, the position-row fact, the op layer, the C ABI's validation and the CLI flag.  Shapes, bars and
references: tests/_promptlens.py.

Calibration figures (dense padded-batch-and-trim on (3, 2600, (2600, 1999, 403)), oracle): the last frame of the two
shorter utterances is 4.9e-1 and 6.0e-1 from alone against the 1e-5 frame bar; their speaker embeddings 2.9e-1 and
7.6e-1 rel-L2."""
import ctypes
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from _common import PKG, orc
import _promptprofile as pp
import _promptlens as pl


@pytest.fixture(scope="module")
def enc():
    return pl.make_encoder("f32", "cpu")


@pytest.fixture(scope="module")
def dec():
    return pl.make_decoder("cpu")


def _module_run(enc, dec, wav, lens):
    frames = [pl.out_len(m) for m in lens]
    with torch.inference_mode():
        z = enc(wav, lens=lens)
        outs, codes, _, qb, spk = dec(z, eval_vq=False, vq=True, lens=frames)
    return z, frames, {"outs": outs, "codes": codes, "qbuf": torch.stack(list(qb)), "spk": spk, "rows": None}


@pytest.mark.parametrize("B,n,lens", pl.E2E_SHAPES[:3], ids=lambda v: str(v))
def test_torch_definition_against_the_oracle_alone(enc, dec, B, n, lens):
    wav, per = pl.e2e_case(B, n, lens)
    z, frames, o = _module_run(enc, dec, pl.filled(wav, lens, "zero"), lens)
    assert z.shape == (B, 256, pl.out_len(n)) and o["codes"].shape == (6, B, pl.out_len(n))
    refs = [p["vq"] for p in per]
    label = f"torch ops {B}x{n}"
    pl.check_encoder("f32", z, lens, per, label)
    pl.check_codes(o["codes"], frames, refs, label)
    pl.check_quantized(o, frames, refs, label)
    pl.check_timbre(o, frames, refs, label)
    # nothing stored behind an end is read
    zn, _, on = _module_run(enc, dec, pl.filled(wav, lens, "nan"), lens)
    assert torch.equal(z, zn)
    for k in ("outs", "codes", "qbuf", "spk"):
        assert torch.equal(o[k], on[k]), k


def test_oracle_gap_facts():
    """What the code checks rely on: no oracle near-tie (top-2 gap < 1e-5) on the valid frames of any end-to-end shape
    nor of the last three VQ shapes, and exactly one on (3, 130, (130, 64, 1)) -- so a changed fixture is noticed."""
    for B, n, lens in pl.E2E_SHAPES:
        _, per = pl.e2e_case(B, n, lens)
        g = min(float(p["vq"]["r32"]["gaps"].min()) for p in per)
        print(f"e2e ({B}, {n}, {lens}): smallest oracle top-2 gap {g:.2e}")
        assert g >= pp.NEAR_TIE, (B, n, lens, g)  # measured 4.2e-4 / 2.7e-4 / 1.0e-2 / 2.2e-5
    near = []
    for B, T, lens in pl.VQ_SHAPES:
        _, refs = pl.vq_case(B, T, lens)
        g = min(float(r["r32"]["gaps"].min()) for r in refs)
        near.append(sum(int((r["r32"]["gaps"] < pp.NEAR_TIE).sum()) for r in refs))
        print(f"vq ({B}, {T}, {lens}): smallest oracle top-2 gap {g:.2e}, near-ties {near[-1]}")
    assert near == [1, 0, 0, 0], near  # measured gaps 4.3e-6 / 2.5e-5 / 1.5e-3 / 2.4e-3


def test_calibration_dense_padded_batch_misses_the_bars():
    """The bars see the bug the feature removes: the dense encode of the zero-padded batch, trimmed, against alone."""
    B, n, lens = pl.E2E_SHAPES[0]
    wav, per = pl.e2e_case(B, n, lens)
    with torch.inference_mode():
        zd = orc.facodec_encode(pl.enc_sd(), pl.filled(wav, lens, "zero"))
        rows = orc.timbre_encoder(pp.decoder_sd(), zd.transpose(1, 2))
        spk = rows.transpose(1, 2).mean(dim=2)
    for u in (1, 2):
        ref, r = per[u]["z"], per[u]["vq"]
        Tu = ref.shape[2]
        e = pl.frame_errors(zd[u:u + 1, :, :Tu], ref)
        se = float(pp.spk_err(spk[u:u + 1], r["r64"]["spk"], r["r64"]["rows"]).max())
        bar = pp.bar_of(pp.floors(r)["spk"])
        print(f"dense padded batch, utterance {u}: last frame {float(e[-1]):.2e} (bar {pl.F32_FRAME_BAR:.0e}), spk {se:.2e} "
              f"(bar {bar:.2e})")
        assert float(e[-1]) >= 50 * pl.F32_FRAME_BAR
        assert se >= 1000 * bar
    e0 = pl.frame_errors(zd[0:1], per[0]["z"])
    assert float(e0.max()) <= pl.F32_FRAME_BAR  # the full-length utterance is what it is alone


def test_out_len_is_the_conv_stacks_length(enc):
    convs = [m for m in enc.modules() if isinstance(m, torch.nn.Conv1d) and m.stride[0] > 1]
    assert [c.stride[0] for c in convs] == list(enc.up_ratios)

    def torch_len(n):
        x = torch.zeros(1, 1, n)
        for c in convs:
            x = F.conv1d(x, torch.ones(1, 1, c.kernel_size[0]), stride=c.stride, padding=c.padding)
        return x.shape[2]
    for n in range(152, 1301):
        assert enc.out_len(n) == torch_len(n) == pl.out_len(n), n
    for n in range(1, 152):
        assert enc.out_len(n) == 0, n
        with pytest.raises(RuntimeError):
            torch_len(n)
    assert enc.min_len() == pl.MIN_N == 152
    assert [enc.out_len(m) for m in (2048, 1985, 1984)] == [10, 10, 10]  # two lengths, one count


def test_position_row_is_the_batch_index_without_lens(dec):
    """The reference's `x + pe[:B]`: utterance 1 of two equal-length prompts does not get its solo speaker embedding
    through the dense module; through lens = [9, 9] it does (and the codes are equal either way)."""
    x = pp.case_input(2, 9)
    with torch.inference_mode():
        _, cd, _, _, sd_ = dec(x, eval_vq=False, vq=True)
        _, cl, _, _, sl = dec(x, eval_vq=False, vq=True, lens=[9, 9])
        _, c1, _, _, s1 = dec(x[1:2], eval_vq=False, vq=True)
        _, c1l, _, _, s1l = dec(x[1:2], eval_vq=False, vq=True, lens=[9])
    rel = float((sd_[1] - s1[0]).norm() / s1[0].norm())
    print(f"dense spk[1] against alone: rel-L2 {rel:.2e}")
    assert rel > 1e-2  # measured 2.0e-1
    assert torch.equal(sl[1], s1[0])
    assert float((sl[0] - sd_[0]).norm() / sd_[0].norm()) < 1e-5  # utterance 0 had pe[0] in the dense call already
    assert torch.equal(cd, cl) and torch.equal(cl[:, 1:2], c1)
    assert torch.equal(s1l, s1) and torch.equal(c1l, c1)  # B = 1, full length: the call without lens


def test_pad_code_default_and_explicit(dec):
    x = pp.case_input(2, 9)
    with torch.inference_mode():
        _, c, _, _, _ = dec(x, eval_vq=False, vq=True, lens=[9, 4])
        _, c7, _, _, _ = dec(x, eval_vq=False, vq=True, lens=[9, 4], pad_code=7)
    assert bool((c[:, 1, 4:] == pl.PAD).all()) and bool((c7[:, 1, 4:] == 7).all())
    assert torch.equal(c[:, :, :4], c7[:, :, :4])


def test_ops_registered_with_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops
    assert "enc_encode_lens" in ops.OPS and "vq_encode_lens" in ops.OPS
    e, v = torch.ops.flamed_hip.enc_encode_lens, torch.ops.flamed_hip.vq_encode_lens
    assert [a.name for a in e.default._schema.arguments] == ["oid", "x", "lens"]
    assert [a.name for a in v.default._schema.arguments] == ["oid", "x", "lens", "pad_code"]
    assert "Int[] lens" in str(e.default._schema) and "Int pad_code" in str(v.default._schema)
    assert [a.name for a in torch.ops.flamed_hip.enc_encode.default._schema.arguments] == ["oid", "x"]  # as they were
    assert [a.name for a in torch.ops.flamed_hip.vq_encode.default._schema.arguments] == ["oid", "x"]

    class EncOwner:
        enc = types.SimpleNamespace(out_channels=256)

        def out_len(self, n):
            return pl.out_len(n)

    class VqOwner:
        dec = types.SimpleNamespace(quantizer=[types.SimpleNamespace(layers=[0] * k) for k in (1, 2, 3)])

    eo, vo = EncOwner(), VqOwner()
    with FakeTensorMode():
        z = e(ops.register(eo), torch.empty(3, 1, 2600), [2600, 1999, 403])
        assert z.shape == (3, 256, 13) and z.dtype == torch.float32
        outs, codes, qb, spk = v(ops.register(vo), torch.empty(3, 256, 13), [13, 10, 2], 1024)
        assert outs.shape == (3, 256, 13) and codes.shape == (6, 3, 13) and codes.dtype == torch.int64
        assert qb.shape == (3, 3, 256, 13) and spk.shape == (3, 256)


def test_module_validation(enc, dec):
    wav = pl.wav_input(3, 2600)
    for bad in ([2600, 1999], [2600, 1999, 403, 403], [2600, 0, 403], [2600, 2601, 403], [2600, -1, 403],
                torch.tensor([2600.0, 1999.0, 403.0]), [2600, 7.5, 403], torch.tensor([[2600, 1999, 403]]), 7):
        with pytest.raises(ValueError):
            enc(wav, lens=bad)
    with pytest.raises(ValueError, match="too short"):
        enc(wav, lens=[2600, 151, 403])
    with torch.inference_mode():
        assert enc(wav, lens=[2600, 152, 403]).shape == (3, 256, 13)
        assert torch.equal(enc(wav, lens=[2600] * 3), enc(wav))  # every length n: the call without lens
        assert torch.equal(enc.inference(wav, torch.tensor([2600, 1999, 403])), enc(wav, lens=[2600, 1999, 403]))
    x = pp.case_input(3, 13)
    for bad in ([13, 7], [13, 0, 2], [13, 14, 2], [13, 7.5, 2], torch.tensor([13.0, 7.0, 2.0]), 7):
        with pytest.raises(ValueError):
            dec(x, eval_vq=False, vq=True, lens=bad)
    from flamed.models.facodec.facodec import EncoderHIP, VqHIP
    with pytest.raises(ValueError):  # before the library or a device is touched
        EncoderHIP(enc, "f32").encode(wav, lens=[2600, 0, 403])
    with pytest.raises(ValueError):
        VqHIP(dec).encode(x, lens=[13, 7, 14], pad_code=1024)


def test_header_binding_export_and_validation():
    from flamed import _native as nat
    root = os.path.dirname(PKG)
    hdr = open(os.path.join(root, "include", "flamed_hip.h")).read()
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in ("flamed_enc_encode_lens", "flamed_vq_encode_lens"):
        assert f"FLAMED_API int {name}(" in hdr and name in nat.SIGNATURES and name in integ
    assert "pe[0]" in hdr
    L = nat.lib()
    one = ctypes.c_void_p(256)  # non-null stand-ins: every check below comes before any pointer is touched

    def lens_of(*v):
        return (ctypes.c_int * len(v))(*v)

    def msg():
        return (L.flamed_last_error() or b"").decode()

    # ---- encoder: a real (host-only, unloaded) handle, since the length range comes from its stride chain
    fn = L.flamed_enc_encode_lens
    assert len(fn.argtypes) == 10 and len(L.flamed_enc_encode.argtypes) == 9
    h = ctypes.c_void_p()
    nat.check(L.flamed_enc_create(32, 4, lens_of(2, 4, 5, 5), 256, nat.FLAMED_F32, ctypes.byref(h)), "flamed_enc_create")
    try:
        B, n = 2, 2600
        good = lens_of(2600, 403)
        for k in range(5):  # handle, wav, lengths, out, workspace
            p = [h, one, good, one, one]
            p[k] = None
            rc = fn(p[0], p[1], B, n, p[2], p[3], p[4], 1 << 20, 1, None)
            assert rc == 1001 and "null" in msg(), (k, rc, msg())
        for bad in ((2600, 151), (2601, 403), (-3, 403), (2600, 0), (2600, 1 << 30)):  # 152 <= len <= n
            rc = fn(h, one, B, n, lens_of(*bad), one, one, 1 << 20, 1, None)
            assert rc == 1001 and "length" in msg() and "152" in msg(), (bad, rc, msg())
        for dims in ((0, 2600), (2, 0), (-1, 2600)):
            assert fn(h, one, dims[0], dims[1], good, one, one, 1 << 20, 1, None) == 1001, dims
        assert fn(h, one, B, n, lens_of(2600, 152), one, one, 1 << 20, 1, None) == 1001 and "not loaded" in msg()
    finally:
        L.flamed_enc_destroy(h)
    # ---- quantizers + timbre encoder
    fn = L.flamed_vq_encode_lens
    assert len(fn.argtypes) == 14 and len(L.flamed_vq_encode.argtypes) == 12
    B, T = 2, 16
    good = lens_of(16, 9)
    for k in range(8):  # handle, x, lengths, outs, codes, qbuf, spk, workspace
        p = [one, one, good, one, one, one, one, one]
        p[k] = None
        rc = fn(p[0], p[1], B, T, p[2], 1024, p[3], p[4], p[5], p[6], p[7], 1 << 20, 1, None)
        assert rc == 1001 and "null" in msg(), (k, rc, msg())
    for bad in ((16, 0), (17, 9), (-3, 9), (16, 1 << 30)):  # 1 <= len <= T
        rc = fn(one, one, B, T, lens_of(*bad), 1024, one, one, one, one, one, 1 << 20, 1, None)
        assert rc == 1001 and "length" in msg(), (bad, rc, msg())
    for dims in ((0, 16), (2, 0), (-1, 16)):
        assert fn(one, one, dims[0], dims[1], good, 1024, one, one, one, one, one, 1 << 20, 1, None) == 1001, dims


def test_encode_prompts_on_cpu(enc, dec):
    """Flamed.encode_prompts on torch ops: three waveforms of different length against each alone, in the form
    sample_batch takes."""
    from _flamed_common import build_flamed
    m, _ = build_flamed("cpu")
    B, n, lens = pl.E2E_SHAPES[0]
    wav, per = pl.e2e_case(B, n, lens)
    prompts = [wav[0, 0, :lens[0]].numpy(), wav[1, 0, :lens[1]], wav[2, 0, :lens[2]].numpy()]
    codes, plens, timbres = m.encode_prompts(prompts, sr=16000, codec_encoder=enc, codec_decoder=dec)
    assert plens == [13, 10, 2] and codes.shape == (3, 6, 13) and timbres.shape == (3, 256)
    pad = m.prior_generator.code_embedding.padding_idx
    assert pad == pl.PAD
    pl.check_codes(codes.permute(1, 0, 2), plens, [p["vq"] for p in per], "encode_prompts CPU", pad)
    pl.check_timbre({"spk": timbres, "rows": None}, plens, [p["vq"] for p in per], "encode_prompts CPU")
    assert m._prompt_lens_from_pad(codes) == plens
    with pytest.raises(ValueError):
        m.encode_prompts([], codec_encoder=enc, codec_decoder=dec)
    with pytest.raises(ValueError):
        m.encode_prompts(prompts)


def test_cli_flag_parses_and_defaults_to_false():
    sys.path.insert(0, PKG)
    import synthesize as syn
    p = syn.build_arg_parser()
    base = ["--ckpt-path", "c", "--cfg-path", "g"]
    assert p.parse_args(base).batch_prompts is False
    assert p.parse_args(base + ["--batch-prompts", "true"]).batch_prompts is True
    assert p.parse_args(base + ["--batch-prompts", "false"]).batch_prompts is False
    assert syn._solver_suffix("euler") == ""  # the flag adds nothing to a name


def test_batched_cache_fill_encodes_each_path_once(monkeypatch):
    sys.path.insert(0, PKG)
    import synthesize as syn
    calls = []

    class M:
        def encode_prompts(self, paths, sr, codec_encoder, codec_decoder):
            calls.append(list(paths))
            B = len(paths)
            return torch.arange(B * 6 * 5).reshape(B, 6, 5), [3 + u for u in range(B)], torch.ones(B, 256)

    cache = {"c.wav": (torch.zeros(6, 2, dtype=torch.long), torch.zeros(256))}
    syn.encode_prompt_batch(M(), None, None, ["a.wav", "c.wav", "b.wav", "a.wav"], cache)
    assert calls == [["a.wav", "b.wav"]]  # the cached path and the duplicate are not encoded again
    assert cache["a.wav"][0].shape == (6, 3) and cache["b.wav"][0].shape == (6, 4) and cache["c.wav"][0].shape == (6, 2)
    syn.encode_prompt_batch(M(), None, None, ["a.wav", "b.wav"], cache)
    assert len(calls) == 1
