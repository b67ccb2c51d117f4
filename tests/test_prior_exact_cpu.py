"""Exact lengths in the prior stage, CPU side (tests/_priorexact.py states the definition and the bars).

The module's torch ops against the oracle run on every utterance alone; the calibration (today's padded call misses
the same bars by more than 100 x on the shorter utterances, and a padded phoneme costs one frame, so running padded
and trimming cannot pass); the defaults (flag off: the old code path, bitwise); prompt lengths from the pad id; the C
entry points' declaration, binding and host-side argument checks; the custom ops; the synthesize.py flag."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from _common import PKG, orc, rel_l2
from _flamed_common import build_flamed, build_codec_encoder
import _priorexact as px

B, L, P = 3, 13, 11
LENS, PLENS = [13, 7, 2], [11, 6, 3]
NFE, TEMP, SEED = 8, 0.3, 0
PAD = 1024


@pytest.fixture(scope="module")
def stack():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    m, dec = build_flamed("cpu")
    sd = {"prior_generator." + k: v.detach() for k, v in m.prior_generator.state_dict().items()}
    return m, dec, sd


@pytest.fixture(scope="module")
def case(stack):
    """Inputs and the alone references, computed once."""
    m, _, sd = stack
    g = torch.Generator().manual_seed(1)
    src = torch.tensor(LENS)
    mask = orc.mask_from_lengths(src, L)
    texts = torch.randint(1, 361, (B, L), generator=g).masked_fill(mask, 0)
    prompts = px.pad_prompts(torch.randint(0, PAD, (B, 6, P), generator=g), PLENS, PAD)
    torch.manual_seed(SEED)
    dn, sn = torch.randn(B, L), torch.randn(B, L)
    with torch.inference_mode():
        enc = orc.prior_encoder(sd, texts, mask)
    flow = px.flow_alone(sd, enc, LENS, dn, sn, NFE, TEMP)
    lr = px.lr_alone(enc, [f[0] for f in flow], [f[1] for f in flow], LENS)
    tgt = torch.tensor([t for _, t in lr])
    T = int(tgt.max())
    x = torch.zeros(B, T, enc.shape[-1])
    for u, (xu, tu) in enumerate(lr):
        x[u, :tu] = xu
    embs, logits = px.decode_alone(sd, x, tgt, prompts, PLENS)
    return dict(texts=texts, src=src, mask=mask, prompts=prompts, enc=enc, flow=flow, tgt=tgt, x=x, embs=embs, logits=logits)


def _check_flow(d, s, flow, lens):
    near = flips = 0
    for u, n in enumerate(lens):
        for got, ref in ((d[u], flow[u][0]), (s[u], flow[u][1])):
            e = rel_l2(got[:n], ref)
            print(f"utterance {u}: log-duration rel-L2 {e:.3e}")
            assert e <= px.DUR_BAR, (u, e)
            assert torch.all(got[n:] == 0)
            a, b = px.near_and_flips(got[:n], ref)
            near, flips = near + a, flips + b
    assert near <= 1 and flips == 0, (near, flips)


def test_definition_torch_ops(stack, case):
    """PriorGenerator.sample(exact_lengths=True, prompt_lens=...) on the module's torch ops is the definition."""
    m, _, sd = stack
    pg = m.prior_generator
    with torch.inference_mode():
        torch.manual_seed(SEED)
        d, s = pg.pva.flow(case["enc"], case["mask"], NFE, TEMP, exact=True)
        _check_flow(d, s, case["flow"], LENS)
        torch.manual_seed(SEED)
        pe, pl, tm = pg.sample(case["texts"], case["src"], L, case["prompts"], P, nfe=NFE, temperature=TEMP,
                               exact_lengths=True, prompt_lens=PLENS)
    assert torch.equal((~tm).sum(-1), case["tgt"])
    for u in range(B):
        ee, el = rel_l2(pe[u], case["embs"][u]), rel_l2(pl[u], case["logits"][u])
        print(f"utterance {u}: prior_embs rel-L2 {ee:.3e}, logits {el:.3e}")
        assert ee <= px.DEC_BAR["f32"] and el <= px.DEC_BAR["f32"], (u, ee, el)
        t = int(case["tgt"][u])
        assert torch.all(pe[u, :, t:] == 0) and torch.all(pl[u, :, :, t:] == 0)


def test_exact_under_autograd_equals_inference(stack, case):
    """The torch-op loop is the same with autograd on."""
    pg = stack[0].prior_generator
    torch.manual_seed(SEED)
    a = pg.sample(case["texts"], case["src"], L, case["prompts"], P, nfe=2, temperature=TEMP, exact_lengths=True,
                  prompt_lens=PLENS)
    with torch.inference_mode():
        torch.manual_seed(SEED)
        b = pg.sample(case["texts"], case["src"], L, case["prompts"], P, nfe=2, temperature=TEMP, exact_lengths=True,
                      prompt_lens=PLENS)
    assert a[0].requires_grad
    assert all(torch.equal(x.detach(), y) for x, y in zip(a, b))


def test_calibration_padded_call_misses_the_bars(stack, case):
    """Today's padded call on the same inputs: the shorter utterances miss the log-duration bar and the f32 decode bar
    by more than 100 x (the issue measured about 1e5 x and more than 3e3 x), the longest one meets them; and a padded
    phoneme repeats one frame, so tgt_len of a shorter utterance is its alone length + (L - len_u) even when no
    duration flips -- an implementation that runs padded and trims cannot pass."""
    m, _, sd = stack
    pg = m.prior_generator
    with torch.inference_mode():
        torch.manual_seed(SEED)
        d, s = pg.pva.flow(case["enc"], case["mask"], NFE, TEMP)
        for u, n in enumerate(LENS):
            ed, es = rel_l2(d[u, :n], case["flow"][u][0]), rel_l2(s[u, :n], case["flow"][u][1])
            print(f"padded flow, utterance {u}: dur {ed:.3e} sil {es:.3e}")
            if n == L:
                assert ed <= px.DUR_BAR and es <= px.DUR_BAR
            else:
                assert ed >= 100 * px.DUR_BAR and es >= 100 * px.DUR_BAR, (u, ed, es)
        # the exact durations (so no duration flips) through the default regulator
        dz = torch.zeros(B, L)
        sz = torch.zeros(B, L)
        for u, n in enumerate(LENS):
            dz[u, :n], sz[u, :n] = case["flow"][u]
        _, tl = pg.pva.length_regulator.LR(case["enc"], orc.log_to_frames(dz), orc.log_to_frames(sz), case["src"], None)
        assert tl.tolist() == [int(case["tgt"][u]) + (L - n) for u, n in enumerate(LENS)]
        _, tx = pg.pva.length_regulator.LR(case["enc"], orc.log_to_frames(dz), orc.log_to_frames(sz), case["src"], None,
                                           exact=True)
        assert torch.equal(tx, case["tgt"])
        # the padded decode of the alone frames: prompt slots of the shorter-prompt utterances are keys, positions shift
        pe, pl, _ = pg._decode(pg.bridge(case["x"]), case["tgt"], orc.mask_from_lengths(case["tgt"], case["x"].shape[1]),
                               case["prompts"], P)
    for u in range(B):
        ee, el = rel_l2(pe[u], case["embs"][u]), rel_l2(pl[u], case["logits"][u])
        print(f"padded decode, utterance {u}: prior_embs {ee:.3e} logits {el:.3e}")
        if PLENS[u] == P:
            assert ee <= px.DEC_BAR["f32"] and el <= px.DEC_BAR["f32"]
        else:
            assert ee >= 100 * px.DEC_BAR["f32"] and el >= 100 * px.DEC_BAR["f32"], (u, ee, el)


def _old_path(m, texts, src, prompts, timbres, nfe):
    """Flamed.sample_batch as it was before the flag: the calls it made, restated."""
    from flamed.utils.tools import get_mask_from_lengths
    pg = m.prior_generator
    src_masks = get_mask_from_lengths(src, texts.size(-1))
    out = pg.encoder(texts, src_masks)
    out, tgt_lens = pg.pva.sample(out, src, src_masks, nfe=nfe, temperature=0.3)
    tgt_masks = get_mask_from_lengths(tgt_lens, out.size(1))
    embs, logits, tgt_masks = pg._decode(pg.bridge(out), tgt_lens, tgt_masks, prompts, prompts.size(-1))
    lat = m.prob_generator.sample(cond=embs, spk=timbres, nfe=2, temperature=0.3, mask=~tgt_masks.unsqueeze(-1),
                                  solver="euler", exact_lengths=False)
    return embs, logits, tgt_masks, lat


def test_defaults_bitwise_and_flag_changes_the_short_utterance(stack, case):
    m = stack[0]
    timbres = torch.randn(B, 256, generator=torch.Generator().manual_seed(2))
    kw = dict(phonemes=case["texts"], src_lens=case["src"], prompts=case["prompts"], timbres=timbres, nsteps_durgen=4,
              nsteps_denoiser=2)
    with torch.inference_mode():
        torch.manual_seed(5)
        old = _old_path(m, case["texts"], case["src"], case["prompts"], timbres, 4)
    torch.manual_seed(5)
    off = m.sample_batch(**kw)
    for a, b in zip(old, (off["prior_embs"], off["prior_logits"], off["tgt_mask"], off["latents"])):
        assert torch.equal(a, b)
    torch.manual_seed(5)
    on = m.sample_batch(exact_prior=True, **kw)
    t_off, t_on = (~off["tgt_mask"]).sum(-1), (~on["tgt_mask"]).sum(-1)
    assert int(t_on[2]) < int(t_off[2]), (t_on, t_off)
    n = int(t_on[2])
    assert not torch.equal(on["prior_embs"][2, :, :n], off["prior_embs"][2, :, :n])
    assert torch.all(on["prior_embs"][2, :, n:] == 0)
    # the flag took the prompt lengths from the pad id
    torch.manual_seed(5)
    on2 = m.sample_batch(exact_prior=True, prompt_lens=PLENS, **kw)
    assert torch.equal(on["prior_embs"], on2["prior_embs"]) and torch.equal(on["tgt_mask"], on2["tgt_mask"])


def test_prompt_lens_from_pad_id(stack, case):
    m = stack[0]
    assert m._prompt_lens_from_pad(case["prompts"]) == PLENS
    assert m._prompt_lens_from_pad(case["prompts"][:1]) == [P]
    hole = case["prompts"].clone()
    hole[1, :, 2] = PAD  # a pad id inside the prompt: not a prefix
    with pytest.raises(ValueError, match="prefix"):
        m._prompt_lens_from_pad(hole)
    ragged = case["prompts"].clone()
    ragged[2, 3, 2] = PAD  # quantizer 3 of utterance 2 one code shorter
    with pytest.raises(ValueError, match="quantizers"):
        m._prompt_lens_from_pad(ragged)
    with pytest.raises(ValueError, match="prefix|quantizers"):
        m.sample_batch(phonemes=case["texts"], src_lens=case["src"], prompts=hole, timbres=torch.zeros(B, 256),
                       nsteps_durgen=2, nsteps_denoiser=2, exact_prior=True)
    with pytest.raises(ValueError, match="prompt_lens"):
        m.prior_generator.sample(case["texts"], case["src"], L, case["prompts"], P, nfe=2, prompt_lens=[11, 6, 12])


def test_header_binding_export_and_validation():
    from flamed import _native as nat
    root = os.path.dirname(PKG)
    hdr = open(os.path.join(root, "include", "flamed_hip.h")).read()
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    names = ("flamed_pva_flow_exact", "flamed_lr_lengths_exact", "flamed_prior_decode_lens")
    for name in names:
        assert f"FLAMED_API int {name}(" in hdr and name in nat.SIGNATURES and name in integ, name
    Lb = nat.lib()
    flow, lrx, dec = (getattr(Lb, n) for n in names)  # exported
    assert len(flow.argtypes) == len(Lb.flamed_pva_flow.argtypes) and lrx.argtypes == Lb.flamed_lr_lengths.argtypes
    assert len(dec.argtypes) == len(Lb.flamed_prior_decode.argtypes) + 1
    one = ctypes.c_void_p(256)  # non-null stand-ins: every check below comes before any pointer is touched

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def err(fn, *args):
        rc = fn(*args)
        return rc, (Lb.flamed_last_error() or b"").decode()

    good = ints(16, 9)
    for k in range(8):  # dur, sil, enc, lens, dur_t, sil_t, ts, ws
        p = [one, one, one, good, one, one, one, one]
        p[k] = None
        rc, msg = err(flow, p[0], p[1], p[2], p[3], p[4], p[5], p[6], 4, 2, 16, p[7], 1 << 20, 1, None)
        assert rc == 1001 and "null" in msg, (k, rc, msg)
    for bad in ((16, 0), (17, 9), (-1, 9)):  # 1 <= len <= L
        rc, msg = err(flow, one, one, one, ints(*bad), one, one, one, 4, 2, 16, one, 1 << 20, 1, None)
        assert rc == 1001 and "length" in msg, (bad, rc, msg)
    for dims in ((0, 2, 16), (4, 0, 16), (4, 2, 0)):
        rc, msg = err(flow, one, one, one, good, one, one, one, *dims, one, 1 << 20, 1, None)
        assert rc == 1001 and "dims" in msg, (dims, rc, msg)
    for k in range(5):  # phone, sil, src_lens, cum, tgt_len
        p = [one] * 5
        p[k] = None
        rc, msg = err(lrx, p[0], p[1], p[2], 2, 16, 1, p[3], p[4], None)
        assert rc == 1001 and "flamed_lr_lengths_exact" in msg, (k, rc, msg)
    # the decode checks its handle first (a null handle is "not loaded"), as flamed_prior_decode does
    rc, msg = err(dec, None, one, one, one, 2, 16, 8, ints(8, 3), None, one, one, one, 1 << 20, 1, None)
    assert rc == 1001 and "not loaded" in msg, (rc, msg)


def test_ops_registered_with_fake_shapes():
    import types
    from torch._subclasses.fake_tensor import FakeTensorMode
    from flamed import ops
    for name in ("pva_flow_exact", "length_regulate_exact", "prior_decode_lens"):
        assert name in ops.OPS
        schema = str(getattr(torch.ops.flamed_hip, name).default._schema)
        assert schema.startswith(f"flamed_hip::{name}("), schema
    assert "[] lens" in str(torch.ops.flamed_hip.pva_flow_exact.default._schema)
    assert "[] prompt_lens" in str(torch.ops.flamed_hip.prior_decode_lens.default._schema)
    # the existing schemas are what they were
    assert str(torch.ops.flamed_hip.pva_flow.default._schema) == \
        "flamed_hip::pva_flow(SymInt oid, Tensor x, Tensor src_mask, Tensor dur_t, Tensor sil_t, Tensor ts, SymInt nfe) -> (Tensor, Tensor)"
    assert str(torch.ops.flamed_hip.prior_decode.default._schema) == \
        "flamed_hip::prior_decode(SymInt oid, Tensor x, Tensor tgt_mask, Tensor prompts, SymInt prompts_len) -> (Tensor, Tensor)"

    class Owner:
        pass

    o = Owner()
    o.pg = types.SimpleNamespace(prior_decoder=[0] * 6, shared_decoder=types.SimpleNamespace(d_model=384),
                                 head=types.SimpleNamespace(weight=torch.empty(1025, 384)))
    oid = ops.register(o)
    with FakeTensorMode():
        x = torch.empty(3, 13, 192)
        d, s = ops.pva_flow_exact(oid, x, torch.empty(3, 13), torch.empty(3, 13), torch.empty(9), 8, [13, 7, 2])
        assert d.shape == (3, 13) and s.shape == (3, 13) and d.dtype == torch.float32
        out, tl = ops.length_regulate_exact(x, torch.empty(3, 13), torch.empty(3, 13),
                                            torch.empty(3, dtype=torch.int64), 40, True)
        assert out.shape == (3, 40, 192) and tl.shape == (3,) and tl.dtype == torch.int64
        e, lg = ops.prior_decode_lens(oid, torch.empty(3, 24, 192), torch.empty(3, 24, dtype=torch.bool),
                                      torch.empty(3, 6, 11, dtype=torch.int64), 11, [11, 6, 3])
        assert e.shape == (3, 6, 24, 384) and lg.shape == (3, 1025, 6, 24)


def test_cli_flag_suffix_and_batch_independent_files(stack, tmp_path):
    """--exact-prior parses, names its outputs, and with --exact-lengths the two files of a batch of two lines with
    different prompts hold the sample counts each line gets in a batch of one.  Duration temperature 0: the noise
    draw of a batch of two is not the draw of a batch of one, the definition slices one draw."""
    sys.path.insert(0, PKG)
    import synthesize as syn
    from flamed.utils.audio import load_wav, write_wav
    a = syn.build_arg_parser().parse_args(["--ckpt-path", "c", "--cfg-path", "g", "--exact-prior", "true"])
    assert a.exact_prior is True
    assert syn.build_arg_parser().parse_args(["--ckpt-path", "c", "--cfg-path", "g"]).exact_prior is False
    assert syn._solver_suffix("euler") == "" and syn._solver_suffix("heun", True) == "-heun-exact"
    assert syn._solver_suffix("euler", False, True) == "-xprior" and syn._solver_suffix("heun", True, True) == "-heun-exact-xprior"
    m, dec, _ = stack
    enc = build_codec_encoder("cpu")
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "pr")
    for i in range(2):
        write_wav(str(tmp_path / "pr" / f"p{i}.wav"), rng.normal(0, 0.1, 4000 + 2400 * i).astype(np.float32))
    lines = ["u0.wav|p0.wav|hello world.", "u1.wav|p1.wav|good morning to you all."]

    def run(name, text, batch):
        meta = tmp_path / f"{name}.txt"
        meta.write_text(text)
        syn.synthesize_with_metadata(m, enc, dec, str(meta), str(tmp_path / "pr"), str(tmp_path / name), 4, 2, 0.0, 0.3,
                                     skip_existing=False, batch_size=batch, exact_lengths=True, exact_prior=True)
        d = tmp_path / name / "nfe2-temp0.3-exact-xprior"
        return {f: len(load_wav(str(d / f), 16000)) for f in sorted(os.listdir(d))}

    both = run("both", "\n".join(lines) + "\n", 2)
    assert sorted(both) == ["u0.wav", "u1.wav"]
    for i, line in enumerate(lines):
        assert run(f"one{i}", line + "\n", 1) == {f"u{i}.wav": both[f"u{i}.wav"]}
    assert both["u0.wav"] != both["u1.wav"]
