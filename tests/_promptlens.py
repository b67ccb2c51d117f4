"""Shared pieces of the exact-lengths prompt stage tests (test_prompt_lens_cpu.py, test_prompt_lens_gpu.py).

The definition under test: utterance u of a padded batch of prompts, encoded and quantized with lens, is what it would
be alone --

    z_u = encoder(wav[u:u+1, :, :lens[u]])                     (1, 256, T_u), T_u = out_len(lens[u])
    outs_u, codes_u, qbuf_u, spk_u = decoder(z_u, vq=True)     (B = 1: the position row is pe[0])
    z[u, :, :T_u] = z_u, codes[:, u, :T_u] = codes_u, outs / qbuf likewise, spk[u] = spk_u
    behind T_u: z, outs, qbuf exactly 0, codes exactly the pad code

so the reference of utterance u is always the oracle on that slice alone (orc.facodec_encode; _promptprofile.refs: the
fp64 and the fp32 oracle of the quantizers and the timbre encoder), never the code under test; each is computed once per
(shape, lengths, seed) and shared.  The bars are the existing ones, restated:

  encoder frames   f32: every frame <= F32_FRAME_BAR (1e-5) and the utterance <= 2e-5 rel-L2 (test_facodec_enc_gpu);
                   bf16: the worst frame <= FACTOR_ENC x the bf16 emulation's worst frame of that utterance alone
  codes            equal to the fp32 oracle's; a cell is excused only where the oracle's top-2 gap is < 1e-5 and the
                   cell is its frame's first mismatch, never more cells than the oracle's near-ties
                   (test_facodec_enc_gpu.py::test_vq_timbre_vs_oracle); where the oracle has no near-tie, none
  outs / qbuf      per frame against the fp64 oracle, bar_of(floor) = min(4 x the fp32 oracle's own distance, 1e-5)
  rows / spk       the same per last-LayerNorm row and for the speaker embedding (_promptprofile)

Weights: the calm-gain seeded encoder (weight-norm gains x the `facodec_calm` gain) and _promptprofile.decoder_sd().

Shapes (the smallest that reach every edge).  End to end, (B, n, lens) in samples; the stage lengths are
n -> n // 2 -> . // 4 -> (. + 1) // 5 -> (. + 1) // 5:"""
import torch

from _common import golden, seeded, orc, rel_l2
from _codecprofile import emulated_encode, frame_errors, assert_frame_profile, F32_FRAME_BAR, FACTOR_ENC, ENC_RATIOS  # noqa: F401
import _promptprofile as pp

E2E_SHAPES = [
    (3, 2600, (2600, 1999, 403)),          # 13 / 10 / 2 frames: a full, a middle and a very short utterance
    (4, 2048, (2048, 1985, 1984, 152)),    # 10 / 10 / 10 / 1: ends on and one past a 64-row activation tile; two lengths
                                           # the (. + 1) // 5 stages map to one count; the shortest legal input
    (1, 1300, (777,)),                     # 4: one utterance with padding
    (2, 13100, (13100, 12590)),            # 65 / 63: both sides of the 64-query / 64-key attention tile
]
# quantizers and timbre encoder alone on _promptprofile.case_input, (B, T, lens) in frames
VQ_SHAPES = [
    (3, 130, (130, 64, 1)),   # the third key chunk holding two keys; an end on the chunk edge; a single frame
    (2, 65, (65, 63)),        # key group 1 holding one key, and empty
    (4, 9, (1, 5, 8, 9)),     # M = 36; every end inside one 32-row tile; the short one first; T - 1 the closest miss
    (1, 7, (3,)),             # one utterance with padding: no dense shortcut
]
PAD = 1024          # the codebook size: the prior's vocab_size, which pad_prompts pads with
F32_REL = 2e-5      # test_facodec_enc_gpu.F32_REL
SPK_CHAIN = 1e-4    # test_facodec_enc_gpu.test_codes_from_hip_encoder_match_reference: spk rel-L2 behind the HIP encoder
MIN_N = 152


def out_len(n):
    for s in ENC_RATIOS:
        span = n + 2 * (s // 2 + s % 2) - 2 * s
        n = 0 if span < 0 else span // s + 1
    return n


def enc_sd():
    def make():
        from flamed.utils.seeded_init import scale_weight_norm_gains
        return scale_weight_norm_gains(seeded("facodec_encoder"), float(golden("facodec_calm")["gain"]))
    return pp.memo("promptlens_enc_sd", make)


def make_encoder(dtype, device):
    from _flamed_common import build_codec_encoder
    e = build_codec_encoder("cpu")
    e.load_state_dict(enc_sd())
    e.hip_dtype = dtype
    return e.to(device)


def make_decoder(device):
    from flamed.models.facodec import FACodecDecoder
    d = FACodecDecoder(in_channels=256, upsample_initial_channel=1024, up_ratios=[5, 5, 4, 2], vq_dim=256).eval()
    d.load_state_dict(pp.decoder_sd())
    d.hip_dtype = "f32"
    return d.to(device)


def wav_input(B, n, seed=0):
    return 0.1 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(1000 * B + n + 7919 * seed))


def _sd64():
    return pp.memo(("prompt_sd64", "seeded"), lambda: pp.to64(pp.decoder_sd()))


def vq_alone(x, lens):
    """Per utterance: _promptprofile.refs of its own frames alone (B = 1, so the oracle adds pe[0])."""
    return [pp.refs(pp.decoder_sd(), _sd64(), x[u:u + 1, :, :n].contiguous()) for u, n in enumerate(lens)]


def vq_case(B, T, lens, s=0):
    """(x (B, 256, T), [refs alone per utterance]) of one seeded input; computed once, never changed."""
    def make():
        x = pp.case_input(B, T, s)
        return x, vq_alone(x, lens)
    return pp.memo(("promptlens_vq", B, T, tuple(lens), s), make)


def e2e_case(B, n, lens, seed=0):
    """(wav (B, 1, n), [{"z": oracle alone, "emu": bf16 emulation alone, "vq": refs of z alone} per utterance])."""
    def make():
        wav = wav_input(B, n, seed)
        per = []
        with torch.inference_mode():
            for u, m in enumerate(lens):
                w = wav[u:u + 1, :, :m]
                z = orc.facodec_encode(enc_sd(), w)
                per.append({"z": z, "emu": emulated_encode(enc_sd(), w), "vq": pp.refs(pp.decoder_sd(), _sd64(), z)})
        return wav, per
    return pp.memo(("promptlens_e2e", B, n, tuple(lens), seed), make)


FILLS = ("zero", "big", "nan", "inf")


def filled(t, lens, kind, seed=99):
    """A copy of t (B, C, n) whose values behind every end are 0, 100 x randn, NaN or inf."""
    out = t.clone()
    g = torch.Generator().manual_seed(seed)
    for u, m in enumerate(lens):
        tail = out[u, :, m:]
        if kind == "zero":
            tail.zero_()
        elif kind == "big":
            tail.copy_(100 * torch.randn(tail.shape, generator=g))
        else:
            tail.fill_(float("nan") if kind == "nan" else float("inf"))
    return out


def check_encoder(mode, z, lens, per, label):
    """z (B, 256, T) of a ragged encode: every utterance against its own oracle alone, exact 0 behind its end."""
    z = torch.as_tensor(z)
    assert torch.isfinite(z).all(), f"{label}: non-finite output"
    for u, m in enumerate(lens):
        ref, emu = per[u]["z"], per[u]["emu"]
        Tu = ref.shape[2]
        assert Tu == out_len(m)
        zu = z[u:u + 1, :, :Tu]
        if mode == "f32":
            e, rel = frame_errors(zu, ref), rel_l2(zu, ref)
            print(f"{label} utterance {u} ({m} samples, {Tu} frames) f32: rel-L2 {rel:.2e}, frame max {float(e.max()):.2e}")
            assert float(e.max()) <= F32_FRAME_BAR and rel <= F32_REL, (u, float(e.max()), rel)
        else:
            assert_frame_profile(zu, ref, emu, f"{label} utterance {u} ({m} samples) bf16")
        tail = z[u, :, Tu:]
        assert torch.count_nonzero(tail) == 0, f"{label}: utterance {u} has non-zero frames behind its end"


def check_codes(codes, frames, refs, label, pad=PAD):
    """codes (n_q, B, T) against each utterance's fp32 oracle alone; the pad code behind every end (whole slices)."""
    codes = torch.as_tensor(codes)
    assert codes.dtype == torch.int64
    for u, Tu in enumerate(frames):
        r32 = refs[u]["r32"]
        cu = codes[:, u, :Tu]
        assert cu.shape == r32["codes"][:, 0].shape
        near = r32["gaps"][:, 0] < pp.NEAR_TIE
        neq = cu != r32["codes"][:, 0]
        first = neq & (neq.float().cumsum(0) == 1)
        print(f"{label} utterance {u} ({Tu} frames): {int(neq.sum())} cells differ, oracle near-ties {int(near.sum())}, "
              f"smallest gap {float(r32['gaps'].min()):.2e}")
        assert bool((near | ~first).all()), f"{label}: utterance {u}: code mismatch away from a near-tie"
        assert int(first.sum()) <= int(near.sum()), f"{label}: utterance {u}: more excused cells than the oracle has near-ties"
        assert bool((codes[:, u, Tu:] == pad).all()), f"{label}: utterance {u}: codes behind its end are not the pad code"


def check_quantized(o, frames, refs, label):
    """outs (B, 256, T), qbuf (G, B, 256, T) per frame against the fp64 oracle alone; exact 0 behind every end."""
    for u, Tu in enumerate(frames):
        r = refs[u]
        f = pp.floors(r)
        keep = (o["codes"][:, u, :Tu] == r["r64"]["codes"][:, 0]).all(0).unsqueeze(0)
        for name, out, ref, fl in [("outs", o["outs"], r["r64"]["outs"], f["outs"])] + \
                [(f"qbuf[{g}]", o["qbuf"][g], r["r64"]["qbuf"][g], f["qbuf"][g]) for g in range(3)]:
            assert torch.isfinite(out).all(), f"{label}: non-finite {name}"
            assert torch.count_nonzero(out[u, :, Tu:]) == 0, f"{label}: utterance {u}: {name} is not 0 behind its end"
            if not bool(keep.any()):
                continue
            e = float(pp.frame_err(out[u:u + 1, :, :Tu], ref, keep).max())
            print(f"{label} utterance {u} {name}: frame max {e:.3e}, floor {fl:.3e}, ratio {e / fl:.2f}")
            assert e <= pp.bar_of(fl), f"{label}: utterance {u}: {name} frame is {e:.3e} from the fp64 oracle, floor {fl:.3e}"


def check_timbre(o, frames, refs, label):
    """rows (B, T, 256; may be None) and spk (B, 256) against the fp64 oracle alone."""
    for u, Tu in enumerate(frames):
        r = refs[u]
        f = pp.floors(r)
        se = float(pp.spk_err(o["spk"][u:u + 1], r["r64"]["spk"], r["r64"]["rows"]).max())
        msg = f"{label} utterance {u} ({Tu} frames): spk {se:.3e}, floor {f['spk']:.3e}, ratio {se / f['spk']:.2f}"
        assert torch.isfinite(o["spk"]).all(), f"{label}: non-finite spk"
        if o.get("rows") is not None:
            assert torch.isfinite(o["rows"]).all(), f"{label}: non-finite rows"
            e = float(pp.row_err(o["rows"][u:u + 1, :Tu], r["r64"]["rows"]).max())
            msg += f"; row max {e:.3e}, floor {f['rows']:.3e}, ratio {e / f['rows']:.2f}"
            print(msg)
            assert e <= pp.bar_of(f["rows"]), f"{label}: utterance {u}: a row is {e:.3e} from the fp64 oracle, floor {f['rows']:.3e}"
        else:
            print(msg)
        assert se <= pp.bar_of(f["spk"]), f"{label}: utterance {u}: spk is {se:.3e} from the fp64 oracle, floor {f['spk']:.3e}"
