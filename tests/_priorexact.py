"""Exact lengths in the prior stage: the definition as oracle calls, one utterance at a time, shared by
tests/test_prior_exact_cpu.py and tests/test_prior_exact_gpu.py.

For utterance u of a padded batch (len_u phonemes, P_u prompt codes), with dn, sn the two (B, L) draws of the default:
  dur_u, sil_u = orc.pva_flow(enc[u:u+1, :len_u], mask of zeros, noise=(dn[u:u+1, :len_u], sn[u:u+1, :len_u]))
  x_u, T_u     = orc.length_regulate(enc[u, :len_u], frames(dur_u), frames(sil_u), [len_u])
  embs, logits = orc.prior_decode(x_u, [T_u], prompts[u:u+1, :, :P_u])

Bars (the project's own): log-durations rel-L2 <= 1e-5 per utterance and no integer-frame flip at a position further
than 1e-4 from a .5 boundary (tests/test_pva_gpu.py); the length regulator bit-exact; prior_embs / logits rel-L2
<= 1e-4 (f32) and <= 1e-2 (bf16) against the fp32 oracle (tests/test_prior_gpu.py).  At most ONE position per case may
sit within 1e-4 of a boundary (a cap on what may be excused, asserted by near_and_flips' callers)."""
import numpy as np
import torch

from _common import orc

DUR_BAR = 1e-5
DEC_BAR = {"f32": 1e-4, "bf16": 1e-2}


def zeros_mask(n):
    return torch.zeros(1, n, dtype=torch.bool)


def flow_alone(sd, enc, lens, dn, sn, nfe, temperature):
    """[(dur_u, sil_u)], each (len_u,), by the oracle on every utterance alone."""
    out = []
    with torch.inference_mode():
        for u, n in enumerate(lens):
            d, s = orc.pva_flow(sd, enc[u:u + 1, :n], zeros_mask(n), nfe, temperature,
                                noise=(dn[u:u + 1, :n], sn[u:u + 1, :n]))
            out.append((d[0], s[0]))
    return out


def near_and_flips(got, ref):
    """(positions of ref within 1e-4 of a .5 rounding boundary, integer-frame flips of got at the other positions)."""
    e = torch.exp(ref) - 1
    safe = (e - e.floor() - 0.5).abs() > 1e-4
    flips = int((orc.log_to_frames(got)[safe] != orc.log_to_frames(ref)[safe]).sum())
    return int((~safe).sum()), flips


def lr_alone(x, d, s, lens, log_domain=True):
    """orc.length_regulate of every utterance alone -> [(x_u (T_u, H), T_u)]; d, s: per-utterance 1-D tensors (log
    durations, or frame counts with log_domain False)."""
    out = []
    for u, n in enumerate(lens):
        pd = orc.log_to_frames(d[u][:n]) if log_domain else d[u][:n]
        sdur = orc.log_to_frames(s[u][:n]) if log_domain else s[u][:n]
        xo, tl = orc.length_regulate(x[u:u + 1, :n].detach().cpu().numpy(), pd.numpy()[None], sdur.numpy()[None],
                                     np.array([n], dtype=np.int64))
        out.append((torch.from_numpy(xo[0]), int(tl[0])))
    return out


def decode_alone(sd, x, tgt, prompts, plens, fn=None):
    """Padded (embs (B, nq, T, D), logits (B, V1, nq, T)) of every utterance decoded alone by `fn` (default
    orc.prior_decode) over x[u, :T_u] behind prompts[u, :, :P_u]; 0 behind every end."""
    fn = orc.prior_decode if fn is None else fn
    B, T = x.shape[:2]
    embs = logits = None
    with torch.inference_mode():
        for u in range(B):
            Tu, Pu = int(tgt[u]), int(plens[u])
            e, lg = fn(sd, x[u:u + 1, :Tu], torch.tensor([Tu]), prompts[u:u + 1, :, :Pu])[:2]
            if embs is None:
                embs = torch.zeros((B, e.shape[1], T, e.shape[3]), dtype=e.dtype)
                logits = torch.zeros((B, lg.shape[1], lg.shape[2], T), dtype=lg.dtype)
            embs[u, :, :Tu], logits[u, :, :, :Tu] = e[0], lg[0]
    return embs, logits


def pad_prompts(prompts, plens, pad):
    """prompts (B, nq, P) with the slots behind every utterance's own length set to the pad id."""
    out = prompts.clone()
    for u, n in enumerate(plens):
        out[u, :, n:] = pad
    return out
