"""torch.library custom-op layer over the HIP library (`flamed_hip::den_step` & co.).

Every hot-path entry point the modules dispatch to on ROCm is registered as a PyTorch custom op in the
`flamed_hip` namespace, so the calls are visible to the dispatcher: `torch.compile` (dynamo traces them
as single opaque nodes instead of graph-breaking on ctypes), FakeTensor / meta shape propagation, and
`torch.library.opcheck`.  The ops are thin: the work is done by the per-module owner objects
(`DenoiserHIP`, `CondFoldHIP`, `PvaHIP`, `FacDecoderHIP`, `EncoderHIP`, `VqHIP`, `PriorHIP`), which own the native handles and
their device-resident weight arenas.  An owner is passed to an op by an integer id (custom-op schemas
take tensors and scalars only); the registry holds weak references, so a dropped module frees its handle.

  op                                    reference function it stands for
  flamed_hip::den_velocity(id, x, t, c)            SimpleMLPAdaLN.forward          prob_generator.py:349-365
  flamed_hip::den_solve(id, xt, ts, spk, nfe)      ProbGenerator.sample Euler loop prob_generator.py:439-445
  flamed_hip::den_solve_rk2(id, xt, ts_eval, spk, nsteps, a)  the same loop, two-stage second-order solver
  flamed_hip::cond_fold(id, cond, mask)            QuantizerEncoding + ConditionDownSampler :167-205, 435-436
  flamed_hip::den_solve_lens(id, xt, ts, spk, nfe, lens)            exact lengths (no reference counterpart): every
  flamed_hip::den_solve_rk2_lens(id, xt, ts_eval, spk, nsteps, a, lens)  utterance of the padded batch solved / folded
  flamed_hip::cond_fold_exact(id, cond, mask)                       over its own frames only, as if alone
  flamed_hip::pva_flow(id, x, mask, dur, sil, ts, nfe)  PVA.sample Euler loops       pva.py:97-109
  flamed_hip::length_regulate(x, pd, sd, lens, max_len, log_domain)  LengthRegulator.LR  pva.py:125-166
  flamed_hip::pva_flow_exact(id, x, dur, sil, ts, nfe, lens)        exact lengths in the prior stage (no reference
  flamed_hip::length_regulate_exact(x, pd, sd, lens, max_len, log)  counterpart): every utterance flowed over its own
  flamed_hip::prior_decode_lens(id, x, mask, prompts, P, plens)     phonemes, padded phonemes repeat 0 frames, every
                                                   utterance decoded behind its own prompt, as if alone
  flamed_hip::fac_decode(id, x, spk)               FACodecDecoder.inference        facodec.py:630-638
  flamed_hip::fac_decode_lens(id, x, spk, lens)    exact lengths (no reference counterpart): every utterance of the
                                                   padded batch decoded over its own frames, as if alone; 0 behind it
  flamed_hip::enc_encode(id, x)                    FACodecEncoder.forward          facodec.py:158-243
  flamed_hip::vq_encode(id, x)                     FACodecDecoder.forward(vq=True) facodec.py:470-533
  flamed_hip::enc_encode_lens(id, x, lens)         exact lengths in the prompt stage (no reference counterpart): every
  flamed_hip::vq_encode_lens(id, x, lens, pad_code)  prompt of the padded batch encoded / quantized over its own samples /
                                                   frames, as if alone (position row pe[0] for every utterance)
  flamed_hip::prior_encode(id, texts, mask)        Encoder.forward (prior)         prior_generator.py:152-153
  flamed_hip::prior_decode(id, x, mask, prompts, P) bridge + decoders + head       prior_generator.py:165-188
  flamed_hip::noise_state(cond, seeds, lens, temperature, stream_id, B, T, C, device)  keyed noise (no reference
                                                   counterpart; opt-in): cond + temperature * n, n counter-based
                                                   normals keyed per utterance (flamed/utils/noise.py), 0 behind lens

None of the ops has an autograd formula: the modules route autograd (training) to their torch ops
before reaching here, exactly as the reference trains.  There is no CPU kernel: the ops are registered
for every device, and the owners raise if the HIP library is missing (no fallback).
"""
from __future__ import annotations

import itertools
import threading
import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor

_ids = itertools.count(1)
_owners: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()
_lock = threading.Lock()


def register(owner) -> int:
    """Give a HIP owner object an id the custom ops can carry."""
    with _lock:
        i = next(_ids)
        _owners[i] = owner
    return i


def owner(i: int):
    o = _owners.get(int(i))
    if o is None:
        raise RuntimeError(f"flamed_hip: no live HIP owner with id {i}")
    return o


# ---------------------------------------------------------------- denoiser

@torch.library.custom_op("flamed_hip::den_velocity", mutates_args=())
def den_velocity(oid: int, x: Tensor, t: Tensor, c: Tensor) -> Tensor:
    return owner(oid).velocity(x, t, c)


@den_velocity.register_fake
def _(oid, x, t, c):
    return x.new_empty(x.shape, dtype=x.dtype)


@torch.library.custom_op("flamed_hip::den_solve", mutates_args=())
def den_solve(oid: int, xt: Tensor, ts: Tensor, spk: Tensor, nfe: int) -> Tensor:
    return owner(oid).solve(xt, ts, spk, nfe)


@den_solve.register_fake
def _(oid, xt, ts, spk, nfe):
    return xt.new_empty(xt.shape, dtype=torch.float32)


@torch.library.custom_op("flamed_hip::den_solve_rk2", mutates_args=())
def den_solve_rk2(oid: int, xt: Tensor, ts_eval: Tensor, spk: Tensor, nsteps: int, a: float) -> Tensor:
    return owner(oid).solve_rk2(xt, ts_eval, spk, nsteps, a)


@den_solve_rk2.register_fake
def _(oid, xt, ts_eval, spk, nsteps, a):
    return xt.new_empty(xt.shape, dtype=torch.float32)


@torch.library.custom_op("flamed_hip::den_solve_lens", mutates_args=())
def den_solve_lens(oid: int, xt: Tensor, ts: Tensor, spk: Tensor, nfe: int, lens: List[int]) -> Tensor:
    return owner(oid).solve(xt, ts, spk, nfe, lens=lens)


@den_solve_lens.register_fake
def _(oid, xt, ts, spk, nfe, lens):
    return xt.new_empty(xt.shape, dtype=torch.float32)


@torch.library.custom_op("flamed_hip::den_solve_rk2_lens", mutates_args=())
def den_solve_rk2_lens(oid: int, xt: Tensor, ts_eval: Tensor, spk: Tensor, nsteps: int, a: float, lens: List[int]) -> Tensor:
    return owner(oid).solve_rk2(xt, ts_eval, spk, nsteps, a, lens=lens)


@den_solve_rk2_lens.register_fake
def _(oid, xt, ts_eval, spk, nsteps, a, lens):
    return xt.new_empty(xt.shape, dtype=torch.float32)


@torch.library.custom_op("flamed_hip::cond_fold", mutates_args=())
def cond_fold(oid: int, cond: Tensor, mask: Tensor) -> Tensor:
    return owner(oid).fold(cond, mask)


@cond_fold.register_fake
def _(oid, cond, mask):
    B, _, T, _ = cond.shape
    return cond.new_empty((B, T, owner(oid).pg.target_dim), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::cond_fold_exact", mutates_args=())
def cond_fold_exact(oid: int, cond: Tensor, mask: Tensor) -> Tensor:
    return owner(oid).fold(cond, mask, exact=True)


@cond_fold_exact.register_fake
def _(oid, cond, mask):
    B, _, T, _ = cond.shape
    return cond.new_empty((B, T, owner(oid).pg.target_dim), dtype=torch.float32)


# ---------------------------------------------------------------- PVA + length regulator

@torch.library.custom_op("flamed_hip::pva_flow", mutates_args=())
def pva_flow(oid: int, x: Tensor, src_mask: Tensor, dur_t: Tensor, sil_t: Tensor, ts: Tensor,
             nfe: int) -> Tuple[Tensor, Tensor]:
    return owner(oid).flow(x, src_mask, dur_t, sil_t, ts, nfe)


@pva_flow.register_fake
def _(oid, x, src_mask, dur_t, sil_t, ts, nfe):
    return (dur_t.new_empty(dur_t.shape, dtype=torch.float32), sil_t.new_empty(sil_t.shape, dtype=torch.float32))


@torch.library.custom_op("flamed_hip::length_regulate", mutates_args=())
def length_regulate(x: Tensor, phone: Tensor, sil: Tensor, src_lens: Tensor, max_len: int,
                    log_domain: bool) -> Tuple[Tensor, Tensor]:
    from .models.synthesizer.pva import hip_length_regulate_impl
    return hip_length_regulate_impl(x, phone, sil, src_lens, max_len, log_domain)


@length_regulate.register_fake
def _(x, phone, sil, src_lens, max_len, log_domain):
    B, _, H = x.shape
    # the regulated length is data-dependent unless max_len pins it (the reference's `.tolist()` sync)
    T = max_len if max_len else torch.library.get_ctx().new_dynamic_size()
    return x.new_empty((B, T, H)), src_lens.new_empty((B,), dtype=torch.int64)


@torch.library.custom_op("flamed_hip::pva_flow_exact", mutates_args=())
def pva_flow_exact(oid: int, x: Tensor, dur_t: Tensor, sil_t: Tensor, ts: Tensor, nfe: int,
                   lens: List[int]) -> Tuple[Tensor, Tensor]:
    return owner(oid).flow(x, None, dur_t, sil_t, ts, nfe, lens=lens)


@pva_flow_exact.register_fake
def _(oid, x, dur_t, sil_t, ts, nfe, lens):
    return (dur_t.new_empty(dur_t.shape, dtype=torch.float32), sil_t.new_empty(sil_t.shape, dtype=torch.float32))


@torch.library.custom_op("flamed_hip::length_regulate_exact", mutates_args=())
def length_regulate_exact(x: Tensor, phone: Tensor, sil: Tensor, src_lens: Tensor, max_len: int,
                          log_domain: bool) -> Tuple[Tensor, Tensor]:
    from .models.synthesizer.pva import hip_length_regulate_impl
    return hip_length_regulate_impl(x, phone, sil, src_lens, max_len, log_domain, exact=True)


@length_regulate_exact.register_fake
def _(x, phone, sil, src_lens, max_len, log_domain):
    B, _, H = x.shape
    T = max_len if max_len else torch.library.get_ctx().new_dynamic_size()
    return x.new_empty((B, T, H)), src_lens.new_empty((B,), dtype=torch.int64)


# ---------------------------------------------------------------- FaCodec

@torch.library.custom_op("flamed_hip::fac_decode", mutates_args=())
def fac_decode(oid: int, x: Tensor, spk: Tensor) -> Tensor:
    return owner(oid).decode(x, spk)


@fac_decode.register_fake
def _(oid, x, spk):
    B, _, T = x.shape
    return x.new_empty((B, 1, owner(oid).dec.hop_length * T), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::fac_decode_lens", mutates_args=())
def fac_decode_lens(oid: int, x: Tensor, spk: Tensor, lens: List[int]) -> Tensor:
    return owner(oid).decode(x, spk, lens=lens)


@fac_decode_lens.register_fake
def _(oid, x, spk, lens):
    B, _, T = x.shape
    return x.new_empty((B, 1, owner(oid).dec.hop_length * T), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::enc_encode", mutates_args=())
def enc_encode(oid: int, x: Tensor) -> Tensor:
    return owner(oid).encode(x)


@enc_encode.register_fake
def _(oid, x):
    o = owner(oid)
    B, _, n = x.shape
    return x.new_empty((B, o.enc.out_channels, o.out_len(n)), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::vq_encode", mutates_args=())
def vq_encode(oid: int, x: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return owner(oid).encode(x)


@vq_encode.register_fake
def _(oid, x):
    B, C, T = x.shape
    q = owner(oid).dec.quantizer
    nq = sum(len(r.layers) for r in q)
    return (x.new_empty((B, C, T)), x.new_empty((nq, B, T), dtype=torch.int64), x.new_empty((len(q), B, C, T)),
            x.new_empty((B, C)))


@torch.library.custom_op("flamed_hip::enc_encode_lens", mutates_args=())
def enc_encode_lens(oid: int, x: Tensor, lens: List[int]) -> Tensor:
    return owner(oid).encode(x, lens=lens)


@enc_encode_lens.register_fake
def _(oid, x, lens):
    o = owner(oid)
    B, _, n = x.shape
    return x.new_empty((B, o.enc.out_channels, o.out_len(n)), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::vq_encode_lens", mutates_args=())
def vq_encode_lens(oid: int, x: Tensor, lens: List[int], pad_code: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return owner(oid).encode(x, lens=lens, pad_code=pad_code)


@vq_encode_lens.register_fake
def _(oid, x, lens, pad_code):
    B, C, T = x.shape
    q = owner(oid).dec.quantizer
    nq = sum(len(r.layers) for r in q)
    return (x.new_empty((B, C, T)), x.new_empty((nq, B, T), dtype=torch.int64), x.new_empty((len(q), B, C, T)),
            x.new_empty((B, C)))


# ---------------------------------------------------------------- prior transformer stack

@torch.library.custom_op("flamed_hip::prior_encode", mutates_args=())
def prior_encode(oid: int, texts: Tensor, src_mask: Tensor) -> Tensor:
    return owner(oid).encode(texts, src_mask)


@prior_encode.register_fake
def _(oid, texts, src_mask):
    B, n = texts.shape
    return texts.new_empty((B, n, owner(oid).pg.encoder.d_model), dtype=torch.float32)


@torch.library.custom_op("flamed_hip::prior_decode", mutates_args=())
def prior_decode(oid: int, x: Tensor, tgt_mask: Tensor, prompts: Tensor, prompts_len: int) -> Tuple[Tensor, Tensor]:
    return owner(oid).decode(x, tgt_mask, prompts, prompts_len)


@prior_decode.register_fake
def _(oid, x, tgt_mask, prompts, prompts_len):
    B, T, _ = x.shape
    pg = owner(oid).pg
    nq, D, V1 = len(pg.prior_decoder), pg.shared_decoder.d_model, pg.head.weight.shape[0]
    return x.new_empty((B, nq, T, D)), x.new_empty((B, V1, nq, T))


@torch.library.custom_op("flamed_hip::prior_decode_lens", mutates_args=())
def prior_decode_lens(oid: int, x: Tensor, tgt_mask: Tensor, prompts: Tensor, prompts_len: int,
                      prompt_lens: List[int]) -> Tuple[Tensor, Tensor]:
    return owner(oid).decode(x, tgt_mask, prompts, prompts_len, prompt_lens=prompt_lens)


@prior_decode_lens.register_fake
def _(oid, x, tgt_mask, prompts, prompts_len, prompt_lens):
    B, T, _ = x.shape
    pg = owner(oid).pg
    nq, D, V1 = len(pg.prior_decoder), pg.shared_decoder.d_model, pg.head.weight.shape[0]
    return x.new_empty((B, nq, T, D)), x.new_empty((B, V1, nq, T))


# ---------------------------------------------------------------- keyed noise

@torch.library.custom_op("flamed_hip::noise_state", mutates_args=())
def noise_state(cond: Optional[Tensor], seeds: List[int], lens: Optional[List[int]], temperature: float, stream_id: int,
                B: int, T: int, C: int, device: torch.device) -> Tensor:
    # (a schema int is signed 64-bit: seeds travel as their two's-complement images)
    from .utils.noise import hip_noise_state
    return hip_noise_state(cond, [s & 0xFFFFFFFFFFFFFFFF for s in seeds], lens, temperature, stream_id, (B, T, C), device)


@noise_state.register_fake
def _(cond, seeds, lens, temperature, stream_id, B, T, C, device):
    return torch.empty((B, T, C), dtype=torch.float32, device=device)


# the ops the model modules call themselves (noise_state is reached through flamed.utils.noise.noise_state)
OPS = ("den_velocity", "den_solve", "den_solve_rk2", "den_solve_lens", "den_solve_rk2_lens", "cond_fold", "cond_fold_exact",
       "pva_flow", "length_regulate", "fac_decode", "fac_decode_lens", "enc_encode", "vq_encode", "prior_encode", "prior_decode",
       "pva_flow_exact", "length_regulate_exact", "prior_decode_lens", "enc_encode_lens", "vq_encode_lens")
