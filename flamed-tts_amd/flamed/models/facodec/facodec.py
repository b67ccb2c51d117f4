"""FaCodec encoder + decoder (drop-in for reference flamed/models/facodec/facodec.py).

Implemented with the reference's module tree and state-dict keys:
  * `FACodecDecoder.inference` (reference :630-638), the waveform decoder used by
    Flamed.sample_batch (`model.*` with weight-norm `weight_g`/`weight_v`, alias-free filter buffers,
    `timbre_linear.*`).  On a CUDA (ROCm) device the whole decoder runs in the gfx950 HIP library
    (weight norm folded at load, implicit-GEMM convs on MFMA, polyphase ConvTranspose, fused
    Activation1d, graph-captured); the library is mandatory there.
  * The prompt-encoding path: `FACodecEncoder.forward` (reference :158-244)
    and `FACodecDecoder.forward(x, vq=True)` (:509-530): the prosody / content / residual factorized
    RVQs (`quantizer.*`) and the timbre transformer (`timbre_encoder.*`), returning the 6 code streams
    and the speaker embedding that Flamed.sample feeds to the prior.

Not implemented: the training-only predictor heads (`f0_predictor`, `phone_predictor`,
`res_*_predictor`, `x_timbre_predictor`, used only by `forward(vq=False)`).  Their checkpoint entries are
accepted by `load_state_dict` and kept in `self.unused_state` so the released checkpoint loads.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils import weight_norm

from flamed import _native as nat
from flamed import ops
from .alias_free_torch import Activation1d
from .quantize import ResidualVQ
from .transformer import TransformerEncoder


def WNConv1d(*args, **kwargs):
    return weight_norm(nn.Conv1d(*args, **kwargs))


def WNConvTranspose1d(*args, **kwargs):
    return weight_norm(nn.ConvTranspose1d(*args, **kwargs))


class SnakeBeta(nn.Module):
    """x + 1/(beta + 1e-9) * sin(alpha * x)^2 with per-channel (optionally log-scale) alpha, beta
    (reference :57-118)."""

    def __init__(self, in_features, alpha=1.0, alpha_trainable=True, alpha_logscale=False):
        super().__init__()
        self.in_features = in_features
        self.alpha_logscale = alpha_logscale
        init = torch.zeros(in_features) if alpha_logscale else torch.ones(in_features)
        self.alpha = nn.Parameter(init * alpha)
        self.beta = nn.Parameter(init.clone() * alpha)
        self.alpha.requires_grad = alpha_trainable
        self.beta.requires_grad = alpha_trainable
        self.no_div_by_zero = 0.000000001

    def forward(self, x):
        a = self.alpha.unsqueeze(0).unsqueeze(-1)
        b = self.beta.unsqueeze(0).unsqueeze(-1)
        if self.alpha_logscale:
            a, b = torch.exp(a), torch.exp(b)
        return x + (1.0 / (b + self.no_div_by_zero)) * torch.pow(torch.sin(x * a), 2)


def _act(dim):
    return Activation1d(activation=SnakeBeta(dim, alpha_logscale=True))


class ResidualUnit(nn.Module):
    """x + conv1x1(act(conv7_dilated(act(x)))) (reference :121-133)."""

    def __init__(self, dim: int = 16, dilation: int = 1):
        super().__init__()
        self.block = nn.Sequential(_act(dim), WNConv1d(dim, dim, kernel_size=7, dilation=dilation,
                                                       padding=((7 - 1) * dilation) // 2),
                                   _act(dim), WNConv1d(dim, dim, kernel_size=1))

    def forward(self, x):
        return x + self.block(x)


class DecoderBlock(nn.Module):
    """act -> ConvTranspose(k=2s, stride s) -> 3 residual units (dilation 1, 3, 9) (reference :246-265)."""

    def __init__(self, input_dim: int = 16, output_dim: int = 8, stride: int = 1):
        super().__init__()
        self.block = nn.Sequential(
            _act(input_dim),
            WNConvTranspose1d(input_dim, output_dim, kernel_size=2 * stride, stride=stride,
                              padding=stride // 2 + stride % 2, output_padding=stride % 2),
            ResidualUnit(output_dim, dilation=1), ResidualUnit(output_dim, dilation=3),
            ResidualUnit(output_dim, dilation=9))

    def forward(self, x):
        return self.block(x)


class EncoderBlock(nn.Module):
    """3 residual units (dilation 1, 3, 9) at dim//2 -> act -> strided WNConv1d(k=2s) to dim
    (reference :136-155)."""

    def __init__(self, dim: int = 16, stride: int = 1):
        super().__init__()
        half = dim // 2
        self.block = nn.Sequential(
            ResidualUnit(half, dilation=1), ResidualUnit(half, dilation=3), ResidualUnit(half, dilation=9),
            _act(half),
            WNConv1d(half, dim, kernel_size=2 * stride, stride=stride, padding=stride // 2 + stride % 2))

    def forward(self, x):
        return self.block(x)


class FACodecEncoder(nn.Module):
    """Waveform (B, 1, n) -> (B, out_channels, n/hop) (reference :158-244)."""

    default_ckpt = os.path.join(os.path.dirname(__file__), "checkpoints", "ns3_facodec_encoder.bin")

    @classmethod
    def from_pretrained(cls, cfg, ckpt_path=None):
        enc = cls(ngf=cfg["ngf"], up_ratios=cfg["up_ratios"], out_channels=cfg["out_channels"])
        sd = torch.load(ckpt_path or cls.default_ckpt, map_location=cfg.get("device", "cpu"), weights_only=True)
        enc.load_state_dict(sd)
        return enc.eval()

    def __init__(self, ngf=32, up_ratios=(2, 4, 5, 5), out_channels=1024):
        super().__init__()
        self.hop_length = int(np.prod(up_ratios))
        self.up_ratios = list(up_ratios)
        self.ngf = ngf
        self.out_channels = out_channels
        d = ngf
        layers: List[nn.Module] = [WNConv1d(1, d, kernel_size=7, padding=3)]
        for stride in self.up_ratios:
            d *= 2
            layers.append(EncoderBlock(d, stride=stride))
        layers += [_act(d), WNConv1d(d, out_channels, kernel_size=3, padding=1)]
        self.block = nn.Sequential(*layers)
        self.enc_dim = d
        # On ROCm tensors the encoder runs in the HIP library; "f32" (default) is the exact-fp32 MFMA
        # mode: the RVQ argmax downstream turns small activation errors into different prompt codes.
        self.hip_dtype = "f32"
        self.hip_graph = True
        self._hip = None
        self._vq_hip = None
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.constant_(m.bias, 0)

    def hip_invalidate(self):
        """Force the next HIP call to re-pack the weights (load_state_dict does this by itself)."""
        if self._hip is not None:
            self._hip._sig = None
        if self._vq_hip is not None:
            self._vq_hip._sig = None

    def _load_from_state_dict(self, *args, **kwargs):
        self.hip_invalidate()  # load_state_dict copies in place: same pointers, maybe no version bump
        super()._load_from_state_dict(*args, **kwargs)

    def _use_hip(self, x):
        if not x.is_cuda or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return False
        return self.hip_dims_ok()

    def hip_dims_ok(self) -> bool:
        """flamed_enc_create specialises these dims; otherwise the encoder keeps its torch ops."""
        return nat.supported("enc", self.ngf, len(self.up_ratios), tuple(self.up_ratios), self.out_channels,
                             nat.dtype_code(self.hip_dtype))

    def out_len(self, n: int) -> int:
        """Frames the encoder makes of n samples: Conv1d(k = 2s, stride s, pad ceil(s / 2)) at every stride, 0 where a
        kernel does not fit its padded input (the same arithmetic as flamed_enc_out_len, on the host for both paths)."""
        n = int(n)
        for s in self.up_ratios:
            span = n + 2 * (s // 2 + s % 2) - 2 * s
            n = 0 if span < 0 else span // s + 1
        return n

    def min_len(self) -> int:
        """The shortest input that leaves a frame (152 samples for ratios 2, 4, 5, 5)."""
        need = 1
        for s in reversed(self.up_ratios):
            need = max(1, (need - 1) * s + 2 * s - 2 * (s // 2 + s % 2))
        return need

    def forward(self, x, lens=None):
        """waveform (B, 1, n) -> (B, out_channels, T) (reference :215-217).

        lens (exact lengths; B sample counts in min_len()..n, a sequence or a 1-D integer tensor): utterance u of the
        padded batch is encoded over its own lens[u] samples, so z[u, :, :T_u] with T_u = out_len(lens[u]) is
        forward(x[u:u+1, :, :lens[u]]) and z[u, :, T_u:] is exactly 0; nothing stored in x[u, :, lens[u]:] is read.
        Every length equal to n is the call without lens."""
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
            for u, n in enumerate(lens):
                if self.out_len(n) <= 0:
                    raise ValueError(f"lens[{u}] = {n} samples is too short for the encoder (at least {self.min_len()})")
            if all(n == x.shape[2] for n in lens):
                lens = None
        if self._use_hip(x):
            if self._hip is None or self._hip.dtype_name != self.hip_dtype:
                self._hip = EncoderHIP(self, self.hip_dtype)
            if lens is not None:
                return ops.enc_encode_lens(self._hip.oid, x, lens)
            return ops.enc_encode(self._hip.oid, x)
        if lens is not None:  # the definition: one utterance after another, alone
            T = self.out_len(x.shape[2])
            return torch.cat([F.pad(self.block(x[u:u + 1, :, :n]), (0, T - self.out_len(n))) for u, n in enumerate(lens)], dim=0)
        return self.block(x)

    def inference(self, x, lens=None):
        return self.forward(x, lens)


class FACodecDecoder(nn.Module):
    """FaCodec decoder (reference :268-660): waveform decoder + prompt-side quantizers / timbre encoder."""

    default_ckpt = os.path.join(os.path.dirname(__file__), "checkpoints", "ns3_facodec_decoder.bin")

    @classmethod
    def from_pretrained(cls, cfg, ckpt_path=None):
        dec = cls(in_channels=cfg["in_channels"], upsample_initial_channel=cfg["upsample_initial_channel"],
                  ngf=cfg["ngf"], up_ratios=cfg["up_ratios"], vq_num_q_c=cfg["vq_num_q_c"],
                  vq_num_q_p=cfg["vq_num_q_p"], vq_num_q_r=cfg["vq_num_q_r"], vq_dim=cfg["vq_dim"],
                  codebook_dim=cfg["codebook_dim"], codebook_size_prosody=cfg["codebook_size_prosody"],
                  codebook_size_content=cfg["codebook_size_content"],
                  codebook_size_residual=cfg["codebook_size_residual"], use_gr_x_timbre=cfg["use_gr_x_timbre"],
                  use_gr_residual_f0=cfg["use_gr_residual_f0"], use_gr_residual_phone=cfg["use_gr_residual_phone"])
        sd = torch.load(ckpt_path or cls.default_ckpt, map_location=cfg.get("device", "cpu"), weights_only=True)
        dec.load_state_dict(sd)
        return dec.eval()

    def __init__(self, in_channels=256, upsample_initial_channel=1536, ngf=32, up_ratios=(5, 5, 4, 2),
                 vq_num_q_c=2, vq_num_q_p=1, vq_num_q_r=3, vq_dim=1024, vq_commit_weight=0.005,
                 vq_weight_init=False, vq_full_commit_loss=False, codebook_dim=8, codebook_size_prosody=10,
                 codebook_size_content=10, codebook_size_residual=10, quantizer_dropout=0.0, dropout_type="linear",
                 use_gr_content_f0=False, use_gr_prosody_phone=False, use_gr_residual_f0=False,
                 use_gr_residual_phone=False, use_gr_x_timbre=False, use_random_mask_residual=True,
                 prob_random_mask_residual=0.75):
        super().__init__()
        self.in_channels = in_channels
        self.upsample_initial_channel = upsample_initial_channel
        self.vq_num_q_p, self.vq_num_q_c, self.vq_num_q_r = vq_num_q_p, vq_num_q_c, vq_num_q_r
        self.codebook_size_prosody = codebook_size_prosody
        self.codebook_size_content = codebook_size_content
        self.codebook_size_residual = codebook_size_residual
        self.use_random_mask_residual = use_random_mask_residual
        self.prob_random_mask_residual = prob_random_mask_residual
        self.use_gr_content_f0, self.use_gr_prosody_phone = use_gr_content_f0, use_gr_prosody_phone
        self.use_gr_residual_f0, self.use_gr_residual_phone = use_gr_residual_f0, use_gr_residual_phone
        self.use_gr_x_timbre = use_gr_x_timbre
        vq_kw = dict(dim=vq_dim, codebook_dim=codebook_dim, threshold_ema_dead_code=2, commitment=vq_commit_weight,
                     weight_init=vq_weight_init, full_commit_loss=vq_full_commit_loss,
                     quantizer_dropout=quantizer_dropout, dropout_type=dropout_type)
        self.quantizer = nn.ModuleList([
            ResidualVQ(num_quantizers=vq_num_q_p, codebook_size=codebook_size_prosody, **vq_kw),
            ResidualVQ(num_quantizers=vq_num_q_c, codebook_size=codebook_size_content, **vq_kw)])
        if vq_num_q_r > 0:
            self.quantizer.append(ResidualVQ(num_quantizers=vq_num_q_r, codebook_size=codebook_size_residual, **vq_kw))
        self.hop_length = int(np.prod(up_ratios))
        self.ngf = ngf
        self.up_ratios = list(up_ratios)
        ch = upsample_initial_channel
        layers: List[nn.Module] = [WNConv1d(in_channels, ch, kernel_size=7, padding=3)]
        out_dim = ch
        for i, stride in enumerate(self.up_ratios):
            layers.append(DecoderBlock(ch // 2 ** i, ch // 2 ** (i + 1), stride))
            out_dim = ch // 2 ** (i + 1)
        layers += [_act(out_dim), WNConv1d(out_dim, 1, kernel_size=7, padding=3), nn.Tanh()]
        self.model = nn.Sequential(*layers)
        self.timbre_encoder = TransformerEncoder(enc_emb_tokens=None, encoder_layer=4, encoder_hidden=256,
                                                 encoder_head=4, conv_filter_size=1024, conv_kernel_size=5,
                                                 encoder_dropout=0.1, use_cln=False)
        self.timbre_linear = nn.Linear(in_channels, in_channels * 2)
        with torch.no_grad():
            self.timbre_linear.bias[:in_channels] = 1
            self.timbre_linear.bias[in_channels:] = 0
        self.timbre_norm = nn.LayerNorm(in_channels, elementwise_affine=False)
        self.unused_state: Dict[str, torch.Tensor] = {}
        self.hip_dtype = "bf16"
        self.hip_graph = True
        self._hip = None
        self._vq_hip = None
        for m in self.modules():
            if isinstance(m, nn.Conv1d):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.constant_(m.bias, 0)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        own = set(self.state_dict().keys())
        extra = {k: v for k, v in state_dict.items() if k not in own}
        self.unused_state = extra
        return super().load_state_dict({k: v for k, v in state_dict.items() if k in own}, strict=strict, assign=assign)

    def hip_invalidate(self):
        """Force the next HIP call to re-pack the weights (load_state_dict does this by itself)."""
        if self._hip is not None:
            self._hip._sig = None
        if self._vq_hip is not None:
            self._vq_hip._sig = None

    def _load_from_state_dict(self, *args, **kwargs):
        self.hip_invalidate()  # load_state_dict copies in place: same pointers, maybe no version bump
        super()._load_from_state_dict(*args, **kwargs)

    def _use_hip(self, x):
        if not x.is_cuda or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return False
        return self.hip_dims_ok()

    def hip_dims_ok(self) -> bool:
        """flamed_fac_create specialises these dims; otherwise the decoder keeps its torch ops."""
        return nat.supported("fac", self.in_channels, self.upsample_initial_channel, len(self.up_ratios),
                             tuple(self.up_ratios), nat.dtype_code(self.hip_dtype))

    def _vq_hip_ok(self, x, n_quantizers):
        """The HIP prompt path covers the eval quantizers with every layer and the non-conditional timbre
        encoder; anything else (training, n_quantizers < all, use_cln, dims flamed_vq_create does not
        specialise) stays on the torch modules."""
        te = self.timbre_encoder
        full = n_quantizers is None or all(n_quantizers >= q.num_quantizers for q in self.quantizer)
        if not (x.is_cuda and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))):
            return False
        if not full or self.quantizer.training or te.use_cln:
            return False
        d = VqHIP.dims_of(self)
        return nat.supported("vq", tuple(d), len(d))

    def quantize(self, x, n_quantizers=None):
        """prosody and content RVQs on x, residual RVQ on x - (prosody + content) (reference :470-507)."""
        outs, qs, losses, qbuf = 0, [], [], []
        for i, q in enumerate(self.quantizer):
            inp = x if i < 2 else x - (qbuf[0] + qbuf[1]).detach()
            out, idx, loss, quantized = q(inp, n_quantizers=n_quantizers)
            outs = outs + out
            qs.append(idx)
            qbuf.append(quantized.sum(0))
            losses.append(loss)
        return outs, torch.cat(qs, dim=0), torch.cat(losses, dim=0), qbuf

    def forward(self, x, vq=True, get_vq=False, eval_vq=True, speaker_embedding=None, n_quantizers=None,
                quantized=None, lens=None, pad_code=None):
        """Prompt encoding (reference :509-530): encoder output (B, C, T) ->
        (quantized sum, codes (n_q, B, T), commit losses, per-RVQ quantized, speaker embedding (B, C)).

        lens (exact lengths; B frame counts in 1..T): utterance u of the padded batch is quantized and its speaker
        embedding taken over its own lens[u] frames, as forward(x[u:u+1, :, :lens[u]]) gives them; behind its end the
        quantized tensors are exactly 0 and the codes are pad_code (default: the codebook size, the prior's vocab_size,
        which pad_prompts uses); nothing stored in x[u, :, lens[u]:] is read.  POSITION ROW: without lens the timbre
        encoder keeps the reference's `x + pe[:B]`, which indexes the position table by the batch index, so utterance b
        gets pe[b] and not even equal-length prompts get their solo speaker embedding.  With lens every utterance gets
        pe[0], the row it gets alone; for B > 1 the call with lens is therefore never the call without, not even with
        every length equal to T.  At B = 1 with lens[0] == T it is the call without lens."""
        if get_vq:
            return self.quantizer.get_emb() if hasattr(self.quantizer, "get_emb") else [q.get_emb() for q in self.quantizer]
        if vq is not True:
            raise NotImplementedError("FACodecDecoder.forward(vq=False) needs the training-only predictor heads, "
                                      "which this build does not implement")
        if eval_vq:
            self.quantizer.eval()
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
            if pad_code is None:
                pad_code = max(q.layers[0]._codebook.weight.shape[0] for q in self.quantizer)
            if len(lens) == 1 and lens[0] == x.shape[2]:
                lens = None
        if self._vq_hip_ok(x, n_quantizers):
            if self._vq_hip is None:
                self._vq_hip = VqHIP(self)
            if lens is not None:
                outs, qs, qb, spk = ops.vq_encode_lens(self._vq_hip.oid, x, lens, int(pad_code))
            else:
                outs, qs, qb, spk = ops.vq_encode(self._vq_hip.oid, x)
            commit_loss = torch.zeros(qs.shape[0], device=x.device)
            return outs, qs, commit_loss, list(qb.unbind(0)), spk
        if lens is not None:  # the definition: one utterance after another, alone (each at batch index 0: pe[0])
            T = x.shape[2]
            solo = [self._forward_torch(x[u:u + 1, :, :n], n_quantizers) for u, n in enumerate(lens)]
            outs = torch.cat([F.pad(r[0], (0, T - n)) for r, n in zip(solo, lens)], dim=0)
            qs = torch.cat([F.pad(r[1], (0, T - n), value=int(pad_code)) for r, n in zip(solo, lens)], dim=1)
            commit_loss = torch.stack([r[2] for r in solo]).mean(0)
            qbuf = [torch.cat([F.pad(r[3][g], (0, T - n)) for r, n in zip(solo, lens)], dim=0) for g in range(len(self.quantizer))]
            return outs, qs, commit_loss, qbuf, torch.cat([r[4] for r in solo], dim=0)
        return self._forward_torch(x, n_quantizers)

    def _forward_torch(self, x, n_quantizers):
        outs, qs, commit_loss, qbuf = self.quantize(x, n_quantizers=n_quantizers)
        spk = self.timbre_encoder(x.transpose(1, 2), None, None).transpose(1, 2).mean(dim=2)
        return outs, qs, commit_loss, qbuf, spk

    def vq2emb(self, vq, use_residual_code=True):
        """codes (n_q, B, T) -> summed out-projected code vectors (reference :618-628)."""
        self.quantizer = self.quantizer.eval()
        p, c = self.vq_num_q_p, self.vq_num_q_c
        out = self.quantizer[0].vq2emb(vq[0:p]) + self.quantizer[1].vq2emb(vq[p:p + c])
        if self.vq_num_q_r > 0 and use_residual_code:
            out = out + self.quantizer[2].vq2emb(vq[p + c:])
        return out

    def inference(self, x, speaker_embedding, lens=None):
        """latents (B, in_channels, T), speaker (B, in_channels) -> wav (B, 1, hop*T).

        lens (exact lengths; B integers in 1..T, a sequence or a 1-D integer tensor): utterance u of the padded batch
        is decoded over its own lens[u] frames, so wav[u, :, :hop*lens[u]] is inference(x[u:u+1, :, :lens[u]],
        speaker_embedding[u:u+1]) and wav[u, :, hop*lens[u]:] is exactly 0; nothing stored in x[u, :, lens[u]:] is
        read.  Every length equal to T is the call without lens."""
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
            if all(n == x.shape[2] for n in lens):
                lens = None
        if self._use_hip(x):
            if self._hip is None or self._hip.dtype_name != self.hip_dtype:
                self._hip = FacDecoderHIP(self, self.hip_dtype)
            if lens is not None:
                return ops.fac_decode_lens(self._hip.oid, x, speaker_embedding, lens)
            return ops.fac_decode(self._hip.oid, x, speaker_embedding)
        if lens is not None:  # the definition: one utterance after another, alone
            T, hop = x.shape[2], self.hop_length
            return torch.cat([F.pad(self._inference_torch(x[u:u + 1, :, :n], speaker_embedding[u:u + 1]), (0, hop * (T - n)))
                              for u, n in enumerate(lens)], dim=0)
        return self._inference_torch(x, speaker_embedding)

    def _inference_torch(self, x, speaker_embedding):
        gamma, beta = self.timbre_linear(speaker_embedding).unsqueeze(2).chunk(2, 1)
        h = self.timbre_norm(x.transpose(1, 2)).transpose(1, 2)
        return self.model(h * gamma + beta)


def check_lens(lens, B: int, T: int) -> List[int]:
    """The lengths of an exact-lengths decode as a list of B ints in 1..T; ValueError otherwise (a wrong count, a
    non-integer, a length outside 1..T), before anything is launched."""
    if isinstance(lens, torch.Tensor):
        if lens.dim() != 1 or lens.dtype.is_floating_point or lens.dtype.is_complex or lens.dtype == torch.bool:
            raise ValueError(f"lens must be a 1-D integer tensor, got shape {tuple(lens.shape)} dtype {lens.dtype}")
        lens = lens.tolist()
    else:
        try:
            lens = list(lens)
        except TypeError:
            raise ValueError(f"lens must be a sequence of {B} integers or a 1-D integer tensor, got {type(lens).__name__}") from None
    if len(lens) != B:
        raise ValueError(f"lens holds {len(lens)} lengths for a batch of {B}")
    out = []
    for u, n in enumerate(lens):
        if isinstance(n, torch.Tensor) and n.numel() == 1 and not (n.dtype.is_floating_point or n.dtype == torch.bool):
            n = n.item()
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError(f"lens[{u}] = {n!r} is not an integer")
        if not 1 <= int(n) <= T:
            raise ValueError(f"lens[{u}] = {int(n)} is outside 1..T = {T}")
        out.append(int(n))
    return out


def fac_weight_list(dec: FACodecDecoder) -> List[torch.Tensor]:
    """Weights in the order flamed_fac_load expects (include/flamed_hip.h)."""

    def act(a):
        return [a.act.alpha, a.act.beta, a.upsample.filter, a.downsample.lowpass.filter]

    def wn(c):
        return [c.weight_g, c.weight_v, c.bias]

    m = dec.model
    w = [dec.timbre_linear.weight, dec.timbre_linear.bias] + wn(m[0])
    nup = len(dec.up_ratios)
    for i in range(nup):
        blk = m[1 + i].block
        w += act(blk[0]) + wn(blk[1])
        for j in range(2, 5):
            ru = blk[j].block
            w += act(ru[0]) + wn(ru[1]) + act(ru[2]) + wn(ru[3])
    w += act(m[1 + nup]) + wn(m[2 + nup])
    return w


class FacDecoderHIP:
    """Owns one flamed_fac_t handle."""

    def __init__(self, dec: FACodecDecoder, dtype_name: str):
        self.dec = dec
        self.dtype_name = dtype_name
        self.handle = None
        self._sig = None
        self._keep = []
        self.ws = nat.Workspace()
        self._bufs = {}
        self.oid = ops.register(self)  # torch.ops.flamed_hip.fac_decode / enc_encode

    def __del__(self):
        try:
            if self.handle is not None:
                nat.destroy(self.handle, "flamed_fac_destroy")
        except Exception:
            pass

    def _ensure(self, dev):
        params = fac_weight_list(self.dec)
        sig = tuple((p.data_ptr(), nat.tensor_version(p)) for p in params) + (str(dev),)
        if sig == self._sig:
            return
        L = nat.lib()
        if self.handle is None:
            h = ctypes.c_void_p()
            ups = (ctypes.c_int * len(self.dec.up_ratios))(*self.dec.up_ratios)
            nat.check(L.flamed_fac_create(self.dec.in_channels, self.dec.upsample_initial_channel,
                                          len(self.dec.up_ratios), ups, nat.dtype_code(self.dtype_name),
                                          ctypes.byref(h)), "flamed_fac_create")
            self.handle = h
            nat.track(h, "flamed_fac_destroy")
        keep = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
        arr = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        nat.check(L.flamed_fac_load(self.handle, arr, len(keep), nat.stream_ptr(dev)), "flamed_fac_load")
        self._keep = keep
        self._sig = sig
        self._bufs = {}

    def decode(self, x, spk, lens=None):
        """lens: None, or B ints in 1..T (flamed_fac_decode_lens: each utterance over its own frames, 0 behind it)."""
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
        dev = x.device
        self._ensure(dev)
        B, C, T = x.shape
        key = (B, T)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = {"x": torch.empty((B, C, T), dtype=torch.float32, device=dev),
                    "s": torch.empty((B, C), dtype=torch.float32, device=dev),
                    "wav": torch.empty((B, 1, self.dec.hop_length * T), dtype=torch.float32, device=dev)}
            self._bufs = {key: bufs}
        bufs["x"].copy_(x)
        bufs["s"].copy_(spk)
        L = nat.lib()
        ws = self.ws.get(L.flamed_fac_workspace_size(self.handle, B, T), dev)
        if lens is not None:
            nat.check(L.flamed_fac_decode_lens(self.handle, nat.ptr(bufs["x"]), nat.ptr(bufs["s"]), B, T,
                                               (ctypes.c_int * B)(*lens), nat.ptr(bufs["wav"]), nat.ptr(ws), ws.numel(),
                                               int(bool(self.dec.hip_graph)), nat.stream_ptr(dev)),
                      "flamed_fac_decode_lens")
        else:
            nat.check(L.flamed_fac_decode(self.handle, nat.ptr(bufs["x"]), nat.ptr(bufs["s"]), B, T, nat.ptr(bufs["wav"]),
                                          nat.ptr(ws), ws.numel(), int(bool(self.dec.hip_graph)), nat.stream_ptr(dev)),
                      "flamed_fac_decode")
        return bufs["wav"].clone()


def enc_weight_list(enc: FACodecEncoder) -> List[torch.Tensor]:
    """Weights in the order flamed_enc_load expects (include/flamed_hip.h)."""

    def act(a):
        return [a.act.alpha, a.act.beta, a.upsample.filter, a.downsample.lowpass.filter]

    def wn(c):
        return [c.weight_g, c.weight_v, c.bias]

    b = enc.block
    w = wn(b[0])
    for i in range(len(enc.up_ratios)):
        blk = b[1 + i].block
        for j in range(3):
            ru = blk[j].block
            w += act(ru[0]) + wn(ru[1]) + act(ru[2]) + wn(ru[3])
        w += act(blk[3]) + wn(blk[4])
    n = len(enc.up_ratios) + 1
    w += act(b[n]) + wn(b[n + 1])
    return w


class EncoderHIP:
    """Owns one flamed_enc_t handle (FaCodec encoder on gfx950)."""

    def __init__(self, enc: FACodecEncoder, dtype_name: str):
        self.enc = enc
        self.dtype_name = dtype_name
        self.handle = None
        self._sig = None
        self._keep = []
        self.ws = nat.Workspace()
        self._bufs = {}
        self.oid = ops.register(self)  # torch.ops.flamed_hip.fac_decode / enc_encode

    def __del__(self):
        try:
            if self.handle is not None:
                nat.destroy(self.handle, "flamed_enc_destroy")
        except Exception:
            pass

    def _ensure_created(self):
        if self.handle is None:
            h = ctypes.c_void_p()
            ups = (ctypes.c_int * len(self.enc.up_ratios))(*self.enc.up_ratios)
            nat.check(nat.lib().flamed_enc_create(self.enc.ngf, len(self.enc.up_ratios), ups, self.enc.out_channels,
                                                  nat.dtype_code(self.dtype_name), ctypes.byref(h)), "flamed_enc_create")
            self.handle = h
            nat.track(h, "flamed_enc_destroy")

    def _ensure(self, dev):
        params = enc_weight_list(self.enc)
        sig = tuple((p.data_ptr(), nat.tensor_version(p)) for p in params) + (str(dev),)
        if sig == self._sig:
            return
        L = nat.lib()
        self._ensure_created()
        keep = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
        arr = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        nat.check(L.flamed_enc_load(self.handle, arr, len(keep), nat.stream_ptr(dev)), "flamed_enc_load")
        self._keep = keep
        self._sig = sig
        self._bufs = {}

    def out_len(self, n: int) -> int:
        """Frames the encoder produces from n samples (the strided conv chain; needs the handle)."""
        self._ensure_created()
        return int(nat.lib().flamed_enc_out_len(self.handle, n))

    def encode(self, x, lens=None):
        """lens: None, or B sample counts (flamed_enc_encode_lens: each utterance over its own samples, 0 behind it)."""
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"FACodecEncoder expects (B, 1, n) audio, got {tuple(x.shape)}")
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
        dev = x.device
        self._ensure(dev)
        B, _, n = x.shape
        L = nat.lib()
        T = L.flamed_enc_out_len(self.handle, n)
        if T <= 0:
            raise ValueError(f"audio of {n} samples is too short for the encoder")
        key = (B, n)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = {"x": torch.empty((B, n), dtype=torch.float32, device=dev),
                    "out": torch.empty((B, self.enc.out_channels, T), dtype=torch.float32, device=dev)}
            self._bufs = {key: bufs}
        bufs["x"].copy_(x.reshape(B, n))
        ws = self.ws.get(L.flamed_enc_workspace_size(self.handle, B, n), dev)
        if lens is not None:
            nat.check(L.flamed_enc_encode_lens(self.handle, nat.ptr(bufs["x"]), B, n, (ctypes.c_int * B)(*lens),
                                               nat.ptr(bufs["out"]), nat.ptr(ws), ws.numel(), int(bool(self.enc.hip_graph)),
                                               nat.stream_ptr(dev)), "flamed_enc_encode_lens")
            return bufs["out"].clone()
        nat.check(L.flamed_enc_encode(self.handle, nat.ptr(bufs["x"]), B, n, nat.ptr(bufs["out"]), nat.ptr(ws), ws.numel(),
                                      int(bool(self.enc.hip_graph)), nat.stream_ptr(dev)), "flamed_enc_encode")
        return bufs["out"].clone()


def vq_weight_list(dec: FACodecDecoder) -> List[torch.Tensor]:
    """Weights in the order flamed_vq_load expects (include/flamed_hip.h)."""
    w = []
    for rvq in dec.quantizer:
        for ly in rvq.layers:
            w += [ly.in_proj.weight_g, ly.in_proj.weight_v, ly.in_proj.bias, ly.out_proj.weight_g,
                  ly.out_proj.weight_v, ly.out_proj.bias, ly._codebook.weight]
    te = dec.timbre_encoder
    w.append(te.position_emb.pe)
    for ly in te.layers:
        a = ly.self_attn
        w += [ly.ln_1.weight, ly.ln_1.bias, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
              ly.ln_2.weight, ly.ln_2.bias, ly.ffn.ffn_1.weight, ly.ffn.ffn_1.bias, ly.ffn.ffn_2.weight,
              ly.ffn.ffn_2.bias]
    return w + [te.last_ln.weight, te.last_ln.bias]


class VqHIP:
    """Owns one flamed_vq_t handle: the prompt-side quantizers + timbre encoder of a FACodecDecoder
    (FACodecDecoder.forward(vq=True), reference facodec.py:470-533)."""

    def __init__(self, dec: FACodecDecoder):
        self.dec = dec
        self.handle = None
        self._sig = None
        self.ws = nat.Workspace()
        self._bufs = {}
        self.oid = ops.register(self)  # torch.ops.flamed_hip.vq_encode

    def __del__(self):
        try:
            if self.handle is not None:
                nat.destroy(self.handle, "flamed_vq_destroy")
        except Exception:
            pass

    def dims(self) -> List[int]:
        return VqHIP.dims_of(self.dec)

    @staticmethod
    def dims_of(d) -> List[int]:
        te = d.timbre_encoder
        nl = [len(q.layers) for q in d.quantizer]
        ks = [q.layers[0]._codebook.weight.shape[0] for q in d.quantizer]
        fvq = d.quantizer[0].layers[0]
        return [fvq.in_proj.weight_v.shape[1], fvq.codebook_dim, len(nl), *nl, *ks, te.encoder_hidden, te.encoder_head, te.conv_filter_size,
                te.conv_kernel_size, len(te.layers), te.position_emb.pe.shape[0]]

    def _ensure(self, dev):
        params = vq_weight_list(self.dec)
        sig = tuple((p.data_ptr(), nat.tensor_version(p)) for p in params) + (str(dev),)
        if sig == self._sig and self.handle is not None:
            return
        L = nat.lib()
        if self.handle is None:
            h = ctypes.c_void_p()
            d = self.dims()
            nat.check(L.flamed_vq_create((ctypes.c_int * len(d))(*d), len(d), ctypes.byref(h)), "flamed_vq_create")
            self.handle = h
            nat.track(h, "flamed_vq_destroy")
        keep = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
        arr = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        nat.check(L.flamed_vq_load(self.handle, arr, len(keep), nat.stream_ptr(dev)), "flamed_vq_load")
        torch.cuda.current_stream(dev).synchronize()  # the arena copies read `keep`
        self._sig = sig
        self._bufs = {}

    def encode(self, x: torch.Tensor, lens=None, pad_code: int = 0):
        """x (B, C, T) encoder output -> (outs (B, C, T), codes (n_q, B, T) int64, per-group quantized sums
        (G, B, C, T), speaker embedding (B, C)).  lens: None, or B frame counts in 1..T (flamed_vq_encode_lens: each
        utterance over its own frames with position row pe[0]; 0 / pad_code behind its end)."""
        if lens is not None:
            lens = check_lens(lens, x.shape[0], x.shape[2])
        dev = x.device
        self._ensure(dev)
        B, C, T = x.shape
        G = len(self.dec.quantizer)
        nq = sum(len(q.layers) for q in self.dec.quantizer)
        key = (B, C, T)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = {"x": torch.empty((B, C, T), dtype=torch.float32, device=dev),
                    "outs": torch.empty((B, C, T), dtype=torch.float32, device=dev),
                    "codes": torch.empty((nq, B, T), dtype=torch.int64, device=dev),
                    "qbuf": torch.empty((G, B, C, T), dtype=torch.float32, device=dev),
                    "spk": torch.empty((B, C), dtype=torch.float32, device=dev)}
            self._bufs = {key: bufs}
        bufs["x"].copy_(x)
        L = nat.lib()
        ws = self.ws.get(L.flamed_vq_workspace_size(self.handle, B, T), dev)
        if lens is not None:
            nat.check(L.flamed_vq_encode_lens(self.handle, nat.ptr(bufs["x"]), B, T, (ctypes.c_int * B)(*lens),
                                              ctypes.c_int64(int(pad_code)), nat.ptr(bufs["outs"]), nat.ptr(bufs["codes"]),
                                              nat.ptr(bufs["qbuf"]), nat.ptr(bufs["spk"]), nat.ptr(ws), ws.numel(),
                                              int(bool(self.dec.hip_graph)), nat.stream_ptr(dev)), "flamed_vq_encode_lens")
            return tuple(bufs[k].clone() for k in ("outs", "codes", "qbuf", "spk"))
        nat.check(L.flamed_vq_encode(self.handle, nat.ptr(bufs["x"]), B, T, nat.ptr(bufs["outs"]), nat.ptr(bufs["codes"]),
                                     nat.ptr(bufs["qbuf"]), nat.ptr(bufs["spk"]), nat.ptr(ws), ws.numel(),
                                     int(bool(self.dec.hip_graph)), nat.stream_ptr(dev)), "flamed_vq_encode")
        return tuple(bufs[k].clone() for k in ("outs", "codes", "qbuf", "spk"))
