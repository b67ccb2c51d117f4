"""Keyed noise: counter-based normals keyed per utterance (DESIGN.md "Keyed noise").

The reference draws `torch.randn((B, T, C))` from the global CPU RNG, so an utterance's noise depends on its place in
the batch, on the padded length and on the batch size.  Here utterance u's element e = t * C + c is lane e % 4 of
Philox4x32-10 with key = (low, high 32 bits of its 64-bit seed) and counter = (e // 4 low, e // 4 high, stream id, 0),
turned into a standard normal by Box-Muller on the word pairs (w0, w1) and (w2, w3).  Nothing in e involves B, the
padded T or the batch position: a batch row equals the call made for that utterance alone, and a shorter length is a
prefix of a longer one, bit for bit within a back end.

Two back ends follow the one definition: the HIP kernel (flamed_noise_state, csrc/noise.hip; CUDA / ROCm tensors) and
numpy (`keyed_normal`; CPU tensors).  They agree to 1e-5 in the normals (their log / sincos differ in the last bits),
not bitwise.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from flamed import _native as nat

_M64 = (1 << 64) - 1
STREAM_LATENT, STREAM_DURATION, STREAM_SILENCE = 0, 1, 2


def utterance_seed(seed: int, index: int) -> int:
    """The 64-bit seed of utterance `index` under the run's `seed`: the splitmix64 finaliser of
    seed + 0x9E3779B97F4A7C15 * (index + 1), in 64-bit wrap-around arithmetic."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(index) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def utterance_seeds(seed: int, indices: Sequence[int]) -> List[int]:
    return [utterance_seed(seed, i) for i in indices]


def _check(seeds, lens, B: int, T: int, C: int, stream_id: int):
    seeds = [int(s) for s in seeds]
    if B < 1 or T < 1 or C < 1:
        raise ValueError(f"keyed noise: B, T, C must be >= 1 (got {B}, {T}, {C})")
    if len(seeds) != B or any(s < 0 or s > _M64 for s in seeds):
        raise ValueError(f"keyed noise: need {B} seeds in [0, 2^64) (got {len(seeds)})")
    if stream_id < 0 or stream_id >= 1 << 32:
        raise ValueError(f"keyed noise: stream_id must be in [0, 2^32) (got {stream_id})")
    if lens is not None:
        lens = [int(n) for n in lens]
        if len(lens) != B or any(n < 1 or n > T for n in lens):
            raise ValueError(f"keyed noise: need {B} lengths in 1..{T} (got {lens})")
    return seeds, lens


def philox4x32_10(block: np.ndarray, stream_id: int, seed: int) -> np.ndarray:
    """Philox4x32-10 words (n, 4) uint32 of the uint64 block indices `block` under one key and stream."""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    block = np.asarray(block, dtype=np.uint64)
    c0, c1 = block & m32, block >> s32
    c2 = np.full_like(block, np.uint64(stream_id))
    c3 = np.zeros_like(block)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack((c0, c1, c2, c3), axis=1).astype(np.uint32)


_VEC_BLOCKS = 16  # blocks are generated in multiples of 16, so numpy's vector loops never end in a scalar tail


def _normals(seed: int, n: int, stream_id: int) -> np.ndarray:
    """The first n normals (fp32) of one utterance's stream."""
    nblk = -(-n // 4)
    nblk = -(-nblk // _VEC_BLOCKS) * _VEC_BLOCKS
    w = philox4x32_10(np.arange(nblk, dtype=np.uint64), stream_id, seed)
    two24 = np.float32(2.0 ** -24)
    wa, wb = w[:, 0::2], w[:, 1::2]  # (nblk, 2): the pairs (w0, w1) and (w2, w3)
    u = ((wa >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * two24
    th = np.float32(2.0 * np.pi) * ((wb >> np.uint32(8)).astype(np.float32) * two24)
    r = np.sqrt(np.float32(-2.0) * np.log(u))
    out = np.empty((nblk, 4), dtype=np.float32)
    out[:, 0::2] = r * np.cos(th)
    out[:, 1::2] = r * np.sin(th)
    return out.reshape(-1)[:n]


def keyed_normal(seeds, lens, T: int, C: int, stream_id: int, device=None) -> torch.Tensor:
    """The CPU back end: (B, T, C) fp32 standard normals, utterance u keyed by seeds[u], exactly 0 behind lens[u]
    (lens None: T for all)."""
    B = len(seeds)
    seeds, lens = _check(seeds, lens, B, int(T), int(C), int(stream_id))
    out = np.zeros((B, T * C), dtype=np.float32)
    for u, s in enumerate(seeds):
        n = (T if lens is None else lens[u]) * C
        out[u, :n] = _normals(s, n, stream_id)
    t = torch.from_numpy(out).reshape(B, T, C)
    return t if device is None else t.to(device)


def hip_noise_state(cond: Optional[torch.Tensor], seeds, lens, temperature: float, stream_id: int, shape=None, device=None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flamed_noise_state on the current stream of the tensors' device.  cond: fp32 (B, T, C) or None (then `shape` and
    `device` say what to make); out: where to write (may be cond itself), a new tensor by default."""
    if cond is not None:
        if cond.dtype != torch.float32 or not cond.is_contiguous() or cond.dim() != 3:
            raise ValueError("noise_state: cond must be a contiguous fp32 (B, T, C) tensor")
        shape, device = tuple(cond.shape), cond.device
    B, T, C = (int(v) for v in shape)
    seeds, lens = _check(seeds, lens, B, T, C, int(stream_id))
    device = torch.device(device)
    if out is None:
        out = torch.empty((B, T, C), dtype=torch.float32, device=device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, T, C) or out.device != device:
        raise ValueError("noise_state: out must be a contiguous fp32 (B, T, C) tensor on cond's device")
    sa = (ctypes.c_ulonglong * B)(*seeds)
    la = (ctypes.c_int * B)(*lens) if lens is not None else None
    with torch.cuda.device(device):
        nat.check(nat.lib().flamed_noise_state(nat.ptr(cond), sa, la, int(stream_id), float(temperature), B, T, C,
                                               nat.ptr(out), nat.stream_ptr(device)), "flamed_noise_state")
    return out


def _signed(s: int) -> int:
    return s - (1 << 64) if s >= 1 << 63 else s


def noise_state(cond: Optional[torch.Tensor], seeds, lens, temperature: float, stream_id: int, shape=None,
                device=None) -> torch.Tensor:
    """x = cond + temperature * n with n the keyed normals of seeds (B ints in [0, 2^64)), 0 behind lens[u] (lens None:
    no padding).  cond None: x = temperature * n of `shape` (B, T, C) on `device`.  CUDA / ROCm: the HIP kernel
    (torch.ops.flamed_hip.noise_state; fp32); CPU: keyed_normal.  The global RNGs are not touched."""
    if cond is not None:
        shape, device = tuple(cond.shape), cond.device
    device = torch.device("cpu" if device is None else device)
    B, T, C = (int(v) for v in shape)
    seeds, lens = _check(seeds, lens, B, T, C, int(stream_id))
    if device.type == "cuda":
        from flamed import ops
        c = None if cond is None else cond.float().contiguous()
        return ops.noise_state(c, [_signed(s) for s in seeds], lens, float(temperature), int(stream_id), B, T, C, device)
    n = keyed_normal(seeds, lens, T, C, stream_id)
    if cond is None:
        return n * temperature
    x = cond + n.to(cond.dtype) * temperature
    if lens is not None:
        for u, m in enumerate(lens):
            x[u, m:] = 0
    return x
