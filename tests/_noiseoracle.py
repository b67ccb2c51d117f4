"""Keyed noise: the test oracle, written from the definition (DESIGN.md "Keyed noise") and independent of
flamed/utils/noise.py -- a scalar-free numpy Philox4x32-10 on uint64 lanes plus an fp64 Box-Muller.  Shared by
tests/test_noise_cpu.py and tests/test_noise_gpu.py.

  utterance seed  z = seed + 0x9E3779B97F4A7C15 (index + 1); z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
                  z = (z ^ z >> 27) 0x94D049BB133111EB; z ^= z >> 31           (mod 2^64)
  element e       lane e % 4 of Philox4x32-10(counter = (e // 4 low, e // 4 high, stream, 0), key = (seed low, seed high))
  normals         u = ((w_a >> 8) + 1) 2^-24, theta = 2 pi (w_b >> 8) 2^-24, r = sqrt(-2 ln u);
                  lanes (0, 1) = (r cos, r sin) of (w0, w1), lanes (2, 3) of (w2, w3)
  state           x = cond + temperature n, 0 behind the utterance's length
"""
import numpy as np

M64 = (1 << 64) - 1
KNOWN = [  # (counter, key, output): the issue's known answers (the first and third are Random123's)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def utterance_seed(seed, index):
    z = (seed + 0x9E3779B97F4A7C15 * (index + 1)) % 2**64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2**64
    return z ^ (z >> 31)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counter word arrays (uint64 holding 32-bit values) under key (k0, k1) -> (n, 4) uint32."""
    lo = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in (c0, c1, c2, c3)]
    n = max(len(v) for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    for r in range(10):
        ka, kb = np.uint64((k0 + r * 0x9E3779B9) % 2**32), np.uint64((k1 + r * 0xBB67AE85) % 2**32)
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ ka, p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ kb, p0 & lo]
    return np.stack(c, axis=1).astype(np.uint32)


def words(seed, stream, first, n):
    """The raw word of elements first .. first + n - 1 (first may exceed 2^34)."""
    e = [first + i for i in range(n)]
    blk = [v // 4 for v in e]
    w = philox([b % 2**32 for b in blk], [b >> 32 for b in blk], stream, 0, seed % 2**32, seed >> 32)
    return w[np.arange(n), np.array([v % 4 for v in e])]


def block_words(seed, stream, nblk):
    blk = np.arange(nblk, dtype=np.uint64)
    return philox(blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), stream, 0, seed % 2**32, seed >> 32)


def normals(seed, stream, n):
    """The first n normals of one utterance's stream, fp64."""
    w = block_words(seed, stream, -(-n // 4)).astype(np.float64)
    out = np.empty_like(w)
    for a in (0, 2):
        u = (np.floor(w[:, a] / 256) + 1) * 2.0 ** -24
        th = 2 * np.pi * (np.floor(w[:, a + 1] / 256) * 2.0 ** -24)
        r = np.sqrt(-2 * np.log(u))
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return out.reshape(-1)[:n]


def state(cond, seeds, lens, temperature, stream, shape=None):
    """fp64 (B, T, C): cond + temperature n, 0 behind lens[u] (lens None: no padding; cond None: zeros of `shape`)."""
    B, T, C = shape if cond is None else cond.shape
    x = np.zeros((B, T, C))
    for u in range(B):
        n = (T if lens is None else lens[u]) * C
        v = temperature * normals(seeds[u], stream, n)
        if cond is not None:
            v = v + np.asarray(cond[u], dtype=np.float64).reshape(-1)[:n]
        x[u].reshape(-1)[:n] = v
    return x
