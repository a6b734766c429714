"""Host reference (numpy) of the random draws at the head of a training step, written from the generator's specification and
not from the kernels (csrc/evae_loss.hip: batch_prologue_kernel, batch_prologue_u8_body).

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a 4 x 32-bit counter, a
2 x 32-bit key, ten rounds.  One round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0));
the key is bumped by the two Weyl constants between rounds.

The step's two streams (element e of a flattened, dense [B x D] or [B x zdim] array takes word e % 4 of quad e // 4):
    image:  counter (t_lo, t_hi, step_lo, (step_hi << 1) & 0xffffffff),        key (seed_lo, seed_hi)
    eps:    counter (q_lo, q_hi, step_lo, ((step_hi << 1) & 0xffffffff) | 1),  key (seed_lo, seed_hi)
so bit 0 of the fourth counter word is the stream and no (quad, step) pair of one stream meets one of the other."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_IMAGE, STREAM_EPS = 0, 1


def _u64(a):
    return np.asarray(a, dtype=np.uint64) & MASK


def philox4x32(counter, key, rounds=10, multipliers=(M0, M1)):
    """counter: four uint32 arrays (broadcast against each other), key: two -> the four output words as uint64 arrays that hold
    32-bit values.  `rounds` and `multipliers` exist so that a test can show that a wrong generator misses the known answers."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) for c in counter])
    k0, k1 = _u64(key[0]), _u64(key[1])
    m0, m1 = np.uint64(multipliers[0]), np.uint64(multipliers[1])
    sh = np.uint64(32)
    for _ in range(rounds):
        p0 = m0 * c0                       # 32 x 32 -> 64 bits: exact in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & MASK, (p0 >> sh) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def philox4x32_10(counter, key):
    return philox4x32(counter, key, 10)


def stream_counter(quad, step, stream):
    """The counter of quad `quad` (array, < 2^64) of `stream` (0: image, 1: eps) at step `step` (< 2^63)."""
    quad = np.asarray(quad, dtype=np.uint64)
    step = int(step)
    step_lo, step_hi = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    return (quad & MASK, quad >> np.uint64(32), np.uint64(step_lo), np.uint64(((step_hi << 1) & 0xFFFFFFFF) | stream))


def seed_key(seed):
    seed = int(seed)
    return (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF))


def _words(n, seed, step, stream):
    """[ceil(n / 4) x 4] uint64 array: the stream's first quads, one per row."""
    nq = (int(n) + 3) // 4
    return np.stack(philox4x32_10(stream_counter(np.arange(nq, dtype=np.uint64), step, stream), seed_key(seed)), axis=1)


def u01(r):
    """[0, 1): the top 24 bits times 2^-24, an exact float32"""
    return (np.asarray(r, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def u01_open(r):
    """(0, 1]: (top 24 bits + 1) times 2^-24, an exact float32"""
    return ((np.asarray(r, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -24)


def image_uniforms(B, D, seed, step):
    """u [B x D] float32 of the image stream"""
    n = int(B) * int(D)
    return u01(_words(n, seed, step, STREAM_IMAGE).reshape(-1)[:n]).reshape(B, D)


def binarise(p, seed, step):
    """p [B x D] float32 probabilities (the gathered batch) -> 1.0 where u < p, compared in float32"""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2
    return (image_uniforms(p.shape[0], p.shape[1], seed, step) < p).astype(np.float32)


def eps_draws(B, zdim, seed, step):
    """eps [B x zdim] float64: Box-Muller on float32-rounded radicand and angle, the transcendentals in float64"""
    n = int(B) * int(zdim)
    w = _words(n, seed, step, STREAM_EPS)
    out = np.empty((w.shape[0], 4), np.float64)
    two_pi = np.float32(6.283185307179586)
    for pair in (0, 1):
        r = np.sqrt(-2.0 * np.log(u01_open(w[:, 2 * pair]).astype(np.float64)))
        a = (two_pi * u01(w[:, 2 * pair + 1])).astype(np.float32).astype(np.float64)
        out[:, 2 * pair] = r * np.cos(a)
        out[:, 2 * pair + 1] = r * np.sin(a)
    return out.reshape(-1)[:n].reshape(B, zdim)
