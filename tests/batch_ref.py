"""numpy restatement of the training set's device generator (pnrf_train_batch_fwd, include/pronerf_hip.h): Philox4x32-10 in uint64 arithmetic,
the word -> uniform map, Box-Muller in float64, and the rule that ties a quad of four columns to its counter.  Nothing here calls the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_JITTER, STREAM_NOISE = 0, 1
CAP_STAGE2, CAP_STAGE1 = 1 - 2e-6, 0.99


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> uint32 array [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, -1).astype(np.uint32)


def unit(x):
    """u = (2 (x >> 9) + 1) 2^-24 of a uint32 word, float64 (the value is exact in fp32 too)."""
    return (2.0 * (np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def words(n, C, seed=0, step=0, stream=0, row0=0):
    """The uint32 words [n, C] behind an [n, C] array: quad q = (row0 + row) (C / 4) + k uses counter (q low, q high, step, stream)."""
    assert C % 4 == 0 and C > 0
    q = (np.uint64(row0) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(C // 4) + np.arange(C // 4, dtype=np.uint64)[None, :]
    seed = int(seed)
    w = philox4x32_10((q & MASK, q >> np.uint64(32), np.uint64(step), np.uint64(stream)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return w.reshape(n, C)


def normals(n, C, seed=0, step=0, stream=0, row0=0):
    """float64 N(0,1) values [n, C]: words (0, 1) and (2, 3) of every quad give (r cos(2 pi u1), r sin(2 pi u1)), r = sqrt(-2 log u0)."""
    u = unit(words(n, C, seed, step, stream, row0)).reshape(n, C // 2, 2)
    r = np.sqrt(-2.0 * np.log(u[..., 0]))
    a = 2.0 * np.pi * u[..., 1]
    return np.stack([r * np.cos(a), r * np.sin(a)], -1).reshape(n, C)


def jitter(n, C, cap, seed=0, step=0, row0=0):
    return np.minimum(np.abs(normals(n, C, seed, step, STREAM_JITTER, row0)) / 5.0, cap)


def noise(n, C, std, seed=0, step=0, row0=0):
    return normals(n, C, seed, step, STREAM_NOISE, row0) * std
