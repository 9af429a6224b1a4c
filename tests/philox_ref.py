"""numpy restatement of the training forward's random stream (include/decafnet_hip.h, dcf_model_set_dropout).

Philox4x32-10 keyed by the two halves of a 64-bit seed; element e of a site takes word e & 3 of counter block
(j & 0xffffffff, j >> 32, site, 0), j = e >> 2; u = (word >> 8) * 2^-24; kept iff u >= p (p as fp32).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

G_FUSION, G_STEM, G_BRANCH, G_REFINE = 1, 2, 3, 4
PROJ, FFN_HID, FFN_OUT, PATH_ATTN, PATH_FFN, TCN = 0, 1, 2, 3, 4, 5


def site(group, layer, sub):
    return group << 16 | layer << 4 | sub


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32-valued array, key: (k0, k1) ints -> (..., 4) uint32 array"""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
    return np.stack(c, -1).astype(np.uint32)


def words(seed, site_, e):
    """the Philox word of every element index in e (int array)"""
    seed = int(seed) & ((1 << 64) - 1)
    e = np.asarray(e, dtype=np.uint64)
    j = e >> np.uint64(2)
    ctr = np.stack([j & MASK32, j >> np.uint64(32), np.full_like(j, site_), np.zeros_like(j)], -1)
    out = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return np.take_along_axis(out, (e & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]


def keep(seed, site_, e, p):
    """keep bits (bool array, shape of e)"""
    u = (words(seed, site_, e) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_mask(seed, site_, shape, p):
    """keep bits of a whole (B', C, T) tensor of the reference, e = (b * C + c) * T + t"""
    return keep(seed, site_, np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape), p)


def drop_path_keep(seed, site_, n, p):
    """per-sample keep bits of drop-path (e = b)"""
    return keep(seed, site_, np.arange(n, dtype=np.uint64), p)
