"""numpy Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the generator
of vl_fbank_augment's noise field: key = the sample's 64-bit seed, counter = (element index / 4, 0), word = index % 4."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def noise_field(seed, T, F):
    """u [T, F] float32 in [0, 1): (bits >> 8) 2^-24."""
    groups = (T * F + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    z = np.zeros(groups, dtype=np.uint64)
    words = np.stack(philox4x32_10(g & M32, g >> np.uint64(32), z, z, seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)[:T * F]
    return ((words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(T, F)
