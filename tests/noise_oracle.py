"""NumPy float64 restatement of the seeded-noise contract of include/flowdec_hip.h ("Seeded noise").

For a clip with 64-bit seed s, draw index d, frequency row f and frame t: Philox4x32-10 (Random123) with key (s & 0xffffffff,
s >> 32) and counter (t >> 1, f, d, 0) gives r0..r3; an even t takes (ra, rb) = (r0, r1), an odd t (r2, r3);
u1 = ((ra >> 9) + 0.5) 2^-23, u2 = (rb >> 8) 2^-24; z = sqrt(-ln u1) (cos 2 pi u2 + i sin 2 pi u2).
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints) and two scalar key words -> the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> SH32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> SH32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def noise_bits(seed, draw, F, T):
    """-> (ra, rb): uint32 [F, T], the two words of every element of the plane (seed, draw)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    f, tp = np.meshgrid(np.arange(F, dtype=np.uint64), np.arange((T + 1) // 2, dtype=np.uint64), indexing="ij")
    r = philox4x32_10(tp, f, np.full_like(f, draw), np.zeros_like(f), seed & 0xFFFFFFFF, seed >> 32)
    ra = np.stack([r[0], r[2]], -1).reshape(F, -1)[:, :T]
    rb = np.stack([r[1], r[3]], -1).reshape(F, -1)[:, :T]
    return ra, rb


def gaussian_from_bits(ra, rb):
    """The contract's Box-Muller in float64 -> complex128."""
    u1 = ((ra >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (rb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    rad, th = np.sqrt(-np.log(u1)), 2 * np.pi * u2
    return rad * np.cos(th) + 1j * rad * np.sin(th)


def noise_plane(seed, draw, F, T):
    """complex128 [F, T]: z(seed, draw, f, t)."""
    return gaussian_from_bits(*noise_bits(seed, draw, F, T))
