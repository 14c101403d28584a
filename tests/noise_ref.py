"""numpy restatement of mkd_noise_fill (include/mkd.h): Philox4x32-10 in integer arithmetic, the open-interval uniform and the Box-Muller
normals in float64.  The angle 2 pi u is folded EXACTLY before it is multiplied by pi: u = m / 2^25 with m odd, so the turn is an
integer count of 2^-25 turns, its octant and its distance to the nearer octant boundary are integers, and sin / cos are only ever
evaluated in (0, pi / 4).  The restatement therefore stays accurate RELATIVE to the small values near the zeros of sin and cos, which is
what a bound in ulps of the result needs."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
Z_MAX = float(np.sqrt(50.0 * np.log(2.0)))          # |z| <= sqrt(-2 ln(2^-25)) = sqrt(50 ln 2)

STREAM_START, STREAM_ETA, STREAM_BLEND, STREAM_POSTERIOR = 0, 1, 2, 3


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (anything numpy takes as unsigned 32-bit values) -> uint32 [..., 4]: ten rounds, the key advanced by the
    Weyl constants between them"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def unit(w):
    """u(w) = ((w >> 8) + 0.5) 2^-24 in float64 (exact)"""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def cos_sin_turn(w):
    """(cospi(2 u(w)), sinpi(2 u(w))) in float64 with the angle folded exactly: m = 2 (w >> 8) + 1 counts 2^-25 turns"""
    m = ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.int64) << 1) + 1          # odd, 1 .. 2^25 - 1
    octant = m >> 22
    r = m - (octant << 22)                                     # 1 .. 2^22 - 1 (odd: never on a boundary)
    near = np.where(octant & 1, (1 << 22) - r, r)              # distance to the octant boundary that is a multiple of a quarter turn
    phi = near.astype(np.float64) * (2.0 * np.pi / 2.0 ** 25)  # in (0, pi / 4)
    c, s = np.cos(phi), np.sin(phi)
    cos = np.select([octant == 0, octant == 1, octant == 2, octant == 3, octant == 4, octant == 5, octant == 6, octant == 7],
                    [c, s, -s, -c, -c, -s, s, c])
    sin = np.select([octant == 0, octant == 1, octant == 2, octant == 3, octant == 4, octant == 5, octant == 6, octant == 7],
                    [s, c, c, s, -s, -c, -c, -s])
    return cos, sin


def normals_from_words(q):
    """uint32 [..., 4] -> float64 [..., 4]: (rho_a cos_a, rho_a sin_a, rho_b cos_b, rho_b sin_b), rho = sqrt(-2 ln u), pairs (r0, r1), (r2, r3)"""
    q = np.asarray(q)
    out = np.empty(q.shape, dtype=np.float64)
    for a in (0, 2):
        rho = np.sqrt(-2.0 * np.log(unit(q[..., a])))
        c, s = cos_sin_turn(q[..., a + 1])
        out[..., a], out[..., a + 1] = rho * c, rho * s
    return out


def blocks(seed, sub, stream, row, n):
    """the words of ceil(n / 4) blocks of one (seed, sub, stream, row): uint32 [nblk, 4]"""
    nblk = (int(n) + 3) // 4
    ctr = np.empty((nblk, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nblk, dtype=np.uint64)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = int(row) & MASK, int(stream) & MASK, int(sub) & MASK
    key = np.empty((nblk, 2), dtype=np.uint64)
    key[:, 0], key[:, 1] = int(seed) & MASK, (int(seed) >> 32) & MASK
    return philox4x32_10(ctr, key)


def fill(seeds, subs, stream, row0, rows, n, kind=0):
    """mkd_noise_fill's output [rows][batch][n]: kind 0 float64 normals (round to fp32 ONCE to compare), kind 1 the uint32 words"""
    B = len(seeds)
    out = np.empty((rows, B, n), dtype=np.float64 if kind == 0 else np.uint32)
    for i in range(rows):
        for b in range(B):
            q = blocks(seeds[b], 0 if subs is None else subs[b], stream, row0 + i, n)
            v = normals_from_words(q) if kind == 0 else q
            out[i, b] = v.reshape(-1)[:n]
    return out


def moments(z):
    """(mean, variance, kurtosis) of a sample, in float64"""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    m = z.mean()
    d = z - m
    v = (d ** 2).mean()
    return float(m), float(v), float((d ** 4).mean() / v ** 2)


def moment_bounds(N):
    """five standard errors of the three moments of N independent standard normals: (|mean|, |var - 1|, |kurtosis - 3|)"""
    return 5.0 / np.sqrt(N), 5.0 * np.sqrt(2.0 / N), 5.0 * np.sqrt(24.0 / N)


MOMENT_SEED = 20241          # the moments tests' seed, host and device: the reference itself lies inside the bounds (test_noise_host.py)
MOMENT_N = 1 << 20


def ulp_distance(a, b):
    """element-wise distance of two float32 arrays in units in the last place (0: the same bits; +0 and -0 count as equal)"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))
