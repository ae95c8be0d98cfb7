"""CPU restatement of the device turbulence (bluesky_amd/csrc/bsa_turb_math.h):
Philox4x64-10 in Python-int arithmetic, the uniform and Box-Muller formulas,
and Turbulence.Woosh's application (turbulence.py:38-46) in numpy's order."""
import numpy as np

M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
PHILOX_W0, PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
REARTH = 6371000.


def philox4x64_10(counter, key):
    """One block: ``counter`` four and ``key`` two 64-bit words (least significant first)."""
    c0, c1, c2, c3 = [int(x) & M64 for x in counter]
    k0, k1 = [int(x) & M64 for x in key]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & M64, (p0 >> 64) ^ c3 ^ k1, p0 & M64
        k0, k1 = (k0 + PHILOX_W0) & M64, (k1 + PHILOX_W1) & M64
    return c0, c1, c2, c3


def numpy_counter(counter):
    """The counter whose block ``np.random.Philox(counter=counter, key=...)`` outputs first:
    numpy advances the 256-bit counter by one before it generates."""
    v = sum((int(x) & M64) << (64 * q) for q, x in enumerate(counter))
    v = (v + 1) & ((1 << 256) - 1)
    return [(v >> (64 * q)) & M64 for q in range(4)]


def raw_words(n, seed=0, call=0, first_index=0):
    """(n, 4) uint64: the block of counter {index, call, 0, 0}, key {seed, 0} per index."""
    out = np.empty((n, 4), dtype=np.uint64)
    for i in range(n):
        out[i] = philox4x64_10((first_index + i, call, 0, 0), (seed, 0))
    return out


def uniforms(words):
    return ((words >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals(words):
    """(n, 3) unit normals of (n, 4) words: z0 / z1 the cosine / sine branch of (u0, u1),
    z2 the cosine branch of (u2, u3)."""
    u = uniforms(words)
    r0 = np.sqrt(-2.0 * np.log(u[:, 0]))
    r1 = np.sqrt(-2.0 * np.log(u[:, 2]))
    a0 = (2.0 * np.pi) * u[:, 1]
    a1 = (2.0 * np.pi) * u[:, 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=1)


def draws(n, seed=0, call=0, first_index=0):
    return normals(raw_words(n, seed, call, first_index))


def clamp_sd(sd):
    sd = np.array(sd, dtype=np.float64)
    return np.where(sd > 1e-6, sd, 1e-6)   # turbulence.py:22


def woosh_apply(z, dt, sd, trk, coslat, lat, lon, alt):
    """turbulence.py:28-46 with the unit normals ``z`` (n, 3) in place of numpy's stream:
    np.random.normal(0, scale, n) is 0 + scale * gauss.  Returns the new (lat, lon, alt)."""
    sd = clamp_sd(sd)
    timescale = np.sqrt(dt)
    turbhf = (sd[0] * timescale) * z[:, 0]
    turbhw = (sd[1] * timescale) * z[:, 1]
    turbalt = (sd[2] * timescale) * z[:, 2]
    trkrad = np.radians(trk)
    turblat = np.cos(trkrad) * turbhf - np.sin(trkrad) * turbhw
    turblon = np.sin(trkrad) * turbhf + np.cos(trkrad) * turbhw
    return (lat + np.degrees(turblat / REARTH), lon + np.degrees(turblon / REARTH / coslat), alt + turbalt)
