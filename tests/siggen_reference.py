"""The signal generator's model in numpy float64 (tests/test_siggen_reference.py, tests/test_siggen_gpu.py, tests/golden/make_golden_siggen.py):

    out[n] = sum_sat (sA[p mod len_a] A[n mod period] + sB[p mod len_b] B[n mod period]) exp(+j (theta0 + 2 pi f n / fs)) + noise[n]
    p = (n + period - delay_samples) // period,    f = doppler_hz + carrier_offset_hz

with n the absolute sample index, in exact integer arithmetic: the carrier's revolutions at the first sample are reduced modulo one as a
Fraction of the doubles f and fs, so the model holds at 2^40 as it does at 0.  The noise is the published Philox4x32-10 round function restated
on numpy integers (counter = (n low, n high, 0, 0), key = (seed low, seed high)) and Box-Muller in float64 on words 0 and 1, as
gnss-sdr_amd/csrc/signal_generator.hip draws them.  A satellite is anything with the attributes of gnss_sdr_amd.signal_generator.Satellite."""
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64; -> four uint32 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def noise_words(seed: int, n0: int, n: int):
    idx = np.uint64(n0) + np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    return philox4x32_10(idx & MASK, idx >> np.uint64(32), z, z, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def noise(seed: int, n0: int, n: int) -> np.ndarray:
    """complex128 noise of samples [n0, n0 + n): u = ((w0 >> 9) + 0.5) 2^-23, r = sqrt(-2 ln u), angle = pi (int32) w1 2^-31"""
    w0, w1, _w2, _w3 = noise_words(seed, n0, n)
    u = ((w0 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u))
    ang = np.pi * w1.view(np.int32).astype(np.float64) * 2.0 ** -31
    return r * (np.cos(ang) + 1j * np.sin(ang))


def amplitude(sat) -> float:
    """the largest |A[m]| + |B[m]| of the satellite: what one of its samples can reach"""
    a = np.abs(np.asarray(sat.table_a, np.complex128))
    if sat.table_b is not None:
        a = a + np.abs(np.asarray(sat.table_b, np.complex128))
    return float(a.max())


def amplitude_sum(sats) -> float:
    return float(sum(amplitude(s) for s in sats))


def satellite_term(sat, fs: float, n0: int, n: int) -> np.ndarray:
    idx = np.uint64(n0) + np.arange(n, dtype=np.uint64)    # absolute indices (below 2^63)
    A = np.asarray(sat.table_a, np.complex128).reshape(-1)
    period = A.size
    sA = np.asarray(sat.signs_a, np.float64).reshape(-1)
    m = (idx % np.uint64(period)).astype(np.int64)
    p = (idx + np.uint64(period - int(sat.delay_samples))) // np.uint64(period)
    base = sA[(p % np.uint64(sA.size)).astype(np.int64)] * A[m]
    if sat.table_b is not None:
        B = np.asarray(sat.table_b, np.complex128).reshape(-1)
        sB = np.asarray(sat.signs_b, np.float64).reshape(-1)
        base = base + sB[(p % np.uint64(sB.size)).astype(np.int64)] * B[m]
    f = float(sat.doppler_hz) + float(sat.carrier_offset_hz)
    rev0 = Fraction(f) * int(n0) / Fraction(float(fs))
    rev0 = float(rev0 - (rev0.numerator // rev0.denominator))
    phase = float(sat.start_phase_rad) + 2.0 * np.pi * (rev0 + (f / float(fs)) * np.arange(n, dtype=np.float64))
    return base * np.exp(1j * phase)


def model(sats, fs: float, n0: int, n: int, noise_seed=None) -> np.ndarray:
    """complex128 samples [n0, n0 + n); noise_seed None: no noise"""
    out = np.zeros(n, np.complex128)
    for sat in sats:
        out += satellite_term(sat, fs, n0, n)
    if noise_seed is not None:
        out += noise(noise_seed, n0, n)
    return out
