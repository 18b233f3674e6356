"""numpy float32 restatement of the reference's beamformer block (src/algorithms/input_filter/gnuradio_blocks/beamformer.cc) and of the item
handling in front of it, the checker of the gsh_beam_* calls (tests/test_beamformer_gpu.py).  tests/test_beamformer_reference.py pins it to the
block's own output (tests/golden/beamformer.npz, minted by tests/golden/make_golden_beamformer.py).

The block (beamformer.cc:53-61):

    gr_complex sum;
    for n: sum = gr_complex(0, 0);                                   // :56
           for i < weight_vector.size(): sum = sum + in[i][n] * weight_vector[i];   // :57-60
           out[n] = sum;                                             // :61

std::complex<float> multiplication of finite values is (a.re b.re - a.im b.im, a.re b.im + a.im b.re), every operation rounded to float32 once;
numpy's float32 array arithmetic does exactly that.  The sum starts from (0, 0), so a product of -0 comes out as +0."""
import numpy as np

F32 = np.float32
ITEM_DTYPES = {"gr_complex": np.float32, "ishort": np.int16, "ibyte": np.int8}


def items_to_complex(items, first_is_q=False, inverted_spectrum=False):
    """items [..., 2] (two values per item, of any of the item types) -> (re, im) float32 arrays: the integer -> float cast of the ring pushes
    (csrc/sample_convert.hip), (I, Q) per first_is_q, conjugated when inverted_spectrum"""
    v = np.asarray(items).astype(F32)
    re, im = (v[..., 1], v[..., 0]) if first_is_q else (v[..., 0], v[..., 1])
    return re.copy(), (-im if inverted_spectrum else im.copy())


def beamform(re, im, w, contracted=False):
    """re, im: float32 [A, n]; w: complex64 [B, A] (or [A]) -> complex64 [B, n], beamformer.cc:56-61 per beam.
    contracted: what a compiler that fuses multiply and add would make of the same lines (x.re w.re - x.im w.im as one fused operation on the
    rounded second product, likewise the imaginary part) -- NOT the block; the tests use it to show that they would notice."""
    re, im = np.asarray(re, F32), np.asarray(im, F32)
    w = np.asarray(w, np.complex64).reshape(-1, re.shape[0])
    out = np.empty((w.shape[0], re.shape[1]), np.complex64)
    for b in range(w.shape[0]):
        sr, si = np.zeros(re.shape[1], F32), np.zeros(re.shape[1], F32)          # :56
        for a in range(re.shape[0]):                                              # :57
            wr, wi = F32(w[b, a].real), F32(w[b, a].imag)
            if contracted:
                pr = (re[a].astype(np.float64) * np.float64(wr) - (im[a] * wi).astype(np.float64)).astype(F32)
                pi = (re[a].astype(np.float64) * np.float64(wi) + (im[a] * wr).astype(np.float64)).astype(F32)
            else:
                pr = re[a] * wr - im[a] * wi                                     # :59, operator* of std::complex<float>
                pi = re[a] * wi + im[a] * wr
            sr, si = sr + pr, si + pi                                             # :59, sum + ...
        out[b].real, out[b].imag = sr, si                                         # :61
    return out


def covariance(re, im):
    """complex128 [A, A]: R[i, j] = sum_n x_i[n] conj(x_j[n]) of the float32 samples, in float64"""
    x = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    return x @ x.conj().T


# ---- the seeded inputs the CPU and the GPU tests share -----------------------------------------------------------------------------------------
N_MAX = 4099 + 1   # the longest case of the GPU grid, read one item past the buffer's start as well


def case_items(item_type, n_antennas, seed=0):
    """[n_antennas, N_MAX, 2] items of `item_type`: full-range integers, floats over 16 binades"""
    rng = np.random.default_rng([seed, n_antennas, {"gr_complex": 0, "ishort": 1, "ibyte": 2}[item_type]])
    shape = (n_antennas, N_MAX, 2)
    if item_type == "gr_complex":
        return (rng.standard_normal(shape) * np.exp2(rng.integers(-8, 9, shape))).astype(np.float32)
    info = np.iinfo(ITEM_DTYPES[item_type])
    return rng.integers(info.min, info.max + 1, shape).astype(ITEM_DTYPES[item_type])


def case_weights(n_beams, n_antennas, seed=0):
    """random complex64 [n_beams, n_antennas], magnitudes over 8 binades"""
    rng = np.random.default_rng([seed + 100, n_beams, n_antennas])
    shape = (n_beams, n_antennas)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.exp2(rng.integers(-4, 5, shape))).astype(np.complex64)


# ---- the end-to-end scenario: a jammed line array (tests/test_beamformer_gpu.py, re-checked on the CPU by tests/test_beamformer_reference.py) -----
E2E = dict(fs=4000000, n=4000, n_antennas=4, prn=7, cn0_dbhz=47.0, doppler_hz=1250.0, code_phase_chips=300.25, sat_deg=20.0,
           jammer_hz=37000.0, jammer_amplitude=10.0, jammer_deg=-40.0, seed=20260)
E2E_ACQ = dict(fs_in=4000000, fft_size=4000, doppler_max=5000, doppler_step=250, samples_per_chip=4, samples_per_code=4000.0)
E2E_PFA = 0.001


def steering(n_antennas, angle_deg):
    """half-wavelength line array: element k sees exp(j pi k sin(angle))"""
    return np.exp(1j * np.pi * np.arange(n_antennas) * np.sin(np.deg2rad(angle_deg)))


def e2e_block(jammer_amplitude=None, seed=None):
    """complex64 [4, 4000]: GPS PRN 7 from 20 degrees and a CW jammer from -40 degrees over complex noise of unit variance (0.5 per component),
    independent per antenna; the satellite's amplitude is helpers.cn0_to_amplitude(47 dB-Hz), as in every scenario of the suite"""
    import oracle
    from helpers import cn0_to_amplitude
    s = E2E
    n, fs, A = s["n"], float(s["fs"]), s["n_antennas"]
    rng = np.random.default_rng(s["seed"] if seed is None else seed)
    x = (rng.standard_normal((A, n)) + 1j * rng.standard_normal((A, n))) * np.sqrt(0.5)
    t = np.arange(n, dtype=np.float64)
    code = oracle.ca_code(s["prn"]).astype(np.float64)
    f_code = 1.023e6 * (1.0 + s["doppler_hz"] / 1575.42e6)
    chip = np.floor(t * (f_code / fs) + s["code_phase_chips"]).astype(np.int64) % 1023
    sat = cn0_to_amplitude(s["cn0_dbhz"], fs) * code[chip] * np.exp(2j * np.pi * s["doppler_hz"] / fs * t)
    amp = s["jammer_amplitude"] if jammer_amplitude is None else jammer_amplitude
    jam = amp * np.exp(2j * np.pi * s["jammer_hz"] / fs * t)
    x += np.outer(steering(A, s["sat_deg"]), sat) + np.outer(steering(A, s["jammer_deg"]), jam)
    return x.astype(np.complex64)
