"""GPU tests of the signal generator (gsh_gen_*, gnss_sdr_amd.SignalGenerator) against the numpy float64 model of tests/siggen_reference.py and the
reference block's own output in tests/golden/siggen.npz.

Bars.  Device against model, per sample: |gpu - model| <= K 2^-24 sum_sat amplitude (amplitude = the satellite's largest |A| + |B|).  K was
measured on one MI355X over every case of tests 1, 2 and 5 below: the worst ratio |gpu - model| / (2^-24 sum amplitude) was 2.713 (one random
satellite of shape "single"; 2.28 on the golden GPS case); K is twice that rounded up to a power of two, headroom for other boxes as helpers.py keeps for the
correlator bars.  Device against the reference block: ref_vs_model_max of the fixture (the reference's float32 phase accumulation) + the bar above.
Noise, per sample (test 5): with r = the sample's Box-Muller radius, the float32 evaluation errs by pi 2^-25 r (the angle rounded to float32) +
2 ulp of sincospif + 1.5 ulp of r (logf, the square root, the product by -2 exact) + half an ulp of each product, 6.1 2^-24 r per component, and half
an ulp of the final sum (at most sum amplitude + r); times sqrt 2 for the complex magnitude: 9 2^-24 r + 2^-24 sum amplitude.
Everything between two device results (cuts, seeks, ring windows, noise on = noise off + noise) is bit for bit."""
import numpy as np
import pytest

import oracle
import siggen_reference as R
from test_siggen_reference import built_satellites, golden  # noqa: F401  (the fixture file, loaded once per module)

pytestmark = pytest.mark.gpu

MEASURED_WORST = 2.713  # worst |gpu - model| / (2^-24 sum amplitude) over tests 1, 2 and 5 on one MI355X
K = 8                  # twice that, rounded up to a power of two
U = 2.0 ** -24
E2E_SEED = 2013      # test 7: on the CPU the oracle detects the model stream plus this seed's noise restated in numpy (statistic 64.6, threshold 45.5)


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


class Gen:
    """a SignalGenerator with its satellites, and samples read back through a device buffer whose first sample may sit on an odd 8-byte slot"""

    def __init__(self, gpu, fs, sats):
        import torch
        from gnss_sdr_amd import SignalGenerator
        self.torch, self.gpu, self.fs, self.sats = torch, gpu, fs, sats
        self.g = SignalGenerator(fs, len(sats), device=gpu)
        for i, s in enumerate(sats):
            self.g.set_satellite(i, s)

    def samples(self, n0, n, slot=0, seek=True):
        if seek:
            self.g.seek(n0)
        assert self.g.position() == n0
        buf = self.torch.full((n + 4, 2), 7.0, dtype=self.torch.float32, device=f"cuda:{self.gpu}")
        self.torch.cuda.synchronize(self.gpu)     # the fill runs on torch's stream, the generator on its own: the fill must have landed first
        self.g.generate_device(n, buf.data_ptr() + 8 * slot)
        assert self.g.position() == n0 + n
        host = buf.cpu().numpy().view(np.complex64).reshape(-1)
        assert np.all(host[:slot] == 7 + 7j) and np.all(host[slot + n:] == 7 + 7j)     # nothing outside [slot, slot + n) was written
        return host[slot:slot + n].copy()

    def close(self):
        self.g.close()


def worst_ratio(got, want, sats):
    return float(np.abs(got.astype(np.complex128) - want).max() / (U * R.amplitude_sum(sats))) if got.size else 0.0


# ---- 1. the reference block's own output ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["gps", "e5a"])
def test_fixture_parity(gpu, golden, tag):  # noqa: F811
    g = golden
    sats = built_satellites(g, tag)
    fs = float(g[f"{tag}_fs"])
    ref = g[f"{tag}_out"]
    gen = Gen(gpu, fs, sats)
    try:
        got = gen.samples(0, ref.size)
    finally:
        gen.close()
    want = R.model(sats, fs, 0, ref.size)
    ratio = worst_ratio(got, want, sats)
    bar = K * U * R.amplitude_sum(sats)
    vs_ref = float(np.abs(got.astype(np.complex128) - ref.astype(np.complex128)).max())
    print(f"fixture {tag}: worst |gpu - model| / (2^-24 sum amplitude) = {ratio:.3f} (K = {K}); |gpu - reference| = {vs_ref:.3e}, "
          f"bar {float(g[f'{tag}_ref_vs_model_max']) + bar:.3e}")
    assert ratio <= K
    assert vs_ref <= float(g[f"{tag}_ref_vs_model_max"]) + bar


# ---- 2. the three combination shapes at the smallest sizes that can break them ---------------------------------------------------------------------
PERIODS = [1, 2, 255, 257, 1023]
SIGN_LENGTHS = [1, 20, 100]


def _random_satellite(rng, shape, period, delay, k):
    """shape "single": A alone (GPS / GLONASS); "pilot": A + B with sB = +1 (Galileo E1 / E6); "iq": A = (Re, 0), B = (0, Im), both signed (E5a / E5b)"""
    from gnss_sdr_amd.signal_generator import Satellite
    amp = np.float32(rng.uniform(0.25, 2.0))
    cplx = lambda: ((rng.standard_normal(period) + 1j * rng.standard_normal(period)) * amp).astype(np.complex64)   # noqa: E731
    la, lb = SIGN_LENGTHS[k % 3], SIGN_LENGTHS[(k + 1) % 3]
    signs = lambda n: (2 * rng.integers(0, 2, n) - 1).astype(np.int8)   # noqa: E731
    if shape == "single":
        a, b, sa, sb = cplx(), None, signs(la), np.ones(1, np.int8)
    elif shape == "pilot":
        a, b, sa, sb = cplx(), cplx(), signs(la), np.ones(1, np.int8)
    else:
        t = cplx()
        a, b, sa, sb = t.real.astype(np.complex64), (1j * t.imag).astype(np.complex64), signs(la), signs(lb)
    return Satellite(a, b, delay, sa, sb, doppler_hz=float(rng.uniform(-9000.0, 9000.0)), start_phase_rad=float(rng.uniform(-7.0, 7.0)),
                     carrier_offset_hz=float(rng.choice([0.0, 562500.0 * rng.integers(-7, 7)])))


def _starts(period, delay):
    """an even and an odd absolute start from which a sign boundary lies exactly 512 samples (one work-group's tile) on"""
    first = (delay - 512) % period
    cands = [first + m * period for m in range(1, 5)]
    even = next((c for c in cands if c % 2 == 0), cands[0] + 1 if cands[0] % 2 else cands[0])
    odd = next((c for c in cands if c % 2 == 1), cands[0] if cands[0] % 2 else cands[0] + 1)
    return even, odd


@pytest.mark.parametrize("n_sats", [1, 2, 9, 32])
@pytest.mark.parametrize("shape", ["single", "pilot", "iq"])
def test_combination_shapes_against_the_model(gpu, shape, n_sats):
    rng = np.random.default_rng([n_sats, len(shape)])
    fs, worst = 4e6, 0.0
    for period in PERIODS:
        for delay in sorted({0, min(1, period - 1), period - 1}):
            sats = [_random_satellite(rng, shape, period, delay, k) for k in range(n_sats)]
            gen = Gen(gpu, fs, sats)
            try:
                for start in _starts(period, delay):
                    for n in (1, 2, 511, 513, 3 * period + 7):
                        got = gen.samples(start, n, slot=start % 2)
                        ratio = worst_ratio(got, R.model(sats, fs, start, n), sats)
                        worst = max(worst, ratio)
                        assert ratio <= K, (shape, n_sats, period, delay, start, n, ratio)
            finally:
                gen.close()
    print(f"shape {shape}, S = {n_sats}: worst |gpu - model| / (2^-24 sum amplitude) = {worst:.3f} (K = {K})")


# ---- 3. cut invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_stretch(gpu, golden):  # noqa: F811
    """samples [0, 40 003) of the scaled golden GPS scenario in one call, noise off and on: computed once, shared, left unchanged"""
    sats = built_satellites(golden, "gps", scaled=True)
    gen = Gen(gpu, 4e6, sats)
    try:
        off = gen.samples(0, 40003)
        gen.g.set_noise(True, 20131)
        on = gen.samples(0, 40003)
    finally:
        gen.close()
    return sats, off, on


@pytest.mark.parametrize("noise", [False, True])
def test_cuts_and_seeks_change_no_bit(gpu, whole_stretch, noise):
    sats, off, on = whole_stretch
    whole = on if noise else off
    gen = Gen(gpu, 4e6, sats)
    try:
        gen.g.set_noise(noise, 20131)
        at, pieces = 0, []
        for n in (1, 513, 4000, 35489):
            pieces.append(gen.samples(at, n, slot=at % 2, seek=False))      # consecutive calls, no seek in between
            at += n
        assert at == 40003 and np.array_equal(_bits(np.concatenate(pieces)), _bits(whole))
        gen.g.seek(12345)
        assert np.array_equal(_bits(gen.samples(12345, 40003 - 12345, slot=1, seek=False)), _bits(whole[12345:]))
    finally:
        gen.close()


def test_time_generate_leaves_the_position_alone_and_generate_reads_back(gpu, whole_stretch):
    sats, off, on = whole_stretch
    gen = Gen(gpu, 4e6, sats)
    try:
        gen.g.seek(777)
        ms = gen.g.time_generate(1 << 16, reps=3)
        assert ms > 0.0 and gen.g.position() == 777
        assert np.array_equal(_bits(gen.samples(777, 1000, seek=False)), _bits(off[777:1777]))
        assert np.array_equal(_bits(gen.g.generate(1001)), _bits(off[1777:2778])) and gen.g.position() == 2778     # the read-back convenience of the Python face
        assert gen.g.generate(0).size == 0 and gen.g.position() == 2778
    finally:
        gen.close()


# ---- 4. straight into a ring -----------------------------------------------------------------------------------------------------------------------
def test_ring_windows_equal_the_generated_samples(gpu, whole_stretch):
    from gnss_sdr_amd.sample_stream import SampleStream
    sats, off, on = whole_stretch
    ring = SampleStream(8192, 4000, device=gpu)
    gen = Gen(gpu, 4e6, sats)
    try:
        gen.g.set_noise(True, 20131)
        for i in range(3):                                   # 15 000 samples through a ring of 8 192: the second and third push wrap
            assert gen.g.push(ring, 5000) == 5000 * i and gen.g.position() == 5000 * (i + 1)
            lo, hi = ring.range()
            assert (lo, hi) == (max(0, 5000 * (i + 1) - 8192), 5000 * (i + 1))
            assert np.array_equal(_bits(ring.read(lo, hi - lo)), _bits(on[lo:hi]))
            for first, n in ((lo, 1), (hi - 4000, 4000), (lo + 1, 3999)):      # windows as a reader takes them (the mirror past the wrap)
                assert np.array_equal(_bits(ring.read(first, n)), _bits(on[first:first + n]))
        # more than the ring holds: refused before anything moves
        from gnss_sdr_amd import GshError
        with pytest.raises(GshError) as e:
            gen.g.push(ring, 8193)
        assert e.value.code == 1 and ring.range() == (15000 - 8192, 15000) and gen.g.position() == 15000
    finally:
        gen.close()
        ring.close()


def test_push_past_a_live_reader_is_refused_and_moves_nothing(gpu):
    """a live tracking channel reads the ring (the ring's only kind of reader that a push can overrun: events order the others); a push that would
    overwrite its next window is GSH_ERR_STATE, and ring and generator stay as they were"""
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.signal_generator import gps_l1_ca_satellite
    from test_tracking_live_gpu import FS, KW, N, _drain, _loop
    sats = [gps_l1_ca_satellite(5, int(FS), delay_chips=100, doppler_hz=-1900.0, cn0_db=50.0)]
    ring = SampleStream(8192, 2 * N, device=gpu)
    gen = Gen(gpu, FS, sats)
    live = _loop(gpu, dict(KW, enable_lock_detectors=0), n_channels=1)
    try:
        gen.g.set_noise(True, 5)
        live.set_stream_ring(ring)
        live.start(0, oracle.ca_code(5), 200, 0, -1900.0 + 6.0)
        live.live_configure(idle_timeout_us=100000, residency_us=1000000)
        assert gen.g.push(ring, 8000) == 0
        before = ring.range()
        held = ring.read(before[0], before[1] - before[0])
        live.live_begin()
        got, lost = [[]], [False]
        _drain(live, got, lost, 2.0, want=[2])
        assert len(got[0]) >= 2
        # the channel stands below 8 000; the ring holds 8 192: 8 192 more would overwrite its next window
        with pytest.raises(GshError) as e:
            gen.g.push(ring, 8192)
        assert e.value.code == 4, str(e.value)
        assert ring.range() == before and gen.g.position() == 8000
        live.live_quiesce()
        assert np.array_equal(_bits(ring.read(before[0], before[1] - before[0])), _bits(held))
        assert gen.g.push(ring, 100) == 8000                 # and the ring still takes the next samples where it stood
    finally:
        live.close()
        gen.close()
        ring.close()


# ---- 5. a large absolute index ---------------------------------------------------------------------------------------------------------------------
def test_phase_and_noise_at_two_to_the_forty(gpu, golden):  # noqa: F811
    sats = built_satellites(golden, "gps", scaled=True)
    fs, start, n, seed = 4e6, 2 ** 40 + 1, 4100, 0x1234567890ABCDEF
    gen = Gen(gpu, fs, sats)
    try:
        off = gen.samples(start, n, slot=1)
        gen.g.set_noise(True, seed)
        on = gen.samples(start, n, slot=1)
    finally:
        gen.close()
    want = R.model(sats, fs, start, n)
    ratio = worst_ratio(off, want, sats)
    print(f"start 2^40 + 1: worst |gpu - model| / (2^-24 sum amplitude) = {ratio:.3f} (K = {K})")
    assert ratio <= K
    noise = R.noise(seed, start, n)
    amp = R.amplitude_sum(sats)
    err = np.abs(on.astype(np.complex128) - (want + noise))
    bar = K * U * amp + 9.0 * U * np.abs(noise) + U * amp
    print(f"noise at 2^40 + 1: worst error / bar = {(err / bar).max():.3f}")
    assert np.all(err <= bar)
    assert np.abs(noise).max() > 3.0          # the stretch is long enough to hold large radii


# ---- 6. noise moments: sampling bounds, five standard deviations --------------------------------------------------------------------------------------
def _corr(a, b):
    return float(np.mean(a * b) / np.sqrt(np.mean(a * a) * np.mean(b * b)))


def test_noise_moments(gpu):
    from gnss_sdr_amd.signal_generator import Satellite
    n = 1 << 22
    silent = [Satellite(np.zeros(1, np.complex64), None, 0)]
    gen = Gen(gpu, 4e6, silent)
    try:
        gen.g.set_noise(True, 42)
        x = gen.samples(0, n).astype(np.complex128)
        gen.g.set_noise(True, 43)
        y = gen.samples(0, n).astype(np.complex128)
    finally:
        gen.close()
    five = 5.0 / np.sqrt(n)
    for part in (x.real, x.imag):
        assert abs(part.mean()) <= five
        assert abs(part.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
        assert abs(_corr(part[1:] - part.mean(), part[:-1] - part.mean())) <= five      # lag-1 autocorrelation
    assert abs(_corr(x.real, x.imag)) <= five
    assert abs(_corr(x.real[1:], x.imag[:-1])) <= five and abs(_corr(x.imag[1:], x.real[:-1])) <= five
    for a in (x.real, x.imag):                                                          # two seeds: unrelated streams
        for b in (y.real, y.imag):
            assert abs(_corr(a, b)) <= five
    assert not np.array_equal(x[:16], y[:16])


def test_noise_on_is_noise_off_plus_noise_exactly(gpu, whole_stretch):
    from gnss_sdr_amd.signal_generator import Satellite
    sats, off, on = whole_stretch
    gen = Gen(gpu, 4e6, [Satellite(np.zeros(1, np.complex64), None, 0)])
    try:
        gen.g.set_noise(True, 20131)
        only = gen.samples(0, off.size)
    finally:
        gen.close()
    total = np.empty_like(off)
    total.real = off.real + only.real        # float32 additions, as the kernel's last step
    total.imag = off.imag + only.imag
    assert np.array_equal(total, on) and np.abs(only).max() > 3.0


# ---- 7. end to end on the device: generator -> ring -> PCPS acquisition -------------------------------------------------------------------------------
def test_generator_feeds_acquisition_on_the_device(gpu):
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank, compute_threshold
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.signal_generator import gps_l1_ca_satellite
    from oracle.pcps_oracle import PcpsOracle
    fs, n, seed = 4000000, 4000, E2E_SEED
    sats = [gps_l1_ca_satellite(10, fs, delay_chips=600, doppler_hz=750.0, cn0_db=44.0)]      # the gsoc2013 scenario
    kw = dict(fs_in=fs, fft_size=n, doppler_max=10000, doppler_step=250, samples_per_chip=4, samples_per_code=float(n))
    code = oracle.ca_code_complex_sampled(10, fs)
    ora = PcpsOracle(**kw)
    ora.set_local_code(code)
    exp = ora.dwell(R.model(sats, fs, 0, n).astype(np.complex64))
    thr = compute_threshold(0.001, n, 80, 1)
    noisy = ora.dwell(R.model(sats, fs, 0, n, noise_seed=seed).astype(np.complex64))
    assert (noisy["index_time"], noisy["index_doppler"]) == (exp["index_time"], exp["index_doppler"]) and noisy["test_statistics"] > thr   # the seed's premise
    ring = SampleStream(8192, n, device=gpu)
    gen = Gen(gpu, fs, sats)
    acq = PcpsAcquisitionBank(device=gpu, max_prn=1, **kw)
    try:
        acq.set_local_code(0, code)
        assert gen.g.push(ring, n) == 0
        clean = acq.dwell_ring(ring, 0, 1)[0]
        assert (clean["index_time"], clean["index_doppler"], clean["doppler_hz"]) == (exp["index_time"], exp["index_doppler"], exp["doppler_hz"])
        assert clean["doppler_hz"] == 750
        gen.g.set_noise(True, seed)
        gen.g.seek(0)
        first = gen.g.push(ring, n)
        got = acq.dwell_ring(ring, first, 1)[0]
        print(f"acquisition with noise: statistic {got['test_statistics']:.2f} (oracle on model + numpy noise {noisy['test_statistics']:.2f}), threshold {thr:.2f}")
        assert (got["index_time"], got["index_doppler"]) == (exp["index_time"], exp["index_doppler"])
        assert got["test_statistics"] > thr
    finally:
        acq.close()
        gen.close()
        ring.close()

