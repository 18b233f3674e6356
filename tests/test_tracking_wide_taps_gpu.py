"""GPU tests of the wide correlator bank (gsh_bank_correlate_wide, csrc/multicorrelator_wide.hip): up to 64 taps per job, standard resampler.

Bars: chip selection EXACT per tap (integer-valued real samples, no carrier: every float32 sum is exact in any order, |sum| <= 7 x 26 000 < 2^24, so
the output equals sum_n x[n] code[idx_t[n]] with oracle.code_indices' indices iff every chip index is right); accumulators within the project's bar
|gpu - truth| / sum|x| <= 1e-6 of the float64 evaluation (helpers.oracle_job / scale_err); a job's output BITS independent of the batch it shares.
"""
import numpy as np
import pytest

import oracle
from helpers import add_code_signal, golden_e1_l5_codes, oracle_job, scale_err, synth_gps_l1_stream, tracking_params_for

pytestmark = pytest.mark.gpu

TOL_SCALE_GPU = 1e-6
WT = 64


def _bank(gpu, codes, max_len=None):
    from gnss_sdr_amd.tracking import CorrelatorBank
    b = CorrelatorBank(len(codes), max_len or max(len(c) for c in codes), device=gpu)
    for i, c in enumerate(codes):
        b.set_code(i, c)
    return b


def _tap_block(n_jobs, max_taps, max_splits=1):
    """The tap block a launch takes (csrc/multicorrelator_wide.hip mcorr_wide_tap_block): the largest of 16 / 8 / 4 that leaves 1 024 work-groups.  The tests
    size their batches with it so that each of the three kernels is reached; a batch that no longer reaches the one it names fails here, not silently."""
    for tb in (16, 8):
        if n_jobs * max_splits * ((max_taps + tb - 1) // tb) >= 1024:
            return tb
    return 4


# ---------------------------------------------------------------------------------------------------------------- exact inputs
def _exact_stream(n, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(-7, 8, size=n).astype(np.float32).astype(np.complex64)


def _exact_codes():
    rng = np.random.default_rng(41)
    pm = lambda n: (2.0 * rng.integers(0, 2, size=n) - 1.0).astype(np.float32)
    return [oracle.ca_code(7), oracle.ca_code(19), pm(2046), pm(10230)]


def _shifts(kind, nt, rng):
    if kind == "uniform":
        sh = 0.1 * (np.arange(nt) - nt // 2)
    elif kind == "pm3":
        sh = np.sort(rng.uniform(-3.0, 3.0, nt))
    elif kind == "pm16":
        sh = np.sort(rng.uniform(-16.0, 16.0, nt))
    elif kind == "pm40":
        sh = np.sort(rng.uniform(-40.0, 40.0, nt))
    elif kind == "dup":
        sh = np.sort(rng.uniform(-2.0, 2.0, nt))
        sh[nt // 2] = sh[nt // 2 - 1]  # two equal shifts
    elif kind == "centre0":
        sh = np.sort(rng.uniform(-1.0, 1.0, nt))
        sh[nt // 2] = 0.0
        sh = np.sort(sh)
    else:
        raise ValueError(kind)
    return np.asarray(sh, np.float32)


STREAM_LEN = 26000 + 5
TAP_COUNTS = (8, 9, 15, 16, 17, 32, 33, 63, 64)
LENGTHS = (1, 63, 255, 1023, 1024, 1025, 4001, 8111, 26000)
STEPS = (0.04, 0.04092, 0.25, 0.5, 0.25575, 1.7)
REMS = (-0.5, 0.0, 0.3, 0.75, 1.0, 1.5)
KINDS = ("uniform", "pm3", "pm16", "pm40", "dup", "centre0")


def _exact_jobs():
    """Every tap count at a block edge x every window length, the other parameters cycling with strides coprime to their list lengths, and the extremes."""
    rng = np.random.default_rng(99)
    jobs = []
    i = 0
    for ti, nt in enumerate(TAP_COUNTS):
        for li, n in enumerate(LENGTHS):
            off = (0, 1, 3, 5, None)[i % 5]
            if off is None or off + n > STREAM_LEN:
                off = STREAM_LEN - n  # the window ends exactly at the stream's end (an odd start for the even lengths, STREAM_LEN is odd)
            jobs.append(dict(sample_offset=off, n_samples=n, code_slot=(i // 2) % 4, rem_code_phase_chips=REMS[(i + ti) % 6],
                             code_phase_step_chips=STEPS[(i + li) % 6], shifts_chips=_shifts(KINDS[(i + 2 * ti) % 6], nt, rng)))
            i += 1
    # +-1 100 chips on a 1 023-chip code at step 1.7: raw indices -1 074 .. 1 910 (negative, and past one period)
    jobs.append(dict(sample_offset=3, n_samples=513, code_slot=0, rem_code_phase_chips=0.25, code_phase_step_chips=1.7,
                     shifts_chips=np.linspace(-1100.0, 1100.0, 64).astype(np.float32)))
    # the longest window at the largest step over each code length: 44 200 chips walked (more than any table holds: whole-code path on the long codes)
    for slot in range(4):
        jobs.append(dict(sample_offset=5, n_samples=26000, code_slot=slot, rem_code_phase_chips=1.5, code_phase_step_chips=1.7,
                         shifts_chips=_shifts("pm40", 64, rng)))
    # window of one sample, odd start at the stream's very end
    jobs.append(dict(sample_offset=STREAM_LEN - 1, n_samples=1, code_slot=2, rem_code_phase_chips=-0.5, code_phase_step_chips=0.5,
                     shifts_chips=_shifts("pm16", 33, rng)))
    return jobs


def _exact_expected(jobs, codes, x, base=0):
    exp = np.zeros((len(jobs), WT), np.float64)
    for j, job in enumerate(jobs):
        code = codes[job.get("code_slot", 0)]
        n, off = job["n_samples"], job.get("sample_offset", 0) + base
        idx = oracle.code_indices(n, job["shifts_chips"], job["rem_code_phase_chips"], job["code_phase_step_chips"], code_len=len(code))
        assert idx.min() >= 0 and idx.max() < len(code)
        exp[j, :len(job["shifts_chips"])] = (code[idx].astype(np.float64) * x[off:off + n].real.astype(np.float64)[None, :]).sum(axis=1)
    assert np.abs(exp).max() < 2 ** 24
    return exp


@pytest.fixture(scope="module")
def exact():
    x = _exact_stream(STREAM_LEN)
    codes = _exact_codes()
    jobs = _exact_jobs()
    return x, codes, jobs, _exact_expected(jobs, codes, x)


def _assert_exact(out, exp):
    assert out.shape == exp.shape and out.dtype == np.complex64
    bad = np.argwhere(out.real.astype(np.float64) != exp)
    assert bad.size == 0, f"{len(bad)} taps differ, first (job, tap) {bad[0]}: gpu {out[tuple(bad[0])]} expected {exp[tuple(bad[0])]}"
    assert np.array_equal(out.real.astype(np.float64), exp)
    assert np.array_equal(out.imag, np.zeros_like(out.imag))


def test_chip_selection_exact(gpu, exact):
    x, codes, jobs, exp = exact
    b = _bank(gpu, codes)
    b.set_stream_host(x)
    _assert_exact(b.correlate_wide(jobs), exp)  # one batch: every tap count, length and code together (two slots and more in one launch)
    # each extreme alone (other launch geometry: small tap blocks), and every job of a few alone
    for j in list(range(len(jobs) - 6, len(jobs))) + [0, 17, 40, 80]:
        _assert_exact(b.correlate_wide([jobs[j]]), exp[j:j + 1])
    # the batch above runs blocks of 4 taps; the same jobs -- every block-edge tap count, length and extreme -- in batches that take blocks of 8 and of 16
    assert _tap_block(len(jobs), 64) == 4
    for extra, tb in ((50, 8), (2 * len(jobs), 16)):
        many = jobs + [jobs[i % len(jobs)] for i in range(extra)]
        assert _tap_block(len(many), 64) == tb
        _assert_exact(b.correlate_wide(many), np.concatenate([exp, exp[np.arange(extra) % len(jobs)]]))
    b.close()


def test_table_beyond_64_kib_of_lds(gpu):
    """A chip-index range just under the table's 16 384 entries: more than 64 KiB of dynamic LDS (table + 1 KiB), which the launch has to ask for."""
    rng = np.random.default_rng(23)
    code = (2.0 * rng.integers(0, 2, size=10230) - 1.0).astype(np.float32)
    n = 9550  # 1.7 chips per sample: 16 235 chips walked, the four taps add 3
    x = _exact_stream(n + 3, seed=5)
    jobs = [dict(sample_offset=3, n_samples=n, code_slot=0, rem_code_phase_chips=0.5, code_phase_step_chips=1.7, shifts_chips=np.array([-1.5, -0.5, 0.0, 1.5], np.float32))]
    a = np.float32(1.7) * np.arange(n, dtype=np.float32)  # the raw (unwrapped) indices of the first and the last tap, float32 operation for operation
    raw = [np.floor((a + np.float32(sh)) - np.float32(0.5)) for sh in (-1.5, 1.5)]
    assert 16128 < int(raw[1].max()) - int(raw[0].min()) + 1 <= 16384 - 16
    b = _bank(gpu, [code])
    b.set_stream_host(x)
    _assert_exact(b.correlate_wide(jobs), _exact_expected(jobs, [code], x))
    b.close()


# ---------------------------------------------------------------------------------------------------------------- noise + carrier
FS2, N2 = 25e6, 25000
PRNS2 = (1, 3, 8, 11, 14, 22, 27, 31)
DOPP2 = (1200.0, -3400.0, 250.0, 4100.0, -800.0, 2900.0, -4700.0, 60.0)


def _config2_jobs(n_taps, span):
    rng = np.random.default_rng(5)
    params = [tracking_params_for(FS2, d, rng) for d in DOPP2]
    sh = np.linspace(-span, span, n_taps).astype(np.float32)
    return [dict(sample_offset=(e * N2 + 3 * c + e), n_samples=N2, code_slot=c, shifts_chips=sh, **params[c]) for e in range(4) for c in range(8)]


@pytest.fixture(scope="module")
def config2():
    """BASELINE config 2's window: 25 Msps, N = 25 000, 8 embedded signals; 32 jobs x 64 taps and 32 jobs x 16 taps with their float64 truths."""
    x = synth_gps_l1_stream(5 * N2, FS2, PRNS2, DOPP2, [10.0 + 100.0 * i for i in range(8)], seed_noise=0x5EED0002)
    codes = [oracle.ca_code(p) for p in PRNS2]
    sets = {}
    for nt, span in ((64, 3.15), (16, 1.5)):
        jobs = _config2_jobs(nt, span)
        truth = [oracle_job(codes[j["code_slot"]], x, j)[1:] for j in jobs]
        sets[nt] = (jobs, truth)
    return x, codes, sets


def _worst(out, jobs, truth):
    worst = 0.0
    for j, (job, (t64, sabs)) in enumerate(zip(jobs, truth)):
        nt = len(job["shifts_chips"])
        worst = max(worst, float(scale_err(out[j, :nt], t64, sabs).max()))
        assert np.all(out[j, nt:] == 0), f"job {j}: taps beyond n_taps must be zero"
    return worst


@pytest.mark.parametrize("nt", [64, 16])
def test_accumulators_against_float64_truth(gpu, config2, nt):
    x, codes, sets = config2
    jobs, truth = sets[nt]
    b = _bank(gpu, codes)
    b.set_stream_host(x)
    w = _worst(b.correlate_wide(jobs), jobs, truth)
    print(f"32 jobs x {nt} taps: worst |gpu - truth| / sum|x| = {w:.3g}")
    assert w <= TOL_SCALE_GPU
    b.close()


@pytest.mark.parametrize("copies,extra,tb", [(8, 0, 16), (4, 2, 8)])
def test_accumulators_in_blocks_of_16_and_8_taps(gpu, config2, copies, extra, tb):
    """The same 32 x 64-tap jobs (noise + carrier, re-seeded phasors) in batches large enough for the 16-tap and the 8-tap kernel: every row to the bar."""
    x, codes, sets = config2
    jobs, truth = sets[64]
    many, many_truth = jobs * copies + jobs[:extra], truth * copies + truth[:extra]
    assert _tap_block(len(many), 64) == tb
    b = _bank(gpu, codes)
    b.set_stream_host(x)
    w = _worst(b.correlate_wide(many), many, many_truth)
    print(f"{len(many)} jobs x 64 taps, blocks of {tb}: worst |gpu - truth| / sum|x| = {w:.3g}")
    assert w <= TOL_SCALE_GPU
    b.close()


def test_one_segment_longer_than_the_seed_table(gpu):
    """One segment of 400 000 samples (explicit set_splits(1)): beyond the factor table's 20 exact seeds (327 680 samples) every lane evaluates its own."""
    fs, n = 25e6, 400000
    x = synth_gps_l1_stream(n + 5, fs, [4], [2300.0], [200.0], seed_noise=31)
    rng = np.random.default_rng(8)
    job = dict(sample_offset=5, n_samples=n, code_slot=0, shifts_chips=np.linspace(-1.0, 1.0, 9).astype(np.float32), **tracking_params_for(fs, 2300.0, rng))
    code = oracle.ca_code(4)
    _, t64, sabs = oracle_job(code, x, job)
    b = _bank(gpu, [code])
    b.set_stream_host(x)
    for s in (1, 0):
        b.set_splits(s)
        out = b.correlate_wide([job])
        w = float(scale_err(out[0, :9], t64, sabs).max())
        print(f"N = 400 000, 9 taps, set_splits({s}): worst |gpu - truth| / sum|x| = {w:.3g}")
        assert w <= TOL_SCALE_GPU and np.all(out[0, 9:] == 0)
    b.close()


def test_galileo_e1_33_taps(gpu):
    e1b = golden_e1_l5_codes()["e1b"][10]
    fs, n = 32e6, 128000
    rate = 8184.0 / n * (1.0 + 1500.0 / 1575.42e6)
    rng = np.random.default_rng(12)
    x = (rng.standard_normal(n + 9) + 1j * rng.standard_normal(n + 9)).astype(np.complex64)
    add_code_signal(x, e1b, fs, rate, 411.3, 1500.0, 0.05, 0.7)
    job = dict(sample_offset=7, n_samples=n, code_slot=0, rem_carr_phase_rad=0.4, phase_step_rad=float(np.float32(2 * np.pi * 1500.0 / fs)),
               rem_code_phase_chips=0.6, code_phase_step_chips=float(np.float32(rate)), shifts_chips=np.linspace(-2.0, 2.0, 33).astype(np.float32))
    _, t64, sabs = oracle_job(e1b, x, job)
    b = _bank(gpu, [e1b])
    b.set_stream_host(x)
    out = b.correlate_wide([job])
    w = float(scale_err(out[0, :33], t64, sabs).max())
    print(f"Galileo E1, N = 128 000, 33 taps: worst |gpu - truth| / sum|x| = {w:.3g}")
    assert w <= TOL_SCALE_GPU and np.all(out[0, 33:] == 0)
    b.close()


def test_output_bits_do_not_depend_on_the_batch(gpu, config2):
    x, codes, sets = config2
    probe = sets[64][0][13]
    rng = np.random.default_rng(77)
    others = []
    for i in range(39):
        nt = int(rng.integers(1, 65))
        n = int(rng.choice([700, 2048, 9000, 25000, 60000]))
        others.append(dict(sample_offset=int(rng.integers(0, 5 * N2 - n)), n_samples=n, code_slot=i % 8, rem_carr_phase_rad=0.3 * i, phase_step_rad=0.001 * i,
                           rem_code_phase_chips=0.1 * (i % 10), code_phase_step_chips=0.04092, shifts_chips=np.sort(rng.uniform(-5, 5, nt)).astype(np.float32)))
    b = _bank(gpu, codes)
    b.set_stream_host(x)
    alone = b.correlate_wide([probe])[0]
    first = b.correlate_wide([probe] + others)[0]
    last = b.correlate_wide(others + [probe])[-1]
    assert np.array_equal(alone.view(np.uint32), first.view(np.uint32))
    assert np.array_equal(alone.view(np.uint32), last.view(np.uint32))
    # the three launches above take blocks of 4 taps.  "The tap block changes no sum": the probe inside batches that take blocks of 8 and of 16 ...
    fill = sets[64][0]
    for n_fill, tb in ((129, 8), (259, 16)):
        batch = [fill[i % 32] for i in range(n_fill)]
        assert _tap_block(n_fill + 1, 64) == tb
        got = b.correlate_wide(batch[:n_fill // 2] + [probe] + batch[n_fill // 2:])[n_fill // 2]
        assert np.array_equal(alone.view(np.uint32), got.view(np.uint32)), f"blocks of {tb}"
    # ... and beside a job long enough for two segments: the launch then goes through partial sums and wide_taps_reduce, the probe's single one included
    long_job = dict(fill[0], sample_offset=11, n_samples=70000)
    _, t64_long, sabs_long = oracle_job(codes[0], x, long_job)
    for n_fill, tb in ((68, 8), (138, 16)):
        batch = [fill[i % 32] for i in range(n_fill)] + [long_job]
        assert _tap_block(n_fill + 2, 64, max_splits=2) == tb
        got = b.correlate_wide([probe] + batch)
        assert np.array_equal(alone.view(np.uint32), got[0].view(np.uint32)), f"blocks of {tb}, two segments"
        assert float(scale_err(got[-1], t64_long, sabs_long).max()) <= TOL_SCALE_GPU
    t64, sabs = sets[64][1][13]
    assert float(scale_err(alone, t64, sabs).max()) <= TOL_SCALE_GPU
    b.close()


def test_splits(gpu, exact, config2):
    x, codes, jobs, exp = exact
    b = _bank(gpu, codes)
    b.set_stream_host(x)
    outs = []
    for s in (1, 4, 0):
        b.set_splits(s)
        outs.append(b.correlate_wide(jobs))
        _assert_exact(outs[-1], exp)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)) and np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    b.close()
    x2, codes2, sets = config2
    jobs2, truth2 = sets[64]
    b = _bank(gpu, codes2)
    b.set_stream_host(x2)
    for s in (1, 4, 0):
        b.set_splits(s)
        w = _worst(b.correlate_wide(jobs2[:8]), jobs2[:8], truth2[:8])
        print(f"splits {s}: worst |gpu - truth| / sum|x| = {w:.3g}")
        assert w <= TOL_SCALE_GPU
    b.close()


def test_ring_bound_bank(gpu):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    cap, win, blk = 9002, 4000, 3001
    x = _exact_stream(6 * blk, seed=8)
    codes = _exact_codes()[:2]
    ring = SampleStream(cap, win, device=gpu)
    b = _bank(gpu, codes)
    b.set_stream_ring(ring)
    rng = np.random.default_rng(4)
    sh = _shifts("pm16", 64, rng)
    n_across = 0
    for k in range(6):
        assert ring.push(x[k * blk:(k + 1) * blk]) == k * blk
        lo, hi = ring.range()
        # windows by absolute index, newest first; every other block the job table is relative and the sample base moves it, by one block
        base = (k - 1) * blk if k % 2 else 0
        b.set_sample_base(base)
        jobs = []
        for c, n in enumerate((2999, 4000, 1025, 513)):
            off = hi - n - 7 * c
            if off < lo:
                continue
            jobs.append(dict(sample_offset=off - base, n_samples=n, code_slot=c % 2, rem_code_phase_chips=0.5, code_phase_step_chips=0.25575, shifts_chips=sh[:64 - 9 * c]))
            if off % cap + n > cap:
                n_across += 1
        _assert_exact(b.correlate_wide(jobs), _exact_expected(jobs, codes, x, base=base))
    assert n_across >= 3
    b.set_sample_base(0)
    lo, hi = ring.range()
    with pytest.raises(GshError):
        b.correlate_wide([dict(sample_offset=lo - 1, n_samples=100, shifts_chips=sh)])
    with pytest.raises(GshError):
        b.correlate_wide([dict(sample_offset=hi - 99, n_samples=100, shifts_chips=sh)])
    b.close()
    ring.close()


def test_facade_33_correlators(gpu):
    """The call pattern of test_tracking_gpu.py::test_reference_unit_test_case with 33 correlators: the standard resampler serves them, the object's default
    (high dynamics, as in the reference) is refused and leaves zeros."""
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.tracking import HipMulticorrelatorRealCodes
    rng = np.random.default_rng(7)
    vlen = 8192
    in_cpu = (rng.random(2 * vlen) + 1j * rng.random(2 * vlen)).astype(np.complex64)
    ca = oracle.ca_code(1)
    outs = np.full(33, 5 + 5j, np.complex64)
    shifts = np.linspace(-1.6, 1.6, 33).astype(np.float32)
    mc = HipMulticorrelatorRealCodes(gpu)
    assert mc.init(vlen, 33)
    assert mc.set_input_output_vectors(outs, in_cpu)
    assert mc.set_local_code_and_taps(1023, ca, shifts)
    with pytest.raises(GshError) as e:  # the flag at its default
        mc.Carrier_wipeoff_multicorrelator_resampler(0.0, 0.1, 0.4, 0.3, 0.00001, 4096)
    assert "GSH_ERR_UNSUPPORTED" in str(e.value) and "set_high_dynamics_resampler(false)" in str(e.value)
    assert np.all(outs == 0)
    mc.set_high_dynamics_resampler(False)
    for form in (7, 6):
        if form == 7:
            assert mc.Carrier_wipeoff_multicorrelator_resampler(1.0, 0.05, 0.0, 0.2, 0.25, 0.0, 4096)
            job = dict(n_samples=4096, shifts_chips=shifts.copy(), rem_carr_phase_rad=1.0, phase_step_rad=0.05, rem_code_phase_chips=0.2, code_phase_step_chips=0.25)
        else:
            shifts[:] = np.linspace(-0.8, 2.4, 33).astype(np.float32)  # borrowed: mutated in place between calls (trk.cc:2132-2146)
            assert mc.Carrier_wipeoff_multicorrelator_resampler(0.0, 0.1, 0.4, 0.3, 0.0, 8192)
            job = dict(n_samples=8192, shifts_chips=shifts.copy(), rem_carr_phase_rad=0.0, phase_step_rad=0.1, rem_code_phase_chips=0.4, code_phase_step_chips=0.3)
        _, t64, sabs = oracle_job(ca, in_cpu, job)
        w = float(scale_err(outs, t64, sabs).max())
        print(f"{form}-argument call, 33 correlators: worst |gpu - truth| / sum|x| = {w:.3g}")
        assert w <= TOL_SCALE_GPU
    assert mc.free()
    mc.close()


def test_errors_leave_the_bank_usable(gpu, exact):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.tracking import CorrelatorBank
    x, codes, jobs, exp = exact
    b = CorrelatorBank(5, 10230, device=gpu)  # slot 4 stays empty
    for i, c in enumerate(codes):
        b.set_code(i, c)
    ok = dict(n_samples=100, shifts_chips=np.linspace(-1, 1, 20).astype(np.float32), code_phase_step_chips=0.25)
    with pytest.raises(GshError, match="no sample stream"):
        b.correlate_wide([ok])
    b.set_stream_host(x)
    narrow = [dict(sample_offset=3, n_samples=4001, code_slot=1, rem_code_phase_chips=0.5, code_phase_step_chips=0.25, shifts_chips=[-0.5, 0.0, 0.5])]
    narrow_exp = _exact_expected(narrow, codes, x)[:, :8]
    b.upload_jobs(narrow)  # a staged narrow table: the wide calls, failed or not, leave it alone
    bad = [
        (dict(ok, n_taps=0), "n_taps"),
        (dict(ok, n_taps=65), "n_taps"),
        (dict(ok, shifts_chips=np.array([0.0, 0.5, 0.25, 1.0], np.float32)), "ascend"),
        (dict(ok, code_slot=4), "no local code"),
        (dict(ok, sample_offset=STREAM_LEN - 99), "past"),
        (dict(ok, code_phase_step_chips=float("nan")), "finite"),
    ]
    for job, what in bad:
        with pytest.raises(GshError, match=what) as e:
            b.correlate_wide([jobs[0], job])
        assert "job 1" in str(e.value)
    out = b.correlate_wide([])
    assert out.shape == (0, WT) and out.dtype == np.complex64
    b.launch()
    b.synchronize()
    got = b.read_outputs()
    assert np.array_equal(got.real.astype(np.float64), narrow_exp) and np.all(got.imag == 0)
    _assert_exact(b.correlate_wide(jobs[:20]), exp[:20])
    got = b.correlate(narrow)
    assert np.array_equal(got.real.astype(np.float64), narrow_exp)
    b.close()
