"""E/P/L at exactly -0.5 / 0 / +0.5 chip: all three taps from the prompt tap's index chain (csrc/mcorr_device.h packed_trip, half-chip taps).

With the taps half a chip apart, w = fl(fl(step n) - rem) (the prompt chain, the reference's float32 expression) and h = floor(2 w) give
    k_P = h >> 1,  k_L = (h + 1) >> 1,  k_E = (h - 1) >> 1
wherever every value of the early ... late chains of a wave's 128 samples lies in one binade before and after the subtraction of rem; the kernel reads the three
code values as the consecutive words D[h - 1], D[h], D[h + 1] of a doubled table D[h] = code[h >> 1].  A launch takes the form when every job of it qualifies
(multicorrelator.h mcorr_half_chip_eligible); launches of at least 5 120 jobs run the two-wave (128-thread) kernels, smaller ones the four-wave kernels.

The GPU tests use the exact-sum method of tests/test_tracking_gpu.py::test_chip_selection_bit_exact: carrier-free integer-valued input (x = 1, and integer weights that
make a swapped pair of indices visible), so every float32 sum is exact and a tap's output equals the oracle's sum iff every chip index equals oracle.code_indices.
The CPU test holds the identity itself in numpy float32 under the kernel's judgement.
"""
import os
import sys

import numpy as np
import pytest

import oracle

f32 = np.float32
HALF_SHIFTS = [-0.5, 0.0, 0.5]
BIG = 5200  # jobs of a launch that runs the two-wave kernels (mcorr_launch: >= 5 120)


# ------------------------------------------------------------------------------------------------------------ the identity, on the CPU
def _binade(x):
    return int(np.array([x], f32).view(np.uint32)[0] >> 23)


def _identity_mismatches(step, rem, N):
    """One window inside one code period, taps -0.5 / 0 / +0.5.  Returns (wave-chunks that pass the kernel's judgement, those of them in which one of the three
    derived indices differs from its separately evaluated chain or the scaled chain's half-precision pattern is not floor(2 w))."""
    step, rem = f32(step), f32(rem)
    nrem = f32(-rem)
    nf = np.arange(N).astype(f32)
    a = (step * nf).astype(f32)                                   # fl(step * (float)n)
    chain = lambda s: ((a + f32(s)).astype(f32) + nrem).astype(f32)
    kE, kL = np.floor(chain(-0.5)).astype(np.int64), np.floor(chain(0.5)).astype(np.int64)
    w = (a + nrem).astype(f32)                                    # zero prompt shift: no add
    kP = np.floor(w).astype(np.int64)
    S = f32(2.0 ** -23)                                           # the ONE scaled chain the trip evaluates
    us = (((step * S).astype(f32) * nf).astype(f32) + f32(nrem * S)).astype(f32)
    ok = all(x == 0 or abs(float(x)) >= 2.0 ** -100 for x in (step, rem))
    judged = bad = 0
    for c0 in range(0, N - 127, 128):                             # a wave's 128 samples of a chunk: judge() of run_segment_packed
        lo1 = f32(f32(step * f32(c0)) + f32(f32(-0.5) - f32(0.125)))
        hi1 = f32(f32(step * f32(f32(c0) + f32(127))) + f32(f32(0.5) + f32(0.125)))
        lo2, hi2 = f32(lo1 - rem), f32(hi1 - rem)
        if not (ok and lo1 >= 1 and hi1 < 1020 and _binade(lo1) == _binade(hi1) and lo2 >= 1 and hi2 < 1020 and _binade(lo2) == _binade(hi2)):
            continue
        judged += 1
        sl = slice(c0, c0 + 128)
        h = np.floor(us[sl].astype(np.float64) * 2.0 ** 24).astype(np.int64)   # v_cvt_pkrtz_f16_f32's bit pattern below 2^-13
        same = (np.array_equal(h, np.floor(2.0 * w[sl].astype(np.float64)).astype(np.int64)) and np.array_equal(h >> 1, kP[sl])
                and np.array_equal((h + 1) >> 1, kL[sl]) and np.array_equal((h - 1) >> 1, kE[sl]))
        bad += not same
    return judged, bad


def test_half_chip_identity_in_float32():
    """h >> 1, (h + 1) >> 1, (h - 1) >> 1 equal the three float32 chains, and the scaled chain's half-precision pattern equals floor(2 w), in every wave-chunk the
    kernel's judgement admits: random (step, rem) at 4 / 12.5 / 25 / 50 Msps and the awkward cases -- dyadic steps (w exactly on half-chip boundaries), steps one ulp
    apart, code phases on, next to, below and beyond [0, 1), code phases too small to be scaled."""
    rng = np.random.default_rng(7)
    judged = bad = 0
    for i in range(160):
        fs = [4e6, 12.5e6, 25e6, 50e6][i % 4]
        step = f32(1.023e6 * (1.0 + rng.uniform(-5000, 5000) / 1575.42e6) / fs)
        rem = f32(rng.uniform(-1.0, 2.0)) if i % 5 == 0 else f32(rng.uniform(0.0, 1.0))
        j, b = _identity_mismatches(step, rem, int(1040 / float(step)))
        judged, bad = judged + j, bad + b
    assert judged > 10000 and bad == 0, (judged, bad)
    judged2 = bad2 = 0
    for step in (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.040919998, 0.0409200004, 1.023e6 / 4e6):
        for rem in (0.0, 0.5, 0.25, 0.999, -0.3, 1.7, 0.4999999, 0.5000001, 1.0 / 3.0, 1e-20, 1e-33, -1e-33, 1e-37):
            j, b = _identity_mismatches(step, rem, int(min(26000, 1040 / float(f32(step)))))
            judged2, bad2 = judged2 + j, bad2 + b
            if abs(rem) < 2.0 ** -100 and rem != 0:
                assert j == 0  # a code phase whose scaled value would be denormal: no wave-chunk may take the form
    assert judged2 > 5000 and bad2 == 0, (judged2, bad2)


# ------------------------------------------------------------------------------------------------------------ the kernels, on the GPU
def _bank(gpu, codes, max_len=None):
    from gnss_sdr_amd.tracking import CorrelatorBank
    max_len = max_len or max(len(c) for c in codes)
    b = CorrelatorBank(len(codes), max_len, device=gpu)
    for i, c in enumerate(codes):
        b.set_code(i, c)
    return b


def _job(step, rem, length, slot, shifts, offset):
    return dict(sample_offset=int(offset), n_samples=int(length), code_slot=int(slot), shifts_chips=list(shifts), rem_carr_phase_rad=0.0, phase_step_rad=0.0,
                rem_code_phase_chips=float(f32(rem)), code_phase_step_chips=float(f32(step)))


def _one_period(step, code_len, n_max):
    """Samples of a window that stays inside one code period (+ a margin inside the table's guard band): beyond it the wrap path takes the job and the paired trips
    are never reached (tests/test_tracking_gpu.py::_derived_tap_jobs)."""
    return int(min(n_max, (code_len + 20) / float(f32(step))))


def _half_chip_jobs(code_lens, n_max, shifts=HALF_SHIFTS):
    """The job list of the issue: code phases that put w exactly on and one ulp either side of a half-chip boundary for many samples (dyadic steps), windows crossing
    every power of two up to the code length (whole periods from chip 0 on, at several rates), code phases below zero and above one, code phases whose scaled value is
    denormal, whole periods of a 1 023-chip code at 25 Msps (its last chips lie beyond the conversion's range).  Offsets alternate between even and odd samples."""
    jobs = []

    def add(step, rem, length=None, slot=None):
        s = len(jobs) % len(code_lens) if slot is None else slot
        jobs.append(_job(step, rem, length or _one_period(step, code_lens[s], n_max), s, shifts, offset=(len(jobs) * 37) % 129))

    for step in (0.5, 0.25, 0.125, 0.0625, 0.03125):
        for rem in (0.0, 0.5, 0.25, 0.4999999, 0.5000001):
            add(step, rem)
    for step in (1.023e6 / 25e6, 1.023e6 / 4e6, 1.023e6 / 12.5e6, 1.023e6 / 50e6, 1.0, 0.040919998, 0.0409200004):
        for rem in (0.999, -0.3, 1.7, -1.0, 2.5, 1.0 / 3.0, 1e-33, -1e-33, 1e-37, 1e-20):
            add(step, rem)
    for slot in range(len(code_lens)):  # every code of the bank over a whole period at 25 Msps, and short windows that start deep inside it
        add(1.023e6 / 25e6, 0.37, slot=slot)
        add(1.023e6 / 25e6, -0.2, length=700, slot=slot)
        add(0.5, 0.5, length=129, slot=slot)
        add(0.25, 0.25, length=1, slot=slot)
    return jobs


def _expected(job, code, xr):
    sh = np.asarray(job["shifts_chips"], f32)
    idx = oracle.code_indices(job["n_samples"], sh, job["rem_code_phase_chips"], job["code_phase_step_chips"], 0.0, len(code), False)
    seg = xr[job["sample_offset"]:job["sample_offset"] + job["n_samples"]].astype(np.float64)
    return np.array([(code[idx[t]].astype(np.float64) * seg).sum() for t in range(len(sh))])


def _assert_exact(gpu, codes, launches, n_max, max_len=None):
    """Every launch (a list of jobs) once below 5 120 jobs (four-wave kernels) and once repeated to BIG jobs (two-wave kernels), over x = 1 and over integer weights:
    every job's three sums must equal the oracle's."""
    rng = np.random.default_rng(20260)
    streams = [np.ones(n_max + 256, f32), rng.integers(-7, 8, n_max + 256).astype(f32)]
    b = _bank(gpu, codes, max_len)
    for xr in streams:
        b.set_stream_host(xr.astype(np.complex64))
        for jobs in launches:
            expect = np.array([_expected(job, codes[job["code_slot"]], xr) for job in jobs])
            small = b.correlate(jobs)
            many = (jobs * (BIG // len(jobs) + 1))[:BIG]
            big = b.correlate(many)
            for name, out in (("four-wave", small), ("two-wave", big)):
                for j, job in enumerate(jobs):
                    got = out[j, :3]
                    assert np.array_equal(got.real.astype(np.float64), expect[j]), (name, job, got, expect[j])
                    assert np.all(got.imag == 0), (name, job, got)
            reps = BIG // len(jobs)
            tiled = np.tile(small, (reps, 1))
            assert np.array_equal(big[:reps * len(jobs)].view(np.uint32), tiled.view(np.uint32)), "the repeats of a job inside one launch must agree"
    b.close()


def _test_codes(lens, seed):
    rng = np.random.default_rng(seed)
    return [oracle.ca_code(7).astype(np.int32) if n == 1023 else (2 * rng.integers(0, 2, n) - 1).astype(np.int32) for n in lens]


@pytest.mark.gpu
def test_half_chip_taps_select_the_reference_chips(gpu):
    """Launches in which every job qualifies: 1 023-chip codes, a 1 024-chip code (the longest the flavour takes), a 511- and a 40-chip code (windows that run into
    the doubled guard bands)."""
    n_max = 26200
    lens = [1023, 1024, 511, 40]
    codes = _test_codes(lens, 1)
    jobs = _half_chip_jobs(lens, n_max)
    launches = [jobs[k:k + 40] for k in range(0, len(jobs), 40)]
    _assert_exact(gpu, codes, launches, n_max)


@pytest.mark.gpu
@pytest.mark.parametrize("shifts", [[-0.5, 0.0, 0.5000001], [-0.25, 0.0, 0.75], [-0.3, 0.0, 0.3], [-1.0, 0.0, 0.0]])
def test_other_shift_sets_do_not_take_the_form_and_stay_exact(gpu, shifts):
    """Shift sets that must not take the half-chip form -- late one ulp beyond +0.5, a one-chip spacing that is not centred, a spacing that is not one chip, a late tap
    on the prompt -- alone in a launch, and mixed into a launch of jobs that would qualify (the launch as a whole then runs the other kernels)."""
    n_max = 26200
    lens = [1023, 511]
    codes = _test_codes(lens, 2)
    sh = [float(f32(s)) for s in shifts]
    other = _half_chip_jobs(lens, n_max, sh)[::3]
    mixed = [dict(j, shifts_chips=(sh if i % 4 == 1 else HALF_SHIFTS)) for i, j in enumerate(_half_chip_jobs(lens, n_max)[1::3])]
    _assert_exact(gpu, codes, [other, mixed], n_max)


@pytest.mark.gpu
def test_a_2046_chip_code_falls_back_as_a_whole(gpu):
    """A bank whose codes are too long for the doubled table (2 046 chips): the same taps run the paired trips of the plain table, exact up to the last chip."""
    n_max = 52000
    lens = [2046, 2046]
    codes = _test_codes(lens, 3)
    jobs = []
    for i, (step, rem) in enumerate((s, r) for s in (2.046e6 / 25e6, 2.046e6 / 50e6, 0.0625, 0.5) for r in (0.0, 0.5, 0.4999999, 0.5000001, -0.3, 1.7, 1e-33)):
        jobs.append(_job(step, rem, _one_period(step, 2046, n_max), i % 2, HALF_SHIFTS, offset=(i * 37) % 129))
    _assert_exact(gpu, codes, [jobs], n_max)


_AB_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_tracking_half_chip_taps_gpu import BIG, _bank, _half_chip_jobs, _test_codes
from helpers import tracking_params_for
rng = np.random.default_rng(5)
n_max = 26200
lens = [1023, 1024, 511, 40]
x = (rng.standard_normal(n_max + 256) + 1j * rng.standard_normal(n_max + 256)).astype(np.complex64)
b = _bank(0, _test_codes(lens, 1))
b.set_stream_host(x)
jobs = _half_chip_jobs(lens, n_max)
for job in jobs:
    p = tracking_params_for(25e6, float(rng.uniform(-5000, 5000)), rng)
    job["rem_carr_phase_rad"] = p["rem_carr_phase_rad"]
    job["phase_step_rad"] = p["phase_step_rad"]
many = (jobs * (BIG // len(jobs) + 1))[:BIG]
big = b.correlate(many)                      # >= 5 120 jobs: the two-wave kernels
small = b.correlate(jobs)                    # the four-wave kernels
np.save(sys.argv[1], np.concatenate([big, small]))
"""


@pytest.mark.gpu
def test_half_chip_taps_are_bit_identical_to_the_per_tap_chains(gpu, tmp_path):
    """Random complex samples with a carrier, the job list above in one launch of 5 200 jobs (two-wave kernels) and in one of its own length (four-wave kernels), with
    the half-chip trips on (default) and with every fast trip off (GSH_MC_PACKED_BODY=3, read once per process: the per-tap chains at the same work-group size):
    same chips, same products, same accumulators -- the outputs must agree bit for bit."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _AB_SCRIPT.format(root=root, tests=os.path.join(root, "tests"))
    outs = {}
    for body in ("1", "3"):
        f = str(tmp_path / f"out_{body}.npy")
        r = subprocess.run([sys.executable, "-c", script, f], cwd=root, env=dict(os.environ, GSH_MC_PACKED_BODY=body), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[body] = np.load(f)
    assert outs["1"].shape == outs["3"].shape and outs["1"].shape[0] >= BIG + 100
    assert np.all(np.isfinite(outs["1"].view(np.float32)))
    assert np.array_equal(outs["1"].view(np.uint32), outs["3"].view(np.uint32))
