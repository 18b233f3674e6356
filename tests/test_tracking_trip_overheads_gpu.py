"""What an E/P/L job pays outside its plain half-chip trips (csrc/mcorr_device.h run_segment_packed, csrc/multicorrelator.hip): the three places that changed.

  1. A run of half-chip trips continues across the end of a 64-chunk judgement mask word (trip 32 at two chunks per trip) instead of ending in a per-tap trip.
  2. The half-chip kernels stage both code tables as a copy of an image the host builds when a code is set (gsh_bank_set_code), not element by element.
  3. The integer sample number of a lane is formed inside the re-seed and edge branches only; the loads take a scalar base and a constant lane offset.

None of them changes a product or the order of a sum: every output must stay bit-identical to the per-tap chains (GSH_MC_PACKED_BODY=3) at the same work-group size, and
the chips must stay the reference's.  GSH_MC_WG and GSH_MC_PACKED_BODY are read once per process, so the kernels run in child processes (one per work-group size and
body, started together, their outputs shared by the tests below); the staged-image test needs neither switch and runs in this process.

Exact chips: the method of tests/test_tracking_half_chip_taps_gpu.py -- carrier-free integer-valued input, so every float32 sum is exact and a tap's output equals the
oracle's sum iff every chip index equals oracle.code_indices.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from helpers import TOL_SCALE, oracle_job, scale_err, tracking_params_for

f32 = np.float32
HALF_SHIFTS = [-0.5, 0.0, 0.5]
TOL_TRUTH = 1e-6  # |gpu - float64 truth| / sum|x|: the bar of tests/test_tracking_gpu.py (TOL_SCALE_GPU), ten times tighter than helpers.TOL_SCALE
assert TOL_TRUTH <= TOL_SCALE
BIG = 5200  # jobs of a launch that runs the two-wave kernels (mcorr_launch: >= 5 120)

# window length and code step per work-group size: 49 trips of 512 samples / 34 trips of 1 024 samples, both crossing trip 32 inside the run of half-chip trips
# between chip 512 and the end of the code, both inside the staged table (1 022.5 / 1 020 chips)
WINDOWS = {128: (25000, 0.0409), 256: (34000, 0.03)}
REMS = [0.0, 0.125, 0.37, 0.5, 0.73, 0.999, 0.25, 0.9]
OFFSETS = [0, 1, 64, 129, 2, 77, 500, 1001]  # both parities of the window's first sample
RESEED_N = 20000  # one job at 128 threads: 40 trips, exact re-seeds at trips 0, 16 and 32, a partial last trip
STREAM_LEN = 36000


def _streams():
    rng = np.random.default_rng(20817)
    ones = np.ones(STREAM_LEN, np.complex64)
    ints = rng.integers(-7, 8, STREAM_LEN).astype(f32).astype(np.complex64)
    noise = (rng.standard_normal(STREAM_LEN) + 1j * rng.standard_normal(STREAM_LEN)).astype(np.complex64)
    return ones, ints, noise


def _word_jobs(wg, with_carrier):
    n, step = WINDOWS[wg]
    rng = np.random.default_rng(wg)
    jobs = []
    for rem, off in zip(REMS, OFFSETS):
        job = dict(sample_offset=off, n_samples=n, code_slot=0, shifts_chips=HALF_SHIFTS, rem_carr_phase_rad=0.0, phase_step_rad=0.0,
                   rem_code_phase_chips=float(f32(rem)), code_phase_step_chips=float(f32(step)))
        if with_carrier:
            p = tracking_params_for(25e6, float(rng.uniform(-5000, 5000)), rng)
            job.update(rem_carr_phase_rad=p["rem_carr_phase_rad"], phase_step_rad=p["phase_step_rad"])
        jobs.append(job)
    return jobs


def _reseed_job():
    rng = np.random.default_rng(3)
    p = tracking_params_for(25e6, 3217.0, rng)
    return dict(sample_offset=1001, n_samples=RESEED_N, code_slot=0, shifts_chips=HALF_SHIFTS, rem_carr_phase_rad=p["rem_carr_phase_rad"],
                phase_step_rad=p["phase_step_rad"], rem_code_phase_chips=p["rem_code_phase_chips"], code_phase_step_chips=float(f32(0.0409)))


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import oracle
import test_tracking_trip_overheads_gpu as T
from gnss_sdr_amd.tracking import CorrelatorBank
wg = int(sys.argv[2])
b = CorrelatorBank(1, 1023, device=0)
b.set_code(0, oracle.ca_code(7))
ones, ints, noise = T._streams()
out = {{}}
for name, x, carrier in (("ones", ones, False), ("ints", ints, False), ("noise", noise, True)):
    b.set_stream_host(x)
    out[name] = b.correlate(T._word_jobs(wg, carrier))
    if carrier and wg == 128:
        out["reseed"] = b.correlate([T._reseed_job()])
b.close()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def child_outputs(gpu, tmp_path_factory):
    """{(work-group size, body): arrays}: the four child processes run side by side."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    tmp = tmp_path_factory.mktemp("trip_overheads")
    procs = {}
    for wg in (128, 256):
        for body in ("1", "3"):
            f = str(tmp / f"out_{wg}_{body}.npz")
            env = dict(os.environ, GSH_MC_WG=str(wg), GSH_MC_PACKED_BODY=body)
            procs[(wg, body)] = (f, subprocess.Popen([sys.executable, "-c", script, f, str(wg)], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                                     text=True))
    outs = {}
    for key, (f, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (key, log[-3000:])
        outs[key] = dict(np.load(f))
    return outs


def _exact_sums(job, code, xr):
    idx = oracle.code_indices(job["n_samples"], np.asarray(HALF_SHIFTS, f32), job["rem_code_phase_chips"], job["code_phase_step_chips"], 0.0, len(code), False)
    seg = xr[job["sample_offset"]:job["sample_offset"] + job["n_samples"]].astype(np.float64)
    return np.array([(code[idx[t]].astype(np.float64) * seg).sum() for t in range(3)])


@pytest.mark.gpu
@pytest.mark.parametrize("wg", [128, 256])
def test_runs_across_a_mask_word_select_the_reference_chips(child_outputs, wg):
    """Eight E/P/L jobs whose run of half-chip trips crosses trip 32: every sum over x = 1 and over integer weights equals the oracle's (exact chips), and all outputs,
    those over noise with a carrier included, equal the per-tap chains' bit for bit."""
    code = oracle.ca_code(7).astype(np.int32)
    ones, ints, _ = _streams()
    fast, slow = child_outputs[(wg, "1")], child_outputs[(wg, "3")]
    jobs = _word_jobs(wg, False)
    for name, x in (("ones", ones), ("ints", ints)):
        for j, job in enumerate(jobs):
            expect = _exact_sums(job, code, x.real)
            got = fast[name][j, :3]
            print(wg, name, j, got.real, expect)
            assert np.array_equal(got.real.astype(np.float64), expect), (wg, name, job, got, expect)
            assert np.all(got.imag == 0), (wg, name, job, got)
    for name in ("ones", "ints", "noise"):
        assert fast[name].shape == slow[name].shape == (8, 8)
        assert np.all(np.isfinite(fast[name].view(np.float32)))
        assert np.array_equal(fast[name].view(np.uint32), slow[name].view(np.uint32)), (wg, name)


@pytest.mark.gpu
def test_reseed_and_edge_trips_keep_their_sample_numbers(child_outputs):
    """One job of 20 000 samples at 128 threads from an odd sample on (masked first trip, three exact re-seeds, partial last trip): within 1e-6 of the float64 truth and
    bit-identical to the per-tap chains."""
    _, _, noise = _streams()
    job = _reseed_job()
    fast, slow = child_outputs[(128, "1")]["reseed"], child_outputs[(128, "3")]["reseed"]
    _, t64, sabs = oracle_job(oracle.ca_code(7), noise, job)
    err = scale_err(fast[0, :3], t64, sabs)
    print("reseed job: |gpu - truth| / sum|x| =", err)
    assert np.all(err <= TOL_TRUTH), (fast[0, :3], t64, err)
    assert np.array_equal(fast.view(np.uint32), slow.view(np.uint32))


def _random_code(n, seed):
    return (2 * np.random.default_rng(seed).integers(0, 2, n) - 1).astype(f32)


def _image_jobs(lens, rng, n=8000):
    jobs = []
    for i in range(4 * len(lens)):
        slot = i % len(lens)
        p = tracking_params_for(25e6, float(rng.uniform(-5000, 5000)), rng)
        step = min(p["code_phase_step_chips"], float(f32((lens[slot] - 2) / n)))  # the window stays inside one period of the slot's code
        jobs.append(dict(sample_offset=int(rng.integers(0, 2000)), n_samples=n, code_slot=slot, shifts_chips=HALF_SHIFTS, **dict(p, code_phase_step_chips=step)))
    return jobs


def _check_against_truth(out, jobs, codes, x):
    worst = 0.0
    for j, job in enumerate(jobs):
        _, t64, sabs = oracle_job(codes[job["code_slot"]], x, job)
        err = scale_err(out[j, :3], t64, sabs)
        assert np.all(err <= TOL_TRUTH), (j, job, out[j, :3], t64, err)
        worst = max(worst, float(err.max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [[511, 1023, 1024], [2046, 2046]], ids=["half-chip", "falls-back"])
def test_staged_image_follows_set_code(gpu, lens):
    """Codes of 511, 1 023 and 1 024 chips take the half-chip form (tables copied from the image of gsh_bank_set_code); a bank of 2 046-chip codes has no image and falls
    back.  Launch, replace ONE slot's code, launch again: both results are within 1e-6 of the float64 truth for the codes then set, the other slots' outputs do not
    change by a bit and the replaced slot's do -- in a launch of the four-wave kernels and in one of 5 200 jobs (two-wave kernels)."""
    from gnss_sdr_amd.tracking import CorrelatorBank
    rng = np.random.default_rng(len(lens))
    x = (rng.standard_normal(12000) + 1j * rng.standard_normal(12000)).astype(np.complex64)
    codes = [_random_code(n, 10 + i) for i, n in enumerate(lens)]
    jobs = _image_jobs(lens, rng)
    many = (jobs * (BIG // len(jobs) + 1))[:BIG]
    b = CorrelatorBank(len(lens), max(lens), device=gpu)
    for i, c in enumerate(codes):
        b.set_code(i, c)
    b.set_stream_host(x)
    first, first_big = b.correlate(jobs), b.correlate(many)
    changed = 1
    codes2 = list(codes)
    codes2[changed] = _random_code(lens[changed], 99)
    b.set_code(changed, codes2[changed])
    second, second_big = b.correlate(jobs), b.correlate(many)
    b.close()
    print("worst |gpu - truth| / sum|x|:", _check_against_truth(first, jobs, codes, x), _check_against_truth(second, jobs, codes2, x))
    _check_against_truth(first_big[:len(jobs)], jobs, codes, x)
    _check_against_truth(second_big[:len(jobs)], jobs, codes2, x)
    for a, c in ((first, second), (first_big, second_big)):
        for j in range(len(a)):
            same = np.array_equal(a[j].view(np.uint32), c[j].view(np.uint32))
            assert same == (many[j]["code_slot"] != changed), (j, many[j]["code_slot"], a[j], c[j])
    reps = BIG // len(jobs)
    assert np.array_equal(second_big[:reps * len(jobs)].view(np.uint32), np.tile(second_big[:len(jobs)], (reps, 1)).view(np.uint32))
