"""Two half-chip trips per pass of the run loop (csrc/mcorr_device.h run_segment_packed, GSH_MC_TRIP_PAIRS, round 9).

At 128 threads a run of half-chip trips takes its trips two at a time while both lie in the run, no exact re-seed falls on the second one and the trip whose loads
the second one issues is still a plain one; everything else goes through the single-trip loop as before.  That changes no product and no order of a sum, so every
output must equal the per-tap chains' (GSH_MC_PACKED_BODY=3) bit for bit at the same work-group size, the chips must be the reference's, and the sums must stay
within 1e-6 of the float64 truth.  The jobs also hold the trips around the pairs: trips in which one chunk of a wave fails the judgement (the crossings of 64, 128 and
256 chips in either chunk, for either wave), per-tap trips of a 2 046-chip code inside and beyond chip 2 040, and a code phase whose scaled constant would be denormal.

Method of tests/test_tracking_trip_overheads_gpu.py: GSH_MC_WG and GSH_MC_PACKED_BODY are read once per process, so the kernels run in four child processes started
together; carrier-free integer-valued input makes every float32 sum exact, so a tap's output equals the oracle's sum iff every chip index is oracle.code_indices'.

The shapes are the smallest that reach every way through the loop; `loop_plan` restates the kernel's judgement and loop in numpy float32 and the first test (no GPU)
asserts that the parameters below really produce the cases they are named for.  Every job is one segment (set_splits(1)), so a window is a run of trips of 4 x 128
(or 4 x 256) samples from the even sample at or before its first one.
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
TOL_TRUTH = 1e-6  # |gpu - float64 truth| / sum|x|: the bar of tests/test_tracking_gpu.py, ten times tighter than helpers.TOL_SCALE
assert TOL_TRUTH <= TOL_SCALE
RESEED = 16       # trips between exact re-seeds at two chunks per trip (mcorr_device.h packed_reseed_trips)
STEP = 0.0409     # chips per sample of GPS L1 C/A at 25 Msps
STREAM_LEN = 25200


def _job(n, off, rem, step=STEP, slot=0):
    return dict(sample_offset=off, n_samples=n, code_slot=slot, shifts_chips=HALF_SHIFTS, rem_carr_phase_rad=0.0, phase_step_rad=0.0,
                rem_code_phase_chips=float(f32(rem)), code_phase_step_chips=float(f32(step)))


# windows of 512 k + r samples from an even and from an odd sample: runs of 0 ... 4 plain trips behind the trips that hold the crossings below chip 32
WINDOW_JOBS = [_job(512 * k + r, off, 0.37) for k in (1, 2, 3, 4, 5) for r in (0, 1, 300) for off in (0, 1)]
# a window that starts at chip 520: beyond the crossing of step * n at 256 (trip 12) ONE run of half-chip trips, trips 13 ... 23, up to chip 1 020
LONG_RUN_JOBS = [_job(12500, 0, -520.25), _job(12500, 1, -520.25)]
# 20 000 samples (40 trips, exact re-seeds at trips 0, 16 and 32) at two code phases: the runs start at other trips, so a re-seed meets the first trip of a pair in one
# wave and would meet the second one in another (that pair is not formed)
RESEED_JOBS = [_job(20000, 1001, 0.37, 0.02), _job(20000, 1001, -300.25, 0.02), _job(20000, 64, -300.25, 0.02)]
# crossings of 64, 128 and 256 chips in chunk A and in chunk B of a trip, for wave 0 and for wave 1 (found by a search over the step; asserted below)
MIXED_JOBS = [_job(7000, 0, 0.25, s) for s in (0.0418, 0.0454, 0.0526)]
# a scaled constant that would be denormal: no trip may take the two-floors form
TINY_REM_JOBS = [_job(3000, 0, 1e-33), _job(3000, 1, 1e-33)]
JOBS_1023 = WINDOW_JOBS + LONG_RUN_JOBS + RESEED_JOBS + MIXED_JOBS + TINY_REM_JOBS
# a 2 046-chip code (paired taps, not the half-chip form): its per-tap trips lie inside [1, 2 040) and, at the window's end, beyond it
JOBS_2046 = [_job(25092, 0, 0.37, 0.0818), _job(25091, 1, 0.625, 0.0818)]  # (49 plain trips: the last one reaches chip 2 052)


def geometry(job, wg):
    """(odd, n_trips, first_plain, last_plain) of a one-segment job at wg threads, as run_segment_packed forms them."""
    odd = job["sample_offset"] & 1
    span = job["n_samples"] + odd
    n_pairs, n_full = (span + 1) >> 1, span >> 1
    return odd, -(-n_pairs // (2 * wg)), odd, n_full // (2 * wg)


def verdicts(job, wg, hi=1020.0):
    """bool [waves, chunks]: the judgement of run_segment_packed (judge) for every wave and chunk of 2 wg samples, in float32 with its own expressions."""
    odd, n_trips, _, _ = geometry(job, wg)
    step, rem = f32(job["code_phase_step_chips"]), f32(job["rem_code_phase_chips"])
    sh = np.asarray(job["shifts_chips"], f32)
    scaled_ok = all(v == 0 or abs(v) >= f32(2.0) ** -100 for v in (step, rem, sh[1], sh[2]))
    waves, chunks = wg // 64, 2 * n_trips
    n_lo = (-odd + 2 * wg * np.arange(chunks)[None, :] + 128 * np.arange(waves)[:, None]).astype(f32)
    lo1 = (step * n_lo).astype(f32) + f32(sh[0] - f32(0.125))
    hi1 = (step * (n_lo + f32(127.0))).astype(f32) + f32(sh[2] + f32(0.125))
    lo2, hi2 = (lo1 - rem).astype(f32), (hi1 - rem).astype(f32)
    assert lo1.dtype == hi1.dtype == lo2.dtype == np.float32

    def one_binade(lo, up):
        return (lo >= 1.0) & (up < f32(hi)) & ((lo.view(np.uint32) >> 23) == (up.view(np.uint32) >> 23))
    ok = one_binade(lo1, hi1) & one_binade(lo2, hi2) & scaled_ok
    ok[:, 128:] = False  # two mask words of 64 chunks
    return ok


def loop_plan(job, wg, wave, hi=1020.0):
    """The form every trip of one wave takes, as the run loop decides it: 'T' per-tap (edge trips included), 'A' / 'B' per-tap although chunk A / B alone passed the
    judgement, 'H' a half-chip trip on its own, 'P' / 'Q' the first / second half-chip trip of a pair (128 threads only); and the trips that re-seed."""
    _, n_trips, first_plain, last_plain = geometry(job, wg)
    ok = verdicts(job, wg, hi)[wave]
    plain = [first_plain <= i < last_plain for i in range(n_trips)]
    fast = [plain[i] and ok[2 * i] and ok[2 * i + 1] for i in range(n_trips)]

    def paired_run(i):
        if not (first_plain <= i < last_plain) or 2 * i >= 128:
            return 0
        run, word_end = 0, (64 - (2 * i & 63)) // 2
        while run < word_end and i + run < last_plain and fast[i + run]:
            run += 1
        return run
    form, reseeds, until = [None] * n_trips, [], 0

    def trip(i, f, second=False):
        nonlocal until
        if until == 0:
            assert not second, "a re-seed on the second trip of a pair"
            reseeds.append(i)
            until = RESEED
        until -= 1
        form[i] = f
    i = 0
    while i < n_trips:
        run = paired_run(i)
        while run > 0:
            pairs = min(run, last_plain - 1 - i) >> 1 if wg == 128 else 0
            if until & 1:
                pairs = min(pairs, until >> 1)
            if pairs > 0:
                run -= 2 * pairs
                for _ in range(pairs):
                    assert fast[i] and fast[i + 1] and i + 2 < last_plain
                    trip(i, "P")
                    trip(i + 1, "Q", second=True)
                    i += 2
            else:
                trip(i, "H")
                i += 1
                run -= 1
            if run == 0:
                run = paired_run(i)
        if i >= n_trips:
            break
        trip(i, "T" if not plain[i] or ok[2 * i] == ok[2 * i + 1] else ("A" if ok[2 * i] else "B"))
        i += 1
    return "".join(form), reseeds


def _runs(plan):
    """lengths of the runs of half-chip trips of a plan"""
    return [len(r) for r in "".join(c if c in "HPQ" else " " for c in plan).split()]


def test_the_parameters_produce_the_cases():
    """No GPU: the loop's own decisions, restated in numpy float32, for the jobs above at 128 threads (and the geometry at 256)."""
    plans = {(j, w): loop_plan(job, 128, w) for j, job in enumerate(JOBS_1023) for w in (0, 1)}
    nW, nL, nR, nM = len(WINDOW_JOBS), len(LONG_RUN_JOBS), len(RESEED_JOBS), len(MIXED_JOBS)
    for key, (plan, reseeds) in plans.items():
        job = JOBS_1023[key[0]]
        _, n_trips, first_plain, last_plain = geometry(job, 128)
        assert len(plan) == n_trips and reseeds == list(range(0, n_trips, RESEED)), (key, plan, reseeds)
        assert plan.count("P") == plan.count("Q") and "PP" not in plan and all(plan[i + 1] == "Q" for i, c in enumerate(plan) if c == "P"), (key, plan)
        # the trip whose loads a pair's second trip issues is a plain one
        assert all(i + 1 < last_plain for i, c in enumerate(plan) if c == "Q"), (key, plan)
        print(key, job["n_samples"], job["sample_offset"] & 1, plan)
    # windows: runs of 0, 1, 2 and 3 plain trips (and longer), single trips, pairs; a pair that ends at the last trip a pair may hold, and a run whose last plain trips
    # stay single because the trip behind them is the masked tail
    window_plans = [plans[(j, w)][0] for j in range(nW) for w in (0, 1)]
    lengths = {n for p in window_plans for n in _runs(p)} | {0 for p in window_plans if not _runs(p)}
    assert {0, 1, 2, 3} <= lengths, lengths
    assert any("Q" in p for p in window_plans) and any("H" in p for p in window_plans)
    assert any(p.rfind("Q") == geometry(WINDOW_JOBS[j], 128)[3] - 2 for j in range(nW) for p in (plans[(j, 0)][0], plans[(j, 1)][0]))
    assert any(p.rstrip("T").endswith("QH") for p in window_plans)
    assert {job["sample_offset"] & 1 for job in WINDOW_JOBS} == {0, 1}
    # one long run from an odd trip on, beyond chip 520
    for j in range(nW, nW + nL):
        for w in (0, 1):
            plan = plans[(j, w)][0]
            marked = "".join(c if c in "HPQ" else " " for c in plan)
            longest = max(marked.split(), key=len)
            start = marked.index(longest)
            assert len(longest) >= 10 and start % 2 == 1 and longest.startswith("PQ"), (j, w, plan)
    # re-seeds: at the first trip of a pair, and where one would fall on a second trip the trip before it stays single
    reseed_plans = [plans[(j, w)][0] for j in range(nW + nL, nW + nL + nR) for w in (0, 1)]
    assert any(p[r] == "P" for p in reseed_plans for r in (16, 32)), reseed_plans
    assert any(p[r - 1] == "H" and p[r - 2] in "HQ" and p[r] in "PH" for p in reseed_plans for r in (16, 32)), reseed_plans
    # crossings at 64, 128 and 256 chips: one chunk of a trip fails, for each wave once chunk A and once chunk B
    seen = set()
    for j in range(nW + nL + nR, nW + nL + nR + nM):
        job = JOBS_1023[j]
        for w in (0, 1):
            for i, c in enumerate(plans[(j, w)][0]):
                if c in "AB":
                    chips = float(job["code_phase_step_chips"]) * (512 * i + 256 * (c == "A") + 128 * w + 64)  # the middle of the failing wave-chunk
                    seen.add((min((64, 128, 256), key=lambda p: abs(chips - p)), w, "B" if c == "A" else "A"))
    print(sorted(seen))
    assert seen == {(p, w, c) for p in (64, 128, 256) for w in (0, 1) for c in "AB"}, sorted(seen)
    # the denormal scaled constant: per-tap trips only
    for j in range(nW + nL + nR + nM, len(JOBS_1023)):
        assert set(plans[(j, 0)][0]) == set(plans[(j, 1)][0]) == {"T"}
    # the 2 046-chip code (paired taps, judged up to 2 040): per-tap trips inside [1, 2 040) -- the crossings -- and beyond it
    for job in JOBS_2046:
        ok = verdicts(job, 128, hi=2040.0)
        _, n_trips, first_plain, last_plain = geometry(job, 128)
        step = float(job["code_phase_step_chips"])
        slow = [i for i in range(first_plain, last_plain) if not ok[:, 2 * i:2 * i + 2].all()]
        assert any(1.0 < step * 512 * i and step * 512 * (i + 1) < 2040.0 for i in slow) and any(step * 512 * (i + 1) > 2040.0 for i in slow), slow
        assert ok.any()
    # 256 threads: the same jobs run, one trip per pass
    assert all(set(loop_plan(job, 256, w)[0]) <= set("TABH") for job in JOBS_1023 for w in range(4))


def _streams():
    rng = np.random.default_rng(90210)
    ones = np.ones(STREAM_LEN, np.complex64)
    ints = rng.integers(-7, 8, STREAM_LEN).astype(f32).astype(np.complex64)
    noise = (rng.standard_normal(STREAM_LEN) + 1j * rng.standard_normal(STREAM_LEN)).astype(np.complex64)
    return ones, ints, noise


def _codes():
    return oracle.ca_code(7).astype(f32), (2 * np.random.default_rng(2046).integers(0, 2, 2046) - 1).astype(f32)


def _with_carrier(jobs):
    rng = np.random.default_rng(len(jobs))
    out = []
    for job in jobs:
        p = tracking_params_for(25e6, float(rng.uniform(-5000, 5000)), rng)
        out.append(dict(job, rem_carr_phase_rad=p["rem_carr_phase_rad"], phase_step_rad=p["phase_step_rad"]))
    return out


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_tracking_trip_pairs_gpu as T
from gnss_sdr_amd.tracking import CorrelatorBank
out = {{}}
for tag, code, jobs in zip(("a", "b"), T._codes(), (T.JOBS_1023, T.JOBS_2046)):
    b = CorrelatorBank(1, len(code), device=0)
    b.set_code(0, code)
    b.set_splits(1)
    for name, x, carrier in zip(("ones", "ints", "noise"), T._streams(), (False, False, True)):
        b.set_stream_host(x)
        out[tag + "_" + name] = b.correlate(T._with_carrier(jobs) if carrier else jobs)
    b.close()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def child_outputs(gpu, tmp_path_factory):
    """{(work-group size, body): arrays}: the four child processes run side by side."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    tmp = tmp_path_factory.mktemp("trip_pairs")
    procs = {}
    for wg in (128, 256):
        for body in ("1", "3"):
            f = str(tmp / f"out_{wg}_{body}.npz")
            env = dict(os.environ, GSH_MC_WG=str(wg), GSH_MC_PACKED_BODY=body)
            procs[(wg, body)] = (f, subprocess.Popen([sys.executable, "-c", script, f], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
def test_every_job_selects_the_reference_chips_and_equals_the_per_tap_chains(child_outputs, wg):
    """Every job above: the sums over x = 1 and over integer weights equal the oracle's (exact chips); all outputs, those over noise with a carrier included, equal the
    per-tap chains' bit for bit; the sums over noise lie within 1e-6 of the float64 truth."""
    ones, ints, noise = _streams()
    fast, slow = child_outputs[(wg, "1")], child_outputs[(wg, "3")]
    worst = 0.0
    for tag, code, jobs in zip(("a", "b"), _codes(), (JOBS_1023, JOBS_2046)):
        for name, x in (("ones", ones), ("ints", ints)):
            for j, job in enumerate(jobs):
                expect = _exact_sums(job, code.astype(np.int32), x.real)
                got = fast[tag + "_" + name][j, :3]
                assert np.array_equal(got.real.astype(np.float64), expect), (wg, tag, name, j, job, got, expect)
                assert np.all(got.imag == 0), (wg, tag, name, j, job, got)
        for name in ("ones", "ints", "noise"):
            a, b = fast[tag + "_" + name], slow[tag + "_" + name]
            assert a.shape == b.shape == (len(jobs), 8)
            assert np.all(np.isfinite(a.view(np.float32)))
            differ = [j for j in range(len(jobs)) if not np.array_equal(a[j].view(np.uint32), b[j].view(np.uint32))]
            assert not differ, (wg, tag, name, differ)
        for j, job in enumerate(_with_carrier(jobs)):
            _, t64, sabs = oracle_job(code, noise, job)
            err = scale_err(fast[tag + "_noise"][j, :3], t64, sabs)
            worst = max(worst, float(err.max()))
            assert np.all(err <= TOL_TRUTH), (wg, tag, j, job, err)
    print(wg, "worst |gpu - truth| / sum|x| =", worst)
