"""One anchor per lane for the half-chip trips' sample numbers (csrc/mcorr_device.h run_segment_packed, GSH_MC_ANCHOR_FMA, round 13).  No GPU: numpy float32.

A half-chip trip evaluates w = fl(fl(step' (float)n) - rem') for four pairs of samples n, n + 2 PPC, n + TRIP, n + TRIP + 2 PPC of a pass of two trips (step', rem':
the constants times 2^-23).  The kernel keeps (float)n of the first of them only and forms the other products as fma(step', (float)n, step' K): for K a power of two
step' K is exact, the FMA rounds the real number step' (n + K) once, and that is the product fl(step' (float)(n + K)) bit for bit.  Here:
  * the identity for every constant the kernels use, at 128 and at 256 threads;
  * its failure for K = 3 * 2 PPC -- why the fourth pair is reached as (n + 2 TRIP) - 2 PPC, behind the anchor's one step per pass;
  * the guard that keeps a segment whose constants are not normal, finite numbers on the per-tap chains;
  * the pass itself, restated with one anchor per lane and driven by the run loop's own decisions (tests/test_tracking_trip_pairs_gpu.py loop_plan), against the
    per-sample chain, window by window and sample by sample; and that the windows reach every way through the loop.
An FMA in numpy: the product of two float32 is exact in float64, and so is its sum with step' K here (the sum is step' (n + K), 24 x 25 significant bits), so one
conversion to float32 is the single rounding.  The jobs below are the ones tests/test_tracking_anchor_fma_gpu.py runs on the device.
"""
import numpy as np
import pytest

from helpers import GPS_CA_CHIP_RATE, GPS_L1_FREQ_HZ
from test_tracking_trip_pairs_gpu import RESEED, geometry, loop_plan

f32, f64 = np.float32, np.float64
PK_SCALE = f32(2.0 ** -23)
HALF_SHIFTS = [-0.5, 0.0, 0.5]
WINDOWS = [512, 513, 1023, 1024, 1025, 1536, 2047, 2048, 2049, 3072, 8229, 16387, 25000, 33001]
RATES = [4e6, 10e6, 25e6, 50e6]
CODE_PHASES = [0.0, 1e-30, 0.37, 0.999]
STREAM_LEN = 33001 + 1 + 2  # the longest window from an odd sample ends on the last but one sample; END_JOBS end on the last


def ca_step(fs, doppler_hz):
    return f32(GPS_CA_CHIP_RATE * (1.0 + doppler_hz / GPS_L1_FREQ_HZ) / fs)


def _job(n, off, rem, step, rem_carr=0.0, phase_step=0.0):
    return dict(sample_offset=int(off), n_samples=int(n), code_slot=0, shifts_chips=list(HALF_SHIFTS), rem_carr_phase_rad=float(f32(rem_carr)),
                phase_step_rad=float(f32(phase_step)), rem_code_phase_chips=float(f32(rem)), code_phase_step_chips=float(f32(step)))


def _grid():
    """every window from an even and from an odd sample at every rate, Doppler +-5 kHz and the code phases in turn; at 25 and 50 Msps every code phase"""
    jobs, k = [], 0
    for fs in RATES:
        for n in WINDOWS:
            for off in (0, 1):
                phases = CODE_PHASES if fs >= 25e6 else [CODE_PHASES[k % 4]]
                for rem in phases:
                    dop = 5000.0 if k % 2 else -5000.0
                    jobs.append(_job(n, off, rem, ca_step(fs, dop), rem_carr=0.1 * (k % 60), phase_step=2.0 * np.pi * dop / fs))
                    k += 1
    return jobs


GRID_JOBS = _grid()
# the short windows again from chip 520 on (a negative code phase, as tests/test_tracking_trip_pairs_gpu.py LONG_RUN_JOBS): their two to six trips are half-chip
# trips, alone and in pairs, where a window that starts at chip 0 spends them on the crossings of 1 ... 32 chips
FAR_JOBS = [_job(n, off, -520.25 - 0.37 * off, ca_step(25e6, 1234.0)) for n in WINDOWS[:10] for off in (0, 1)]
# the window that ends on the stream's last sample (the longest and a short one)
END_JOBS = [_job(n, STREAM_LEN - n, 0.37, ca_step(fs, -2500.0)) for n, fs in ((33001, 50e6), (25000, 25e6), (2049, 25e6), (1025, 50e6))]
# a code phase whose scaled value would be denormal: the guard keeps every trip on the per-tap chains
TINY_JOBS = [_job(3072, off, 1e-33, ca_step(25e6, 0.0)) for off in (0, 1)]
JOBS = GRID_JOBS + FAR_JOBS + END_JOBS + TINY_JOBS


def fma32(a, b, c):
    """fl(a * b + c) with one rounding; valid where a * b + c is exact in float64 (asserted by the callers' construction: see the module's docstring)"""
    return (a.astype(f64) * b.astype(f64) + np.asarray(c, f64)).astype(f32)


def anchor_constants(step, wg):
    """(C_chunk, C_trip, step' 2 TRIP) as run_segment_packed forms them: one float32 product of the step each"""
    ppc, trip = wg, 4 * wg
    return tuple(f32(step) * f32(PK_SCALE * f32(k)) for k in (2 * ppc, trip, 2 * trip))


def scaled_ok(step, rem, sh=HALF_SHIFTS, wg=128):
    """the kernel's guard: nothing scaled is denormal (rounds 6 - 12), and the anchor's three constants are normal, finite numbers (round 13)"""
    with np.errstate(over="ignore", invalid="ignore"):
        scales = all(f32(v) == 0 or abs(f32(v)) >= f32(2.0 ** -100) for v in (step, rem, sh[1], sh[2]))
        normal = all(abs(c) >= f32(2.0 ** -126) and abs(c) < f32(np.inf) for c in anchor_constants(step, wg))
    return bool(scales and normal)


def _steps_and_numbers(count, seed):
    rng = np.random.default_rng(seed)
    fs = rng.uniform(2e6, 50e6, count // 2)
    dop = rng.uniform(-10e3, 10e3, count // 2)
    steps = np.concatenate([(GPS_CA_CHIP_RATE * (1.0 + dop / GPS_L1_FREQ_HZ) / fs), rng.uniform(1e-3, 1.2, count - count // 2)]).astype(f32)
    return steps, rng.integers(0, 1 << 24, count)


@pytest.mark.parametrize("wg", [128, 256])
def test_fma_from_the_anchor_is_the_product_for_the_kernels_constants(wg):
    steps, n = _steps_and_numbers(1 << 20, wg)
    sp = steps * PK_SCALE
    assert sp.dtype == np.float32 and np.array_equal(sp.astype(f64) * 2.0 ** 23, steps.astype(f64))
    for K in (2 * wg, 4 * wg, -2 * wg, 8 * wg):
        m = np.clip(n, max(0, -K), (1 << 24) - 1 - max(0, K))  # m and m + K both in [0, 2^24)
        C = sp * f32(K)
        assert np.array_equal(C.astype(f64), sp.astype(f64) * K)  # exact
        got = fma32(m.astype(f32), sp, C)
        want = sp * (m + K).astype(f32)
        assert want.dtype == np.float32
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (wg, K, bad[:5], steps[bad[:5]], m[bad[:5]])


@pytest.mark.parametrize("wg", [128, 256])
def test_three_chunks_ahead_is_no_single_fma(wg):
    """K = 3 * 2 PPC: step' K is rounded when it is formed, and the FMA then misses the product for some (step, n) -- the order of the pass exists for this"""
    steps, n = _steps_and_numbers(1 << 20, 7 + wg)
    sp = steps * PK_SCALE
    K = 6 * wg
    m = np.minimum(n, (1 << 24) - 1 - K)
    C = sp * f32(K)
    got = fma32(m.astype(f32), sp, C)
    want = sp * (m + K).astype(f32)
    assert np.count_nonzero(got != want) > 0


def test_the_guard_rejects_constants_that_are_not_normal():
    for wg in (128, 256):
        for step in (0.0409, 1e-3, 1.2, float(ca_step(2e6, 1e4)), 2.0 ** -100):
            assert scaled_ok(step, 0.37, wg=wg) and scaled_ok(step, 0.0, wg=wg), step
            c = anchor_constants(step, wg)
            assert all(np.isfinite(v) and abs(v) >= np.finfo(f32).tiny for v in c)
            assert c[0].astype(f64) == f64(f32(step)) * 2.0 ** -23 * 2 * wg
        # a step whose scaled value (or a constant of it) is denormal or zero, or not finite: the per-tap chains
        for step in (0.0, 2.0 ** -101, 1e-38, 2.0 ** -149, float("inf"), float("nan")):
            assert not scaled_ok(step, 0.37, wg=wg), step
        assert not scaled_ok(0.0409, 1e-33, wg=wg) and not scaled_ok(0.0409, 2.0 ** -120, wg=wg)
        assert scaled_ok(0.0409, 1e-30, wg=wg)  # (the smallest code phase of the grid still scales exactly: its windows run half-chip trips)


def anchored_chains(job, wave, wg=128):
    """w' = chain value times 2^-23 of every half-chip trip of one wave of a one-segment job, float32 [trip, chunk, lane, sample of the pair], as the kernel forms
    them from ONE anchor per lane; NaN rows for the other trips.  Also the plan and the anchor's history (for the coverage assertions)."""
    odd, n_trips, first_plain, last_plain = geometry(job, wg)
    plan, reseeds = loop_plan(job, wg, wave)
    step, rem = f32(job["code_phase_step_chips"]), f32(job["rem_code_phase_chips"])
    sp, nrem = step * PK_SCALE, -rem * PK_SCALE
    c_chunk, c_trip, _ = anchor_constants(step, wg)
    ppc, trip = wg, 4 * wg
    n_first = job["sample_offset"] - odd
    lanes = 64 * wave + np.arange(64)
    out = np.full((n_trips, 2, 64, 2), np.nan, f32)
    anchor, until, events = None, 0, []
    for i, form in enumerate(plan):
        if form != "Q" and until == 0:  # exact re-seed, on first trips only: resets the anchor
            assert i in reseeds
            n0 = n_first + i * trip + 2 * lanes
            anchor = np.stack([n0, n0 + 1], -1).astype(f32)
            until = RESEED
            events.append(("seed", i, form))
        else:
            assert i not in reseeds
        until -= 1
        if form in "HP":
            prod_a = anchor * sp
            prod_b = fma32(anchor, np.broadcast_to(sp, anchor.shape), c_chunk)
            if form == "H":
                anchor = anchor + f32(trip)
        elif form == "Q":
            prod_a = fma32(anchor, np.broadcast_to(sp, anchor.shape), c_trip)
            anchor = anchor + f32(2 * trip)  # the pass' one step
            prod_b = fma32(anchor, np.broadcast_to(sp, anchor.shape), -c_chunk)
        else:
            # a per-tap or an edge trip: chunk B's number is the anchor's plus 2 PPC, formed where it is used (exact); the anchor steps by one trip
            assert np.array_equal((anchor + f32(2 * ppc)).astype(f64), anchor.astype(f64) + 2 * ppc)
            anchor = anchor + f32(trip)
            continue
        assert prod_a.dtype == prod_b.dtype == anchor.dtype == np.float32
        out[i, 0], out[i, 1] = prod_a + nrem, prod_b + nrem
    return out, plan, events


def per_sample_chains(job, wave, wg=128):
    """fl(fl(step (float)n) - rem) of the same samples: the chain the reference evaluates per sample"""
    odd, n_trips, _, _ = geometry(job, wg)
    step, rem = f32(job["code_phase_step_chips"]), f32(job["rem_code_phase_chips"])
    n = (job["sample_offset"] - odd + 4 * wg * np.arange(n_trips)[:, None, None, None] + 2 * wg * np.arange(2)[None, :, None, None]
         + 2 * (64 * wave + np.arange(64))[None, None, :, None] + np.arange(2)[None, None, None, :])
    assert n.max() < 1 << 24
    w = step * n.astype(f32) - rem
    assert w.dtype == np.float32
    return w


def in_table(job):
    """the window's chips stay inside the staged whole code (1 023 chips): the job runs the trips loop_plan describes"""
    end = float(job["code_phase_step_chips"]) * (job["n_samples"] + 1) - float(job["rem_code_phase_chips"]) + 0.5
    return end < 1023.0


def test_one_anchor_per_lane_reproduces_the_per_sample_chain():
    """Every half-chip trip of every job and wave: the anchored pass gives fl(fl(step n) - rem) for each of its 512 samples, bit for bit (times 2^-23, exactly)."""
    checked = 0
    for job in JOBS:
        if not scaled_ok(job["code_phase_step_chips"], job["rem_code_phase_chips"]):
            assert set(loop_plan(job, 128, 0)[0]) <= {"T"}
            continue
        for wave in (0, 1):
            got, plan, _ = anchored_chains(job, wave)
            want = per_sample_chains(job, wave)
            half = np.array([c in "HPQ" for c in plan])
            assert not np.isnan(got[half]).any() and np.isnan(got[~half]).all()
            scaled_back = got[half].astype(f64) * 2.0 ** 23
            assert np.array_equal(scaled_back.astype(f32).astype(f64), scaled_back)  # a power of two: exact
            differ = np.argwhere(scaled_back.astype(f32).view(np.uint32) != want[half].view(np.uint32))
            assert differ.size == 0, (job, wave, plan, differ[:4])
            checked += int(half.sum())
    assert checked > 2000, checked


def test_the_windows_reach_every_way_through_the_loop():
    """a pass of the loop, the peeled last pass, a single half-chip trip, per-tap trips between them, a re-seed on the first trip of a pair inside a run, and runs
    of pairs that start with an even and with an odd count of trips left to the re-seed (an odd one ends the pairs one trip before it)"""
    seen = set()
    for job in JOBS:
        if not in_table(job) or not scaled_ok(job["code_phase_step_chips"], job["rem_code_phase_chips"]):
            continue
        for wave in (0, 1):
            _, plan, events = anchored_chains(job, wave)
            _, n_trips, first_plain, last_plain = geometry(job, 128)
            if "PQPQ" in plan:
                seen.add("pass")
            if "Q" in plan:
                seen.add("peeled last pass")
            if "H" in plan:
                seen.add("single trip")
            if "QH" in plan:
                seen.add("single trip behind a pair")
            if "T" in plan.strip("T").replace("H", "").replace("PQ", "") or "TP" in plan or "TH" in plan:
                seen.add("per-tap trip in front of half-chip trips")
            for kind, i, form in events:
                if i > 0 and form == "P" and plan[i - 1] in "QH":
                    seen.add("re-seed inside a run, on a pair's first trip")
                if i > 0 and form == "H":
                    seen.add("re-seed on a single trip")
            for i, c in enumerate(plan):
                if c == "P" and (i == 0 or plan[i - 1] != "Q"):
                    left = (RESEED - i % RESEED) % RESEED  # trips left to the re-seed when the pairs start (re-seeds fall on multiples of RESEED)
                    seen.add("pairs start with %s trips left" % ("an odd count of" if left & 1 else "an even count of"))
                if c == "H" and i + 1 < n_trips and plan[i + 1] == "P" and (i + 1) % RESEED == 0:
                    seen.add("pairs end one trip before the re-seed")
            if n_trips > 64:
                assert set(plan[64:]) == {"T"}
                seen.add("trips beyond the judgement's two mask words")
    want = {"pass", "peeled last pass", "single trip", "single trip behind a pair", "per-tap trip in front of half-chip trips",
            "re-seed inside a run, on a pair's first trip", "pairs start with an odd count of trips left", "pairs start with an even count of trips left",
            "pairs end one trip before the re-seed", "trips beyond the judgement's two mask words"}
    print(sorted(seen))
    assert want <= seen, sorted(want - seen)
    # the parameters of the issue: every window with both parities, every rate, every code phase
    assert {(j["n_samples"], j["sample_offset"] & 1) for j in GRID_JOBS} == {(n, p) for n in WINDOWS for p in (0, 1)}
    assert {f32(j["rem_code_phase_chips"]) for j in GRID_JOBS} == {f32(r) for r in CODE_PHASES}
    assert 150 <= len(JOBS) <= 500
    assert max(j["sample_offset"] + j["n_samples"] for j in JOBS) == STREAM_LEN and any(j["sample_offset"] + j["n_samples"] == STREAM_LEN for j in END_JOBS)
