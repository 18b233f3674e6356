"""Two trips of sample loads in flight inside a run of trip pairs (csrc/mcorr_device.h run_segment_packed, GSH_MC_PAIR_QUEUE, round 10).

At 128 threads a run of half-chip trip pairs keeps a second set of sample registers: the run starts with one more pair of loads (its second trip's), every trip of
a pass then issues the loads of the trip TWO ahead into the registers it has just rotated out of, and the run's last pass is peeled -- its first trip issues the loads
of the trip behind the run, its second trip none -- so that outside the run the queue is one trip deep as before.  No product and no order of a sum changes, so every
output must equal the per-tap chains' (GSH_MC_PACKED_BODY=3) bit for bit, the chips must be the reference's, and the sums must stay within 1e-6 of the float64 truth.

Method and helpers of tests/test_tracking_trip_pairs_gpu.py (geometry, the judgement in numpy float32, the streams, the exact sums): the kernels run in two child
processes at 128 threads (GSH_MC_WG, GSH_MC_PACKED_BODY are read once per process); carrier-free integer-valued input makes every float32 sum exact, so a tap's
output equals the oracle's sum iff every chip index is oracle.code_indices'.

`queue_plan` restates the run loop AND its load queue: which trip issues whose loads, in which form.  The first test (no GPU) asserts on it that the loads of every
trip go out exactly once, the plain (unmasked, 16-byte) form only for plain trips, that a trip outside a run of pairs finds exactly its own loads in flight -- so the
set of addresses a job reads is the one-deep queue's -- and that the windows below really drive every way through the loop.  The windows are 2 to 12 trips long
(1 024 to 6 144 samples, and odd lengths); what cannot happen in twelve trips has a longer window of its own: an exact re-seed comes every 16 trips, a word of the
judgement mask ends every 32.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_tracking_trip_pairs_gpu as pairs
from helpers import TOL_SCALE, oracle_job, scale_err

f32 = np.float32
TOL_TRUTH = 1e-6  # |gpu - float64 truth| / sum|x|
assert TOL_TRUTH <= TOL_SCALE
RESEED = pairs.RESEED
STEP = pairs.STEP
STREAM_LEN = pairs.STREAM_LEN
WG = 128
TRIP = 4 * WG  # samples of a trip

_job = pairs._job
# 512 k + r samples from an even and from an odd sample, k = 2 ... 12, at 0.0409 chips per sample: the crossings of 32, 64, 128 and 256 chips fall into trips 1, 3, 6
# and 12, all of them into the half of a chunk that wave 0 holds.  Wave 1 so has ONE run of half-chip trips from trip 1 to the window's last plain trip, and the window's
# length alone decides its passes and its end; wave 0 has runs of 1, 2 and 5 trips between per-tap trips that are plain ones.
LENGTH_JOBS = [_job(TRIP * k + r, off, 0.37) for k in range(2, 13) for r in (0, 1, 300) for off in (0, 1)]
# other steps: the crossings fall elsewhere, into either wave's half, and the trip behind a run of pairs -- the one the last pass' look-ahead loads belong to -- or the
# one behind that holds a crossing
CROSSING_JOBS = [_job(TRIP * k + r, off, 0.37, step) for step in (0.03, 0.05) for k in (10, 12) for r in (0, 300) for off in (0, 1)]
# the stream buffer's end: the window's last sample is the buffer's last one, at the end of a plain trip (whole trips from an even sample) and inside a masked tail
END_JOBS = [_job(n, STREAM_LEN - n, 0.37) for n in (TRIP * 4, TRIP * 5, TRIP * 6 + 300, TRIP * 7 + 301, TRIP * 12)]
# exact re-seeds at trip 16, in a run of trips in one binade from chip 520 on: at 0.0409 chips per sample the run starts at trip 13, the re-seed would meet the second
# trip of a pair and the trip in front of it stays single; at 0.045 it starts at trip 12 and the re-seed meets the first trip of a pass inside the run
RESEED_JOBS = [_job(12500, 0, -520.25), _job(12500, 1, -520.25), _job(12500, 0, -520.25, 0.045)]
# 36 trips, the last eleven in the binade of 512 chips: the run goes on across the end of the judgement mask's first word (trip 32)
MASK_WORD_JOBS = [_job(18000, 0, 0.37), _job(18301, 1, 0.37)]
JOBS = LENGTH_JOBS + CROSSING_JOBS + END_JOBS + RESEED_JOBS + MASK_WORD_JOBS
# a ring of 12 402 samples (and 6 200 of mirror) after three pushes holds samples 5 598 ... 17 999, and sample 12 402 lies at its start again: windows across it
RING_CAP, RING_WIN = 12402, 6200
RING_PUSHES = (0, 6000, 12000, 18000)
RING_JOBS = [_job(n, RING_CAP - back, 0.37) for n, back in ((TRIP * 10 + 300, 2000), (TRIP * 10 + 300, 2049), (TRIP * 6, 1024), (TRIP * 12, 4001), (TRIP * 4 + 1, 700))]


def queue_plan(job, wave):
    """(plan, reseeds, loads) of one wave at 128 threads.  plan: the form of every trip -- 'T' per-tap, 'H' a half-chip trip on its own, 'P' / 'Q' the two trips of a
    pass of a run of pairs, 'p' / 'q' those of its last pass; loads[i] = (the trip that issues trip i's loads, -1: in front of the first trip; plain form or not)."""
    _, n_trips, first_plain, last_plain = pairs.geometry(job, WG)
    ok = pairs.verdicts(job, WG)[wave]
    plain = [first_plain <= i < last_plain for i in range(n_trips)]
    fast = [plain[i] and ok[2 * i] and ok[2 * i + 1] for i in range(n_trips)]
    form, reseeds, loads, until = [None] * n_trips, [], {}, 0
    done = -1  # trips [0, done] have run

    def issue(i, by, plain_form):
        assert i not in loads, (i, by, "loaded twice")
        assert 0 <= i < n_trips and by < i
        assert plain[i] or not plain_form, (i, by, "a masked trip loaded in the plain form")
        loads[i] = (by, plain_form)

    def trip(i, f):
        nonlocal until, done
        assert i == done + 1 and i in loads
        if until == 0:
            assert f not in "Qq", "a re-seed on the second trip of a pair"
            reseeds.append(i)
            until = RESEED
        until -= 1
        form[i] = f
        done = i

    def single(i, f):
        assert set(loads) == set(range(i + 1)), (i, sorted(loads), "outside a run of pairs exactly this trip's loads are in flight")
        trip(i, f)
        if i + 1 < n_trips:
            issue(i + 1, i, plain[i + 1])

    def paired_run(i):
        if not (first_plain <= i < last_plain) or 2 * i >= 128:
            return 0
        run, word_end = 0, (64 - (2 * i & 63)) // 2
        while run < word_end and i + run < last_plain and fast[i + run]:
            run += 1
        return run
    if n_trips > 0:
        issue(0, -1, plain[0])
    i = 0
    while i < n_trips:
        run = paired_run(i)
        while run > 0:
            n_pass = min(run, last_plain - 1 - i) >> 1
            if until & 1:
                n_pass = min(n_pass, until >> 1)
            if n_pass > 0:
                run -= 2 * n_pass
                assert set(loads) == set(range(i + 1))
                issue(i + 1, i - 1, True)  # on entering the run: its second trip's loads
                for k in range(n_pass):
                    last = k == n_pass - 1
                    assert fast[i] and fast[i + 1]
                    trip(i, "p" if last else "P")
                    issue(i + 2, i, True)
                    trip(i + 1, "q" if last else "Q")
                    if not last:
                        issue(i + 3, i + 1, True)
                    i += 2
            else:
                single(i, "H")
                i += 1
                run -= 1
            if run == 0:
                run = paired_run(i)
        if i >= n_trips:
            break
        single(i, "T")
        i += 1
    assert set(loads) == set(range(n_trips)) and None not in form
    return "".join(form), reseeds, loads


def _passes(plan):
    """passes of every run of pairs of a plan"""
    return [len(r) // 2 for r in "".join(c if c in "PQpq" else " " for c in plan).split()]


def _half_runs(plan):
    return [len(r) for r in "".join(c if c in "HPQpq" else " " for c in plan).split()]


def test_the_windows_produce_the_cases():
    """No GPU: the loop's decisions and its load queue, restated in numpy float32 (128 threads)."""
    every = JOBS + RING_JOBS
    plans = {(j, w): queue_plan(job, w) for j, job in enumerate(every) for w in (0, 1)}
    at = {}
    for name, jobs in (("length", LENGTH_JOBS), ("crossing", CROSSING_JOBS), ("end", END_JOBS), ("reseed", RESEED_JOBS), ("word", MASK_WORD_JOBS), ("ring", RING_JOBS)):
        first = sum(len(v) for v in at.values())
        at[name] = range(first, first + len(jobs))
    for (j, w), (plan, reseeds, loads) in plans.items():
        job = every[j]
        _, n_trips, first_plain, last_plain = pairs.geometry(job, WG)
        print(j, w, job["n_samples"], job["sample_offset"], plan)
        assert len(plan) == n_trips and reseeds == list(range(0, n_trips, RESEED)), (j, w, plan, reseeds)
        # the same trips pair up as with the one-deep queue, and the last pass of every run of pairs is the peeled one
        old = pairs.loop_plan(job, WG, w)[0].replace("A", "T").replace("B", "T")
        assert plan.upper() == old and "Qq" not in plan.replace("Qp", "") and all(plan[i - 1] == "p" for i, c in enumerate(plan) if c == "q"), (j, w, plan, old)
        assert all(plan[i + 1] in "Pp" for i, c in enumerate(plan) if c == "Q") and all(i + 1 == n_trips or plan[i + 1] not in "Q" for i, c in enumerate(plan) if c == "q")
        # the loads: never more than two trips ahead, two ahead only from inside a run of pairs (or on entering it), and the trip behind a run is a plain one
        for i, (by, plain_form) in loads.items():
            assert i - by in (1, 2), (j, w, i, by)
            if i - by == 2:
                assert plain_form and (plan[by] in "PQp" or plan[i - 1] in "Pp"), (j, w, i, by, plan)
        assert all(i + 1 < last_plain for i, c in enumerate(plan) if c == "q"), (j, w, plan)
    word = lambda name: [plans[(j, w)][0] for j in at[name] for w in (0, 1)]  # noqa: E731
    # windows of 2 ... 12 trips: runs of one, two, three and four passes; odd and even runs; no pair at all in the shortest
    length_plans = word("length")
    assert all(2 <= len(p) <= 13 for p in length_plans) and {len(p) for p in length_plans} >= {2, 3, 12}
    n_pass = {n for p in length_plans for n in _passes(p)}
    assert {1, 2, 3, 4} <= n_pass, n_pass
    assert any(not _passes(p) for p in length_plans)
    runs = {n for p in length_plans for n in _half_runs(p)}
    assert {n % 2 for n in runs} == {0, 1} and {2, 3, 4, 5} <= runs, runs
    assert {every[j]["sample_offset"] & 1 for j in at["length"]} == {0, 1}
    # the masked tail two and three trips behind a run's last pair; and right behind what would have been a pair: those two trips stay single
    assert any(p.endswith("pqHT") for p in length_plans) and any(p.endswith("pqHHT") for p in length_plans), length_plans
    assert any(p.endswith("pqH") for p in length_plans) and any(p.endswith("pqHH") for p in length_plans), length_plans  # (whole trips: the window ends with a plain trip)
    # crossings of a power of two: the trip behind a run of pairs -- the one whose loads the last pass issues -- is a per-tap trip, and one trip further
    crossing_plans = word("crossing") + length_plans
    assert any("pqT" in p and p.index("pqT") + 3 < len(p) for p in crossing_plans), crossing_plans
    assert any("pqHT" in p and p.index("pqHT") + 4 < len(p) for p in crossing_plans), crossing_plans
    assert {1, 2} <= {n for p in crossing_plans for n in _passes(p)}
    # the end of the stream buffer, in a plain trip and in a masked one, behind a run of pairs
    for j in at["end"]:
        assert every[j]["sample_offset"] + every[j]["n_samples"] == STREAM_LEN and _passes(plans[(j, 1)][0])
    assert {plans[(j, 1)][0][-1] for j in at["end"]} == {"H", "T"}
    # re-seeds: on the first trip of a pass inside a run, and where one would fall on a second trip the pairs end one trip early
    reseed_plans = word("reseed")
    assert any(p[16] in "Pp" and p[15] == "Q" for p in reseed_plans), reseed_plans
    assert any(p[14:16] == "qH" and p[16] in "Pp" for p in reseed_plans), reseed_plans
    # the run goes on in the judgement mask's second word: a run of pairs ends with trip 31 and another one starts with trip 32
    word_plans = word("word")
    assert all(len(p) >= 36 for p in word_plans) and any(p[28:32] == "PQpq" and p[32] in "Pp" for p in word_plans), word_plans
    # the ring: every window lies across the wrap and holds a run of pairs; one of them has its pairs on the wrap itself
    for j in at["ring"]:
        off, n = every[j]["sample_offset"], every[j]["n_samples"]
        assert off >= RING_PUSHES[-1] - RING_CAP and off + n <= RING_PUSHES[-1] and n <= RING_WIN and off % RING_CAP + n > RING_CAP and _passes(plans[(j, 1)][0])
    assert any(plans[(j, 1)][0][(RING_CAP - (every[j]["sample_offset"] & ~1)) // TRIP] in "PQpq" for j in at["ring"])


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_tracking_load_queue_gpu as T
from gnss_sdr_amd.tracking import CorrelatorBank
from gnss_sdr_amd.sample_stream import SampleStream
out = {{}}
code = T.pairs._codes()[0]
b = CorrelatorBank(1, len(code), device=0)
b.set_code(0, code)
b.set_splits(1)
for name, x, carrier in zip(("ones", "ints", "noise"), T.pairs._streams(), (False, False, True)):
    b.set_stream_host(x)
    out["flat_" + name] = b.correlate(T.pairs._with_carrier(T.JOBS) if carrier else T.JOBS)
for name, x, carrier in zip(("ones", "ints", "noise"), T.pairs._streams(), (False, False, True)):
    ring = SampleStream(T.RING_CAP, T.RING_WIN, device=0)
    for lo, hi in zip(T.RING_PUSHES[:-1], T.RING_PUSHES[1:]):
        assert ring.push(x[lo:hi]) == lo
    b.set_stream_ring(ring)
    out["ring_" + name] = b.correlate(T.pairs._with_carrier(T.RING_JOBS) if carrier else T.RING_JOBS)
    b.set_stream_ring(None)
    ring.close()
b.close()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def child_outputs(gpu, tmp_path_factory):
    """{body: arrays} at 128 threads: the half-chip trips (body 1) and the per-tap chains (body 3), the two child processes side by side."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    tmp = tmp_path_factory.mktemp("load_queue")
    procs = {}
    for body in ("1", "3"):
        f = str(tmp / f"out_{body}.npz")
        env = dict(os.environ, GSH_MC_WG=str(WG), GSH_MC_PACKED_BODY=body)
        procs[body] = (f, subprocess.Popen([sys.executable, "-c", script, f], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = {}
    for body, (f, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (body, log[-3000:])
        outs[body] = dict(np.load(f))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["flat", "ring"])
def test_every_window_selects_the_reference_chips_and_equals_the_per_tap_chains(child_outputs, where):
    """Every window above, out of a flat stream buffer and out of a ring across its wrap: the sums over x = 1 and over integer weights equal the oracle's (exact
    chips); all outputs, those over noise with a carrier included, equal the per-tap chains' bit for bit; the sums over noise lie within 1e-6 of the float64 truth."""
    ones, ints, noise = pairs._streams()
    code = pairs._codes()[0]
    jobs = JOBS if where == "flat" else RING_JOBS
    fast, slow = child_outputs["1"], child_outputs["3"]
    for name, x in (("ones", ones), ("ints", ints)):
        for j, job in enumerate(jobs):
            expect = pairs._exact_sums(job, code.astype(np.int32), x.real)
            got = fast[where + "_" + name][j, :3]
            assert np.array_equal(got.real.astype(np.float64), expect), (where, name, j, job, got, expect)
            assert np.all(got.imag == 0), (where, name, j, job, got)
    for name in ("ones", "ints", "noise"):
        a, b = fast[where + "_" + name], slow[where + "_" + name]
        assert a.shape == b.shape == (len(jobs), 8)
        assert np.all(np.isfinite(a.view(np.float32)))
        differ = [j for j in range(len(jobs)) if not np.array_equal(a[j].view(np.uint32), b[j].view(np.uint32))]
        assert not differ, (where, name, differ)
    worst = 0.0
    for j, job in enumerate(pairs._with_carrier(jobs)):
        _, t64, sabs = oracle_job(code, noise, job)
        err = scale_err(fast[where + "_noise"][j, :3], t64, sabs)
        worst = max(worst, float(err.max()))
        assert np.all(err <= TOL_TRUTH), (where, j, job, err)
    print(where, "worst |gpu - truth| / sum|x| =", worst)
