"""One anchor per lane for the half-chip trips' sample numbers (csrc/mcorr_device.h run_segment_packed, GSH_MC_ANCHOR_FMA, round 13), on the device.

The half-chip trips form the products step' n of a trip's second chunk, and of the second trip of a pair, by v_pk_fma_f32 from the first chunk's running sample number
instead of keeping and stepping a number per chunk.  Each product is the multiply's bit for bit (tests/test_tracking_anchor_fma.py), so nothing that is summed changes:
  * the default build equals the per-tap chains (GSH_MC_PACKED_BODY=3) bit for bit, at 128 threads (single trips and trip pairs) and at 256 threads (single trips);
  * a forced walk (GSH_MC_WALK=8) equals the run of the same tables without it (GSH_MC_WALK=0), both at 128 threads, bit for bit;
  * over carrier-free integer-valued samples the three sums equal the oracle's exact sums: every chip is the reference's;
  * over noise with a carrier the sums lie within 1e-6 of the float64 truth.
The jobs are tests/test_tracking_anchor_fma.py's -- windows of 512 ... 33 001 samples from even and odd samples at 4, 10, 25 and 50 Msps, Doppler +-5 kHz, code phases
0, 1e-30, 0.37 and 0.999, short windows from chip 520 on, windows that end on the stream's last sample, a code phase the guard rejects -- which that file shows to reach
every way through the loop; here one launch per rate, so that the launches of 25 and 50 Msps are half-chip launches whatever the others need.  The same windows also
run out of a ring, across its wrap.  The switches are read once per process: five child processes side by side, as tests/test_tracking_trip_pairs_gpu.py does.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import test_tracking_anchor_fma as A
from helpers import TOL_SCALE, oracle_job, scale_err

f32 = np.float32
TOL_TRUTH = 1e-6  # |gpu - float64 truth| / sum|x|
assert TOL_TRUTH <= TOL_SCALE
# a ring of 52 002 samples (25 100 of mirror) after three pushes holds samples 25 998 ... 77 999; sample 52 002 lies at its start again
RING_CAP, RING_WIN = 52002, 25100
RING_PUSHES = (0, 26000, 52000, 78000)
RING_WINDOWS = [(25000, 39999), (25000, 27500), (16387, 43000), (8229, 47001), (2049, 51000), (2049, 50001), (1025, 51500), (1025, 51001), (513, 51801), (3072, 50000),
                (2048, 50979), (1024, 51490)]


def launches():
    """[(name, jobs)]: one launch per sample rate, then the other jobs"""
    per_rate = len(A.GRID_JOBS) // len(A.RATES)
    groups, at = [], 0
    for fs in A.RATES:
        count = sum(1 for j in A.GRID_JOBS if f32(j["code_phase_step_chips"]) in (A.ca_step(fs, 5000.0), A.ca_step(fs, -5000.0)))
        groups.append(("fs%d" % int(fs / 1e6), A.GRID_JOBS[at:at + count]))
        at += count
    assert at == len(A.GRID_JOBS) and per_rate > 0
    groups.append(("far", A.FAR_JOBS + A.END_JOBS + A.TINY_JOBS))
    return groups


def ring_jobs():
    far = A.FAR_JOBS
    return [dict(far[k % len(far)] if k % 3 == 2 else A.GRID_JOBS[-1 - 8 * k], n_samples=n, sample_offset=off) for k, (n, off) in enumerate(RING_WINDOWS)]


def streams(n):
    rng = np.random.default_rng(1313)
    ints = rng.integers(-7, 8, n).astype(f32).astype(np.complex64)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return ints, noise


def no_carrier(jobs):
    return [dict(j, rem_carr_phase_rad=0.0, phase_step_rad=0.0) for j in jobs]


def code():
    return oracle.ca_code(7).astype(f32)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_tracking_anchor_fma_gpu as T
from gnss_sdr_amd import _lib
from gnss_sdr_amd.tracking import CorrelatorBank
from gnss_sdr_amd.sample_stream import SampleStream
lib = _lib.load()
out = {{}}
def walked(f):
    before = lib.gsh_mcorr_walk_launches()
    r = f()
    return r, lib.gsh_mcorr_walk_launches() - before
b = CorrelatorBank(1, 1023, device=0)
b.set_code(0, T.code())
b.set_splits(1)
for name, x in zip(("ints", "noise"), T.streams(T.A.STREAM_LEN)):
    b.set_stream_host(x)
    for tag, jobs in T.launches():
        t = T.no_carrier(jobs) if name == "ints" else jobs
        out[tag + "_" + name], out["walked_" + tag + "_" + name] = walked(lambda: b.correlate(t))
for name, x in zip(("ints", "noise"), T.streams(T.RING_PUSHES[-1])):
    ring = SampleStream(T.RING_CAP, T.RING_WIN, device=0)
    for lo, hi in zip(T.RING_PUSHES[:-1], T.RING_PUSHES[1:]):
        assert ring.push(x[lo:hi]) == lo
    b.set_stream_ring(ring)
    t = T.no_carrier(T.ring_jobs()) if name == "ints" else T.ring_jobs()
    out["ring_" + name], out["walked_ring_" + name] = walked(lambda: b.correlate(t))
    b.set_stream_ring(None)
    ring.close()
b.close()
np.savez(sys.argv[1], **out)
"""

ENVS = {"fast128": dict(GSH_MC_WG="128", GSH_MC_WALK="0"), "taps128": dict(GSH_MC_WG="128", GSH_MC_WALK="0", GSH_MC_PACKED_BODY="3"),
        "fast256": dict(GSH_MC_WG="256"), "taps256": dict(GSH_MC_WG="256", GSH_MC_PACKED_BODY="3"), "walk128": dict(GSH_MC_WG="128", GSH_MC_WALK="8")}


@pytest.fixture(scope="module")
def child_outputs(gpu, tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    tmp = tmp_path_factory.mktemp("anchor_fma")
    base = {k: v for k, v in os.environ.items() if k not in ("GSH_MC_WG", "GSH_MC_WALK", "GSH_MC_PACKED_BODY")}
    procs = {}
    for tag, env in ENVS.items():
        f = str(tmp / f"out_{tag}.npz")
        procs[tag] = (f, subprocess.Popen([sys.executable, "-c", script, f], cwd=root, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = {}
    for tag, (f, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (tag, log[-3000:])
        outs[tag] = dict(np.load(f))
    return outs


def _tables():
    """[(key, jobs, integer stream, noise stream)] of every launch"""
    ints, noise = streams(A.STREAM_LEN)
    rints, rnoise = streams(RING_PUSHES[-1])
    return [(tag, jobs, ints, noise) for tag, jobs in launches()] + [("ring", ring_jobs(), rints, rnoise)]


@pytest.fixture(scope="module")
def references():
    """{key: (exact sums over the integer stream [jobs, 3], float64 truth over noise [jobs, 3], sum|x| [jobs])}, computed once"""
    c = code()
    ref = {}
    for key, jobs, ints, noise in _tables():
        exact, truth, sabs = [], [], []
        for job in jobs:
            idx = oracle.code_indices(job["n_samples"], np.asarray(A.HALF_SHIFTS, f32), job["rem_code_phase_chips"], job["code_phase_step_chips"], 0.0, len(c), False)
            seg = ints.real[job["sample_offset"]:job["sample_offset"] + job["n_samples"]].astype(np.float64)
            exact.append([(c[idx[t]].astype(np.float64) * seg).sum() for t in range(3)])
            _, t64, s = oracle_job(c, noise, job)
            truth.append(t64)
            sabs.append(s)
        ref[key] = (np.array(exact), np.array(truth), np.array(sabs))
    return ref


def test_the_tables_hold_the_issues_shapes():
    """No GPU: a few hundred jobs; every ring window lies across the wrap, inside what the ring holds; the stream's last sample ends a window."""
    n = sum(len(jobs) for _, jobs in launches())
    assert n == len(A.JOBS) and 150 <= n + len(RING_WINDOWS) <= 500
    assert [tag for tag, _ in launches()] == ["fs4", "fs10", "fs25", "fs50", "far"]
    for length, off in RING_WINDOWS:
        assert off < RING_CAP < off + length and off >= RING_PUSHES[-1] - RING_CAP and off + length <= RING_PUSHES[-1] and length <= RING_WIN
    assert {off & 1 for _, off in RING_WINDOWS} == {0, 1}
    assert any(j["sample_offset"] + j["n_samples"] == A.STREAM_LEN for j in A.END_JOBS)


def _bit_equal(a, b, what):
    assert a.shape == b.shape and a.shape[1] >= 3 and np.all(np.isfinite(a.view(np.float32)))
    differ = [j for j in range(len(a)) if not np.array_equal(a[j].view(np.uint32), b[j].view(np.uint32))]
    assert not differ, (what, differ[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("fast,slow", [("fast128", "taps128"), ("fast256", "taps256"), ("walk128", "fast128")])
def test_outputs_are_bit_equal_and_the_chips_are_the_references(child_outputs, references, fast, slow):
    a, b = child_outputs[fast], child_outputs[slow]
    worst = 0.0
    for key, jobs, _, _ in _tables():
        exact, truth, sabs = references[key]
        for name in ("ints", "noise"):
            _bit_equal(a[key + "_" + name], b[key + "_" + name], (fast, slow, key, name))
        got = a[key + "_ints"][:, :3]
        wrong = [j for j in range(len(jobs)) if not (np.array_equal(got[j].real.astype(np.float64), exact[j]) and np.all(got[j].imag == 0))]
        assert not wrong, (fast, key, wrong[:10], [jobs[j] for j in wrong[:3]])
        for j in range(len(jobs)):
            err = scale_err(a[key + "_noise"][j, :3], truth[j], sabs[j])
            worst = max(worst, float(err.max()))
            assert np.all(err <= TOL_TRUTH), (fast, key, j, jobs[j], err)
    print(fast, "worst |gpu - truth| / sum|x| =", worst)
    # the forced walk walked the half-chip launches, the others never did
    counts = {k: int(v) for k, v in a.items() if k.startswith("walked_")}
    print(fast, counts)
    if fast == "walk128":
        assert all(counts["walked_%s_%s" % (key, name)] >= 1 for key in ("fs25", "fs50", "far", "ring") for name in ("ints", "noise")), counts
    else:
        assert not any(counts.values()), counts
