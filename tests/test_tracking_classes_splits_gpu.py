"""A batch of mixed tap counts, with and without split windows, whose three-tap class runs the two-wave kernels (csrc/multicorrelator.hip launch_class,
reduce_if_split; csrc/multicorrelator_t128.hip): every class is one launch among the others and the partials are summed once, behind the last of them.

A bank of 12 jobs over GPS C/A codes, tap counts 1, 3 and 5 mixed (job i has TAPS[i % 3] taps, so the bank launches per class), the three-tap jobs E/P/L at
+-0.5 chip; noise with a carrier, and carrier-free integer-valued samples.  Two sets of windows, offsets of both parities:
  * 2 048, 2 049 and 4 100 samples.  The bank keeps at least 2 048 samples per work-group (tracking_api.hip bank_splits), so set_splits(2) leaves these whole;
  * 4 096, 4 099 and 8 200 samples, which set_splits(2) does cut in two: the launches that write partials.
Each with set_splits(2) and again with set_splits(1).  At 4 Msps the longest window of either set spans the whole code, so the host stages whole codes and the
three-tap class is one that GSH_MC_WG=128 sends to the two-wave kernels.

GSH_MC_WG is read once per process, so the kernels run in child processes (as in tests/test_tracking_walk_gpu.py): child A with GSH_MC_WG=128, child B with
GSH_MC_WG=256; A also runs the three-tap jobs alone, as a plain (single-class) bank with the same splits.  Held:
  * in A the 1- and 5-tap rows equal B's bit for bit (they run the four-wave kernels in both);
  * in A the three-tap rows equal the plain bank's bit for bit (the same kernel, the same split order) -- and differ from B's over noise (two waves sum in
    another order than four: A did take other kernels);
  * over integer samples every row equals the oracle's sums exactly, over noise it lies within TOL_TRUTH of the float64 truth; unused tap columns are zero.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import test_tracking_walk_gpu as W
from helpers import tracking_params_for

f32 = np.float32
FS = 4e6
N_JOBS = 12
N_CH = 4
TAPS = [1, 3, 5]
SHIFTS = {1: [0.0], 3: [-0.5, 0.0, 0.5], 5: [-1.0, -0.5, 0.0, 0.5, 1.0]}
WINDOW_SETS = {"whole": [2048, 2049, 4100], "cut": [4096, 4099, 8200]}
SPLITS = [2, 1]
STREAM_LEN = 8200 + 129


def codes():
    return [oracle.ca_code(prn).astype(np.int32) for prn in range(1, N_CH + 1)]


def streams():
    return W.streams(STREAM_LEN)


def table(windows, seed=0):
    jobs = []
    for i in range(N_JOBS):
        rng = np.random.default_rng(7919 * seed + i)
        p = tracking_params_for(FS, float(rng.uniform(-5000, 5000)), rng)
        jobs.append(dict(sample_offset=int((i * 37 + 5 + seed) % 129), n_samples=int(windows[(i // 3) % 3]), code_slot=i % N_CH,
                         shifts_chips=list(SHIFTS[TAPS[i % 3]]), **p))
    return jobs


def three_tap(jobs):
    return [j for j in jobs if len(j["shifts_chips"]) == 3]


def key(wset, name, splits, plain=False):
    return "%s_%s_s%d%s" % (wset, name, splits, "_plain" if plain else "")


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_tracking_classes_splits_gpu as T
from gnss_sdr_amd.tracking import CorrelatorBank
with_plain = sys.argv[2] == "plain"
out = {{}}
b = CorrelatorBank(T.N_CH, 1023, device=0)
for i, c in enumerate(T.codes()):
    b.set_code(i, c)
for name, x in zip(("ints", "noise"), T.streams()):
    b.set_stream_host(x)
    prep = T.W.no_carrier if name == "ints" else (lambda t: t)
    for wset, windows in T.WINDOW_SETS.items():
        jobs = prep(T.table(windows))
        for splits in T.SPLITS:
            b.set_splits(splits)
            b.correlate(prep(T.table(windows, seed=3)))  # stale rows
            out[T.key(wset, name, splits)] = b.correlate(jobs)
            if with_plain:
                b.correlate(T.three_tap(prep(T.table(windows, seed=3))))
                out[T.key(wset, name, splits, plain=True)] = b.correlate(T.three_tap(jobs))
b.close()
np.savez(sys.argv[1], **out)
"""


def test_the_tables_drive_what_they_claim():
    """(no GPU) every tap class meets every window of a set, its shortest included (the plain bank then splits as the mixed one does); set_splits(2) cuts the
    second set only; the longest window spans the code, so whole codes are staged; offsets of both parities; the three-tap jobs are half-chip E/P/L sets."""
    for wset, windows in WINDOW_SETS.items():
        t = table(windows)
        for taps in TAPS:
            assert {j["n_samples"] for j in t if len(j["shifts_chips"]) == taps} == set(windows), (wset, taps)
        assert min(windows) // 2048 == (2 if wset == "cut" else 1)  # bank_splits: at least 2 048 samples per work-group
        seg = max(windows) // (min(windows) // 2048)  # the longest window's segment at the most splits the bank grants
        assert all(2 * (j["code_phase_step_chips"] * seg + 16) > 1023 + 64 for j in t if j["n_samples"] == max(windows))  # bank_window_floats: no code window
        assert {j["sample_offset"] & 1 for j in t} == {0, 1} and {j["sample_offset"] & 1 for j in three_tap(t)} == {0, 1}
        assert max(j["sample_offset"] + j["n_samples"] for j in t + table(windows, seed=3)) <= STREAM_LEN
        assert all(j["shifts_chips"] == [-0.5, 0.0, 0.5] for j in three_tap(t)) and len(three_tap(t)) == 4


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """{"A": arrays, "B": arrays}: the two child processes, side by side."""
    tmp = tmp_path_factory.mktemp("classes_splits")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    procs = {}
    for tag, wg, what in (("A", "128", "plain"), ("B", "256", "mixed")):
        env = {k: v for k, v in os.environ.items() if k not in ("GSH_MC_WALK", "GSH_MC_WG")}
        env["GSH_MC_WG"] = wg
        f = str(tmp / (tag + ".npz"))
        procs[tag] = (f, subprocess.Popen([sys.executable, "-c", script, f, what], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = {}
    for tag, (f, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, (tag, log[-3000:])
        outs[tag] = dict(np.load(f))
    return outs


def _cases():
    return [(wset, windows, splits) for wset, windows in WINDOW_SETS.items() for splits in SPLITS]


def _rows(jobs, taps):
    return [i for i, j in enumerate(jobs) if len(j["shifts_chips"]) in taps]


@pytest.mark.gpu
def test_one_and_five_tap_rows_are_the_four_wave_kernels_in_both(runs):
    for wset, windows, splits in _cases():
        rows = _rows(table(windows), (1, 5))
        for name in ("ints", "noise"):
            k = key(wset, name, splits)
            W._same_bits(runs["A"][k][rows], runs["B"][k][rows], k)


@pytest.mark.gpu
def test_three_tap_rows_are_the_plain_banks_and_not_the_four_wave_kernels(runs):
    for wset, windows, splits in _cases():
        rows = _rows(table(windows), (3,))
        for name in ("ints", "noise"):
            k = key(wset, name, splits)
            W._same_bits(runs["A"][k][rows], runs["A"][key(wset, name, splits, plain=True)], k)
        k = key(wset, "noise", splits)
        assert not np.array_equal(runs["A"][k][rows].view(np.uint32), runs["B"][k][rows].view(np.uint32)), k


@pytest.mark.gpu
def test_every_row_is_the_oracles(runs):
    cs = codes()
    ints, noise = streams()
    worst = 0.0
    for wset, windows, splits in _cases():
        jobs = table(windows)
        for tag in ("A", "B"):
            W._exact(runs[tag][key(wset, "ints", splits)], W.no_carrier(jobs), cs, ints, (tag, wset, splits))
            out = runs[tag][key(wset, "noise", splits)]
            worst = max(worst, W._truth(out, jobs, cs, noise, (tag, wset, splits)))
            for j, job in enumerate(jobs):
                assert np.all(out[j, len(job["shifts_chips"]):] == 0), (tag, wset, splits, j, out[j])
        W._exact(runs["A"][key(wset, "ints", splits, plain=True)], W.no_carrier(three_tap(jobs)), cs, ints, ("plain", wset, splits))
    print("worst |gpu - truth| / sum|x| =", worst)
