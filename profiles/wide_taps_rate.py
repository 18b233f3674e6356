"""Rate of the wide correlator bank against the same taps cut into eight-tap jobs (a tool, not a test; needs the GPU).

For each shape -- jobs x taps at N = 25 000 on one stream -- the wide form (gsh_bank_time_launches_wide) and the comparator (the same taps as ceil(T / 8)
gsh_corr_job per window through the unchanged eight-tap kernels, gsh_bank_time_launches) are timed alternately, three pairs after a warm-up, with device
events.  Before any time is taken the two forms' outputs on the timed inputs are compared: |wide - narrow| / sum|x| must hold the accumulator bar (1e-6).
Prints a table; --out FILE also writes it there.

    python profiles/wide_taps_rate.py [--out profiles/wide_taps_summary.txt] [--reps 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import oracle
from gnss_sdr_amd.tracking import CorrelatorBank, make_jobs, make_jobs_wide
from helpers import synth_gps_l1_stream, tracking_params_for

FS, N, CHANNELS = 25e6, 25000, 32
PEAK_FP32 = 157.3e12  # packed-FP32 vector peak of the MI355X, flop/s
SHAPES = ((3200, 64), (3200, 16), (32, 64))  # jobs x taps
BAR = 1e-6


def build(n_jobs, n_taps, params):
    """The wide jobs and the comparator's eight-tap jobs (the groups of one window next to each other), epoch-major and channel-minor."""
    span = 0.05 * (n_taps - 1)  # 0.1 chip between taps: +-3.15 chips at 64
    sh = np.linspace(-span, span, n_taps).astype(np.float32)
    wide, narrow = [], []
    for j in range(n_jobs):
        e, c = divmod(j, CHANNELS)
        job = dict(sample_offset=(e % 8) * N + 3 * c + e % 2, n_samples=N, code_slot=c, **params[c])
        wide.append(dict(job, shifts_chips=sh))
        for t0 in range(0, n_taps, 8):
            narrow.append(dict(job, shifts_chips=sh[t0:t0 + 8]))
    return wide, narrow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prns = [1 + c % 32 for c in range(CHANNELS)]
    dopp = [-4500.0 + 290.0 * c for c in range(CHANNELS)]
    x = synth_gps_l1_stream(9 * N + 200, FS, prns[:8], dopp[:8], [30.0 + 90.0 * i for i in range(8)], seed_noise=0x5EED0002)
    rng = np.random.default_rng(6)
    params = [tracking_params_for(FS, d, rng) for d in dopp]
    bank = CorrelatorBank(CHANNELS, 1023, device=0)
    for c in range(CHANNELS):
        bank.set_code(c, oracle.ca_code(prns[c]))
    bank.set_stream_host(x)
    ax = np.abs(x.astype(np.complex128))
    csum = np.concatenate([[0.0], np.cumsum(ax)])

    say("wide bank vs the same taps as eight-tap jobs, N = %d, one stream; device events, %d launches per figure" % (N, a.reps))
    say("%-18s %12s %12s %8s %22s %14s %10s" % ("jobs x taps", "wide us", "8-tap us", "ratio", "8-tap repeats us", "Gtap-samples/s", "% FP32 pk"))
    verdicts = []
    for n_jobs, n_taps in SHAPES:
        wide, narrow = build(n_jobs, n_taps, params)
        wj, nj = make_jobs_wide(wide), make_jobs(narrow)
        # ---- the two forms agree on the timed inputs before any ratio is quoted
        ow = bank.correlate_wide(wj)
        on = bank.correlate(nj)
        g = (n_taps + 7) // 8
        worst = 0.0
        for j, job in enumerate(wide):
            sabs = csum[job["sample_offset"] + N] - csum[job["sample_offset"]]
            ref = np.concatenate([on[j * g + k, :min(8, n_taps - 8 * k)] for k in range(g)])
            worst = max(worst, float(np.abs(ow[j, :n_taps].astype(np.complex128) - ref).max() / sabs))
        if not worst <= BAR:
            say("%d x %d: the two forms differ by %.3g of sum|x| (bar %.0e): not timed" % (n_jobs, n_taps, worst, BAR))
            verdicts.append(False)
            continue
        reps = a.reps if n_jobs >= 1000 else 10 * a.reps
        bank.upload_jobs(nj)
        bank.time_launches(3)
        bank.time_launches_wide(wj, 3)
        pairs = []
        for _ in range(3):
            t_n = bank.time_launches(reps) * 1e3
            t_w = bank.time_launches_wide(wj, reps) * 1e3
            pairs.append((t_w, t_n))
        for k, (t_w, t_n) in enumerate(pairs):
            flops = n_jobs * N * (6 + 4 * n_taps)
            say("%-18s %12.1f %12.1f %8.2f %22s %14.1f %10.1f" % (
                "%d x %d #%d" % (n_jobs, n_taps, k + 1), t_w, t_n, t_n / t_w,
                ("%.1f .. %.1f" % (min(p[1] for p in pairs), max(p[1] for p in pairs))) if k == 0 else "",
                n_jobs * n_taps * N / (t_w * 1e-6) / 1e9, 100.0 * flops / (t_w * 1e-6) / PEAK_FP32))
        faster = all(t_w < t_n for t_w, t_n in pairs)
        verdicts.append(faster)
        say("%d x %d: outputs agree to %.2g of sum|x|; wide %s in all three pairs" % (n_jobs, n_taps, worst, "FASTER" if faster else "NOT faster"))
    bank.close()
    say("verdict: the wide form is %s" % ("faster at every shape, in every pair" if all(verdicts) else "NOT faster at every shape (see above)"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
