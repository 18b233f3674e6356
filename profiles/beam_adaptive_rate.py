"""Rate of the beamformer's adaptive push against the fixed push and the host loop it replaces (a tool, not a test; needs the GPU).

One block of 2^22 ishort frames of 4 antennas (interleaved: 16-byte frames), 2 beams, each into its ring, in one process on one device:
  fixed push      gsh_beam_push / gsh_beam_push_device with the caller's weights
  adaptive push   the same calls on an adaptive handle: covariance -> final sums -> accumulate and solve -> beam pass, on the push's stream
  host loop       what the adaptive push replaces: gsh_beam_covariance (synchronises, reads R back), numpy power-inversion weights,
                  gsh_beam_set_weights, gsh_beam_push (the block crosses PCIe a second time)
all three timed with the HOST clock around the synchronous calls, `--runs` runs each after a warm-up, taken in turn so that drift hits them alike;
and the device work alone, between two device events (gsh_beam_time_process: on an adaptive handle the whole chain), next to the expectation it is
compared with -- the fixed beam pass plus the covariance call of the same run (the same kernels; the covariance call's figure is host-clocked and
includes its 36-number read-back).  min / median / max over the runs: the spread is the run-to-run spread of this process.

    python profiles/beam_adaptive_rate.py [--out profiles/beam_adaptive_rate.txt] [--runs 7]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd.array import ArrayFormat, Beamformer, power_inversion_weights
from gnss_sdr_amd.sample_stream import SampleStream

N, A, B = 1 << 22, 4, 2


def block():
    """noise of a few hundred counts and a strong CW jammer across the array, as 16-bit frames [N, A, 2]"""
    rng = np.random.default_rng(5)
    t = np.arange(N)
    jam = 8000.0 * np.exp(2j * np.pi * (0.01 * t))[:, None] * np.exp(1j * np.pi * np.arange(A) * np.sin(np.deg2rad(-40.0)))[None, :]
    x = jam + 300.0 * (rng.standard_normal((N, A)) + 1j * rng.standard_normal((N, A)))
    out = np.empty((N, A, 2), np.int16)
    out[..., 0] = np.clip(np.round(x.real), -32767, 32767)
    out[..., 1] = np.clip(np.round(x.imag), -32767, 32767)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    x = block()
    d_x = torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev)
    torch.cuda.synchronize()
    ptrs = [d_x.data_ptr()]
    fmt = ArrayFormat(A, "ishort", "interleaved")
    fixed, adaptive, loop = (Beamformer(fmt, B, device=0) for _ in range(3))
    adaptive.set_adaptive(reference=[0, 1], loading_rel=1e-6)
    rings = [SampleStream(N, 1024, device=0) for _ in range(B)]

    def host_loop():
        R = loop.covariance(x)
        loop.set_weights(np.stack([power_inversion_weights(R, r, loading=1e-6 * float(np.trace(R).real) / A) for r in range(B)]))
        loop.push(rings, x)

    def cov_call():
        fixed.covariance_device(ptrs, N)

    timed = (("fixed push (host block)", lambda: fixed.push(rings, x)),
             ("adaptive push (host block)", lambda: adaptive.push(rings, x)),
             ("host loop: covariance + numpy + set_weights + push", host_loop),
             ("fixed push_device", lambda: fixed.push_device(rings, ptrs, N)),
             ("adaptive push_device", lambda: adaptive.push_device(rings, ptrs, N)),
             ("covariance_device call (synchronous, reads R back)", cov_call))
    # the adaptive push and the host loop agree on what they compute before any time is quoted (float32 weights of two different solvers: not bit for bit)
    adaptive.push(rings, x)
    host_loop()
    w_a, w_h = adaptive.adaptive_state()["weights"], loop.weights
    say("beamformer: one block of 2^22 ishort frames x %d antennas (interleaved) -> %d beams into rings; %d runs per figure, min / median / max" % (A, B, a.runs))
    say("adaptive weights against the host loop's (numpy, float32): worst |dw| / |w| = %.2e" % float(np.max(np.abs(w_a - w_h)) / np.max(np.abs(w_h))))
    for _, f in timed:
        f()
    host_us = {name: [] for name, _ in timed}
    dev_us = {"fixed beam pass (device events)": [], "adaptive chain (device events)": []}
    for _ in range(a.runs):
        for name, f in timed:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            host_us[name].append((time.perf_counter() - t0) * 1e6)
        dev_us["fixed beam pass (device events)"].append(fixed.time_process(N, reps=10) * 1e3)
        dev_us["adaptive chain (device events)"].append(adaptive.time_process(N, reps=10) * 1e3)

    def row(name, v):
        v = sorted(v)
        say("%-56s %10.1f %10.1f %10.1f us" % (name, v[0], v[len(v) // 2], v[-1]))
        return v[len(v) // 2], v[-1] - v[0]

    say("%-56s %10s %10s %10s" % ("host clock around the synchronous call", "min", "median", "max"))
    med = {name: row(name, host_us[name]) for name, _ in timed}
    say("%-56s %10s %10s %10s" % ("device work alone", "min", "median", "max"))
    med.update({name: row(name, v) for name, v in dev_us.items()})
    beam, chain, cov = med["fixed beam pass (device events)"], med["adaptive chain (device events)"], med["covariance_device call (synchronous, reads R back)"]
    expect, spread = beam[0] + cov[0], max(beam[1], chain[1], cov[1])
    in_bytes, out_bytes = A * 4 * N, 8 * B * N
    say("expectation for the adaptive chain: fixed beam pass + covariance call = %.1f us; measured %.1f us (%+.1f us; run-to-run spread %.1f us)"
        % (expect, chain[0], chain[0] - expect, spread))
    say("bytes per block: %d in + %d out fixed (%.0f GB/s at the fixed pass's median), %d in + %d out adaptive (%.0f GB/s at the chain's median)"
        % (in_bytes, out_bytes, (in_bytes + out_bytes) / beam[0] / 1e3, 2 * in_bytes, out_bytes, (2 * in_bytes + out_bytes) / chain[0] / 1e3))
    say("adaptive push over the host loop, host blocks, medians: %.2fx" % (med["host loop: covariance + numpy + set_weights + push"][0] / med["adaptive push (host block)"][0]))
    for h in (fixed, adaptive, loop):
        h.close()
    for r in rings:
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
