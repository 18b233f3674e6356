"""Time of the conditioner's push with the notch stage against the loose chain it replaces (a tool, not a test; needs the GPU).

One 25 000-sample ibyte block, inverted, through K = 33, D = 2, f_c / f_s = 0.15 and a 4 -> 2.5 Msps resampler, Notch with L = 32, on handles primed
with the same 100 000 samples: once with every segment filtered and no floor values formed, once with every segment estimating.  The stage:
gsh_cond_time_push between two device events, and a HOST clock around gsh_cond_push_device + a stream synchronise.  The loose chain: a host clock
around gsh_convert_samples_device -> gsh_fir_process_device -> synchronise -> gsh_notch_process_device (it runs on a private stream and synchronises
inside, so device events cannot bracket it) -> gsh_direct_resample_device -> gsh_stream_push_device -> synchronise: what a caller of the loose calls
pays per block.  20 warm-up blocks, then five alternating rounds of 200 blocks.  Prints the figures and writes them to
profiles/conditioner_notch_rate.json (the committed file is the run quoted in DESIGN.md 3.4b).

    python profiles/conditioner_notch_rate.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd import SignalConditioner
from gnss_sdr_amd.sample_stream import FirFilter, NotchFilter, SampleStream, convert_samples_device, direct_resample_device

N, K, D, FC, FS, RS = 25000, 33, 2, 1.2e6, 8e6, (4e6, 2.5e6)
taps = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (2.5 * D))).astype(np.float32)
taps /= taps.sum()
rng = np.random.default_rng(3)
n_prime = 4 * N
x = rng.standard_normal((n_prime + N, 2)) * 8.0
x[:, 0] += 30.0 * np.cos(2 * np.pi * -0.13 * np.arange(len(x)))
x[:, 1] += 30.0 * np.sin(2 * np.pi * -0.13 * np.arange(len(x)))
raw = np.clip(np.round(x), -127, 127).astype(np.int8)
dev = torch.device("cuda", 0)
d_raw = torch.from_numpy(raw).to(dev)
side = torch.cuda.Stream(device=dev)
s = side.cuda_stream
block = d_raw.data_ptr() + 2 * n_prime
out = {}
for label, notch in (("steady state (no floor values)", dict(length=32, segments_est=40, segments_reset=5000000)),
                     ("estimating (floor values formed)", dict(length=32, segments_est=1000000, segments_reset=5000000))):
    ring = SampleStream(1 << 20, 4096, device=0)
    cond = SignalConditioner(ring, "ibyte", True, taps, D, FC, FS, RS[0], RS[1], device=0, notch=notch)
    cond.push_device(d_raw.data_ptr(), n_prime, hip_stream=s)
    side.synchronize()
    st = cond.notch_state()
    # the loose chain, primed alike
    ring2 = SampleStream(1 << 20, 4096, device=0)
    fir = FirFilter(taps, D, FC, FS, "gr_complex", device=0)
    nf = NotchFilter(0.001, 0.9, 32, notch["segments_est"], notch["segments_reset"], 0, device=0)
    d_x = torch.zeros(n_prime, dtype=torch.complex64, device=dev)
    d_y = torch.zeros(n_prime // D + 2, dtype=torch.complex64, device=dev)
    d_w = torch.zeros(n_prime // D + 2, dtype=torch.complex64, device=dev)
    d_r = torch.zeros(n_prime // D + 2, dtype=torch.complex64, device=dev)

    def loose(ptr, n):
        convert_samples_device(0, ptr, "ibyte", d_x.data_ptr(), n, inverted_spectrum=True, hip_stream=s)
        m = fir.process_device(d_x.data_ptr(), n, d_y.data_ptr(), d_y.numel(), hip_stream=s)
        side.synchronize()                       # the notch call runs on its own stream
        w = nf.process_device(d_y.data_ptr(), m, d_w.data_ptr())
        n_r, _c = direct_resample_device(0, d_w.data_ptr(), 0, w, RS[0], RS[1], 0, d_r.data_ptr(), d_r.numel(), hip_stream=s)
        ring2.push_device(d_r.data_ptr(), n_r, hip_stream=s)
        side.synchronize()

    loose(d_raw.data_ptr(), n_prime)

    def stage_wall(reps):
        t = time.perf_counter()
        for _ in range(reps):
            cond.push_device(block, N, hip_stream=s)
            side.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    def loose_wall(reps):
        t = time.perf_counter()
        for _ in range(reps):
            loose(block, N)
        return (time.perf_counter() - t) / reps * 1e3

    stage_wall(20), loose_wall(20)               # warm-up of every shape
    ev = [cond.time_push(block, N, reps=200) for _ in range(5)]
    sw, lw = [], []
    for _ in range(5):                           # alternating
        sw.append(stage_wall(200))
        lw.append(loose_wall(200))
    res = dict(stage_event_ms=ev, stage_wall_ms=sw, loose_wall_ms=lw, ratio_wall=float(np.median(lw) / np.median(sw)), state_before=str(st), state_after=str(cond.notch_state()))
    out[label] = res
    print(label, json.dumps(res, indent=1))
    cond.close(); fir.close(); nf.close(); ring.close(); ring2.close()
with open(os.path.join(ROOT, "profiles", "conditioner_notch_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
