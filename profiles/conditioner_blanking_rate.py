"""Rate of the conditioner's push with the pulse-blanking stage against the loose chain it replaces (a tool, not a test; needs the GPU).

For each shape the device work of one push on a handle with blanking -- gsh_cond_time_push: carry, filter outputs into the stage buffer, energies,
decision, masked gather, carry and history update, between two device events -- and the loose chain's four calls on the same block --
gsh_convert_samples_device -> gsh_fir_process_device -> gsh_pb_process_device -> gsh_direct_resample_device -- are timed alternately, three pairs after
a warm-up, in the same process on the same device.  The loose blanker runs on a private stream and synchronises inside its call, so the loose side is
timed with the HOST clock around a synchronised sequence (the stages before the blanker are synchronised for it, the sequence ends synchronised): its
figure includes those waits, which a receiver that uses the loose calls pays too; the fused figure is device time alone.  Before any time is taken the
two forms' outputs on the timed block are compared bit for bit (the loose blanker is offered one sample more: it leaves a segment that ends on the last
offered item for its next call).  Prints a table; --out FILE also writes it there.

    python profiles/conditioner_blanking_rate.py [--out profiles/conditioner_blanking_rate.txt] [--reps 20]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

from gnss_sdr_amd import SignalConditioner
from gnss_sdr_amd.sample_stream import FirFilter, PulseBlanking, SampleStream, convert_samples_device, direct_resample_device

N = 1 << 22
L = 32
BLANKING = dict(pfa=0.04, length=L, segments_est=12500, segments_reset=5000000)
# name, taps (0: no filter), IF, filter rate, resampler (rate after the filter, rate out) or None
SHAPES = (("ibyte 2^22, K=65, D=1, 25 -> 4 Msps, L=32", 65, 3.1e6, 25e6, (25e6, 4e6)),
          ("ibyte 2^22, no filter, no resampler, L=32", 0, 0.0, 1.0, None))


def taps_of(K):
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / 2.5)).astype(np.float32)
    return t / t.sum()


def block():
    """noise with bursts of 40 - 200 samples at 8x every 200 - 1 200 samples, as 8-bit items"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, 2)) * 10.0
    pos = int(rng.integers(200, 1201))
    while pos < N:
        x[pos:pos + int(rng.integers(40, 201))] *= 8.0
        pos += int(rng.integers(200, 1201))
    return np.clip(np.round(x), -127, 127).astype(np.int8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    d_raw = torch.from_numpy(block()).to(dev)
    d_x = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    d_y = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    d_z = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    d_r = torch.zeros(N + 2, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    say("conditioner push with the blanking stage vs the loose chain's four calls, one block of %d ibyte samples, %d runs per figure" % (N, a.reps))
    say("fused: device events around gsh_cond_time_push; loose: host clock around the synchronised sequence (the loose blanker synchronises inside)")
    say("%-46s %10s %10s %8s %10s %9s %12s %12s" % ("shape", "fused us", "loose us", "ratio", "outputs", "blanked", "fused GB/s", "loose GB/s"))
    for name, K, fc, fs, rs in SHAPES:
        taps = taps_of(K) if K else None
        fir = FirFilter(taps, 1, fc, fs, "gr_complex", device=0) if K else None
        pb = PulseBlanking(BLANKING["pfa"], L, BLANKING["segments_est"], BLANKING["segments_reset"], device=0)

        def loose(pb=pb, fir=fir):
            convert_samples_device(0, d_raw.data_ptr(), "ibyte", d_x.data_ptr(), N, hip_stream=st.cuda_stream)
            src = d_x
            if fir is not None:
                assert fir.process_device(d_x.data_ptr(), N, d_y.data_ptr(), d_y.numel(), hip_stream=st.cuda_stream) == N
                src = d_y
            st.synchronize()                                     # the blanker reads on its own stream
            done = pb.process_device(src.data_ptr(), N + 1, d_z.data_ptr())   # (the sample behind the block: zero, or an earlier run's: not part of a segment)
            assert done == N
            if rs is None:
                return done, d_z
            n_r, _cons = direct_resample_device(0, d_z.data_ptr(), 0, done, rs[0], rs[1], 0, d_r.data_ptr(), d_r.numel(), hip_stream=st.cuda_stream)
            st.synchronize()
            return n_r, d_r

        # ---- the two forms agree on the timed block before any ratio is quoted (fresh handles: stream position 0 and a fresh state on both sides)
        n_out, d_out = loose()
        st.synchronize()
        want = d_out.cpu().numpy()[:n_out].copy()
        ring = SampleStream(max(n_out, 2048), 1024, device=0)
        kw = dict(input_kind="ibyte", device=0, blanking=BLANKING)
        if K:
            kw.update(taps=taps, decimation=1, center_freq_hz=fc, sampling_freq_hz=fs)
        if rs is not None:
            kw.update(fs_in=rs[0], fs_out=rs[1])
        cond = SignalConditioner(ring, **kw)
        first, n_c = cond.push_device(d_raw.data_ptr(), N)
        same = n_c == n_out and np.array_equal(ring.read(first, n_c).view(np.uint32), want.view(np.uint32))
        state = cond.blanking_state()
        same = same and (float(state["noise_power_estimation"]), state["n_segments"], state["last_filtered"]) == pb.state()
        cond.close()
        ring.close()
        if not same:
            say("%s: the fused push and the loose chain DIFFER: not timed" % name)
            continue
        cond = SignalConditioner(None, **kw)   # position 0 and a fresh state again: the timed push is the one compared above
        M = N
        # algorithmic HBM bytes.  fused: 2 N in, 8 M + 4 M / L stage and energy writes, 8 M read again for the energies (they have a launch of their
        # own), at most 8 M read again by the gather, 8 n out.  loose: convert 2 + 8, FIR 8 + 8, blanker 8 + 8 + 8, gather 8 + 8 per output
        fused_bytes = 2 * N + 8 * M + 4 * M // L + 8 * M + 8 * min(M, n_out) + 8 * n_out
        loose_bytes = 10 * N + (16 * N if K else 0) + 24 * M + (16 * n_out if rs is not None else 0)
        cond.time_push(d_raw.data_ptr(), N, 3)
        for _ in range(3):
            loose()
        pairs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                loose()
            st.synchronize()
            t_l = (time.perf_counter() - t0) / a.reps * 1e6
            t_f = cond.time_push(d_raw.data_ptr(), N, a.reps) * 1e3
            pairs.append((t_f, t_l))
        for k, (t_f, t_l) in enumerate(pairs):
            say("%-46s %10.1f %10.1f %8.2f %10d %8.1f%% %12.0f %12.0f" % ("%s #%d" % (name, k + 1), t_f, t_l, t_l / t_f, n_out,
                                                                         100.0 * state["n_blanked"] / max(1, state["n_decided"]),
                                                                         fused_bytes / (t_f * 1e-6) / 1e9, loose_bytes / (t_l * 1e-6) / 1e9))
        faster = all(t_f < t_l for t_f, t_l in pairs)
        say("%s: outputs and blanking state equal bit for bit; fused %s in all three pairs" % (name, "FASTER" if faster else "NOT faster"))
        cond.close()
        pb.close()
        if fir is not None:
            fir.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0  # a completed measurement, whatever it says; any error raises


if __name__ == "__main__":
    sys.exit(main())
