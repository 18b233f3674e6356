"""GPU tests of pulse blanking as a stage of the signal conditioner's push (gsh_cond_set_blanking).

Yardsticks, both BIT FOR BIT (array_equal on the uint32 views):
  * the loose chain in one call per stage over the whole stream: gsh_convert_samples_device / gsh_unpack_device -> gsh_fir_process_device ->
    gsh_pb_process_device -> gsh_direct_resample_device (the loose blanker gets one extra trailing sample where M is a multiple of L: it leaves a segment
    that ends on the last offered item for its next call, the conditioner emits it);
  * PulseBlankingOracle + the oracle resampler, fed with the device FIR's own outputs.  That comparison is valid only where no decision is marginal:
    the oracle is walked segment by segment and every decided segment must have |ratio / thres - 1| >= 1e-4 (the seed of a case is chosen so that the
    oracle alone meets this; the 1e-4 is never changed).

Streams: complex Gaussian noise with bursts of 40 - 200 samples at 8x amplitude every 200 - 1 200 samples, about 400 segments.  pfa 0.04,
n_segments_est 20, n_segments_reset 50 unless the case says otherwise, so that the estimating branch, the "previous segment was blanked" branch and the
reset are all taken several times (asserted on the CPU).

Every case runs with three cut patterns -- one push; seeded random cuts with 1-sample pushes, pushes shorter than a segment and a zero-output push;
cuts exactly on segment boundaries -- and the three push flavours rotate.  The ring holds 4 096 samples, so the cut runs wrap several times.  One
departure, forced by a rule the conditioner keeps: a push that yields more samples than the ring's capacity is refused, so the one-push run has a ring
as large as its push (it is bound near the ring's end, so that push wraps too), and the cuts never complete more than 4 096 outputs at once.
"""
import ctypes as C
import mmap

import numpy as np
import pytest

import oracle
from oracle.pulse_blanking_oracle import PulseBlankingOracle

pytestmark = pytest.mark.gpu

CAPACITY = 4096
WINDOW = 512
BASE = CAPACITY - 301   # samples already in the ring when the conditioner is bound: every run wraps early, the short ones too
PFA = 0.04


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _taps(K, D):
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (2.5 * D))).astype(np.float32)
    return t / t.sum()


def _two_bit_cpx():
    from gnss_sdr_amd.sample_stream import PackedFormat
    return PackedFormat.from_signal_source("Two_Bit_Cpx_File_Signal_Source")


CASES = {
    "1 gr_complex L32": dict(kind="gr_complex", L=32, n=12801, seed=1),
    "2 ibyte inverted xlating K33 D2 L5": dict(kind="ibyte", inv=True, K=33, D=2, fc=1.2e6, fs=8e6, L=5, n=4011, seed=1),
    "3 ishort K65 25to4 L100": dict(kind="ishort", K=65, D=1, fc=0.0, fs=25e6, rs=(25e6, 4e6), L=100, est=8, reset=30, n=40037, seed=1),
    "4 two-bit packed xlating K17 4to5 L32": dict(kind="two_bit_cpx", K=17, D=1, fc=0.4e6, fs=4e6, rs=(4e6, 5e6), L=32, n=12810, seed=1),
    "5 gr_complex L1": dict(kind="gr_complex", L=1, n=403, seed=1),
    "6 gr_complex L4096": dict(kind="gr_complex", L=4096, est=2, reset=6, n=40 * 4096 + 1, seed=1),
    "7 gr_complex L32 ending on a segment": dict(kind="gr_complex", L=32, n=12800, seed=1),
}


def _blanking(case):
    return dict(pfa=PFA, length=case["L"], segments_est=case.get("est", 20), segments_reset=case.get("reset", 50))


def _signal(case):
    """the stream as complex128: unit-variance-per-component noise, bursts of 40 - 200 samples at 8x every 200 - 1 200 samples"""
    rng = np.random.default_rng(case["seed"])
    n = case["n"]
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    pos = int(rng.integers(200, 1201))
    while pos < n:
        x[pos:pos + int(rng.integers(40, 201))] *= 8.0
        pos += int(rng.integers(200, 1201))
    return x


def _raw(case):
    """(the raw array sliced by units, samples per unit, the decoded samples as the adapter yields them)"""
    x = _signal(case)
    kind = case["kind"]
    if kind == "gr_complex":
        raw = x.astype(np.complex64)
        return raw, 1, raw
    if kind in ("ibyte", "ishort"):
        scale, top, dt = (4.0, 127, np.int8) if kind == "ibyte" else (100.0, 32767, np.int16)
        raw = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -top, top).astype(dt)
        dec = (raw[:, 0].astype(np.float32) + 1j * raw[:, 1].astype(np.float32)).astype(np.complex64)
        return raw, 1, np.conj(dec) if case.get("inv") else dec
    # Two_Bit_Cpx: values +-1 below two sigma, +-3 above (noise mostly +-1, bursts +-3); field = ((v - 1) / 2) & 3, sample 0 = (bits 7:6, bits 5:4),
    # sample 1 = (bits 3:2, bits 1:0)
    q = lambda v: np.where(np.abs(v) < 2.0, 1, 3) * np.where(v < 0, -1, 1)
    vi, vq = q(x.real), q(x.imag)
    f = lambda v: ((v - 1) // 2) & 3
    raw = ((f(vi[0::2]) << 6) | (f(vq[0::2]) << 4) | (f(vi[1::2]) << 2) | f(vq[1::2])).astype(np.uint8)
    return raw, 2, (vi + 1j * vq).astype(np.complex64)


def _plan(case, n_in):
    from gnss_sdr_amd.conditioner import outputs_after
    return outputs_after(n_in, blanking=_blanking(case), **_chain_kw(case))


def _chain_kw(case):
    kw = dict(input_kind=_two_bit_cpx() if case["kind"] == "two_bit_cpx" else case["kind"], inverted_spectrum=case.get("inv", False))
    if "K" in case:
        kw.update(taps=_taps(case["K"], case["D"]), decimation=case["D"], center_freq_hz=case["fc"], sampling_freq_hz=case["fs"])
    if "rs" in case:
        kw.update(fs_in=case["rs"][0], fs_out=case["rs"][1])
    return kw


def walk_oracle(case, y):
    """PulseBlankingOracle over the filter outputs y, one segment per call (L + 1 items offered): (mitigated stream, mask, the oracle, figures)"""
    L = case["L"]
    b = _blanking(case)
    orc = PulseBlankingOracle(b["pfa"], L, b["segments_est"], b["segments_reset"])
    n_seg = len(y) // L
    yy = np.concatenate([y, np.zeros(1, np.complex64)])
    out, mask = [], np.zeros(n_seg, np.uint8)
    fig = dict(estimated=0, decided=0, blanked=0, after_blank=0, resets=0, margin=np.inf)
    for s in range(n_seg):
        seg = yy[s * L:(s + 1) * L + 1]
        estimating = orc.n_segments < orc.n_segments_est and not orc.last_filtered
        if estimating:
            fig["estimated"] += 1
        else:
            fig["decided"] += 1
            fig["after_blank"] += bool(orc.last_filtered)          # decided right after a blanked segment
            mag = (seg[:L].real * seg[:L].real + seg[:L].imag * seg[:L].imag).astype(np.float32)
            ratio = np.float32(np.sum(mag, dtype=np.float64)) / orc.noise_power_estimation
            fig["margin"] = min(fig["margin"], abs(float(ratio) / float(orc.thres) - 1.0))
        before = orc.n_segments
        z, done = orc.general_work(seg)
        assert done == L
        if not estimating:
            mask[s] = orc.last_filtered
            fig["resets"] += orc.n_segments == 1 and before > 0
        out.append(z)
    fig["blanked"] = int(mask.sum())
    return (np.concatenate(out) if out else np.zeros(0, np.complex64)), mask, orc, fig


_EXPECTED = {}


def _expected(gpu, torch, name):
    """computed once per case and shared, read-only: (case, raw, samples per unit, the loose chain's ring content, its blanker's state, the mask)"""
    if name in _EXPECTED:
        return _EXPECTED[name]
    import test_conditioner_gpu as plain
    from gnss_sdr_amd.sample_stream import PulseBlanking, direct_resample_device
    case = CASES[name]
    L, b = case["L"], _blanking(case)
    raw, per_unit, _dec = _raw(case)
    n = len(raw) * per_unit
    assert n == case["n"]
    dev = torch.device("cuda", gpu)
    # adapter and filter of the loose chain, as the plain conditioner's tests run them
    loose = {k: v for k, v in case.items() if k in ("inv", "K", "D", "fc", "fs")}
    loose["kind"] = _two_bit_cpx() if case["kind"] == "two_bit_cpx" else case["kind"]
    y = plain._loose_chain(gpu, torch, loose, raw, per_unit)
    M = (n + case.get("D", 1) - 1) // case.get("D", 1)
    assert len(y) == M
    Mp = (M // L) * L
    # the loose blanker over the whole stream in one call
    offered = np.concatenate([y, np.zeros(1, np.complex64)]) if M % L == 0 else y
    d_y = torch.from_numpy(offered).to(dev)
    d_z = torch.zeros(len(offered), dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    pb = PulseBlanking(b["pfa"], L, b["segments_est"], b["segments_reset"], device=gpu)
    assert pb.process_device(d_y.data_ptr(), len(offered), d_z.data_ptr()) == Mp
    state = pb.state() + (np.float32(pb.threshold),)
    pb.close()
    z = d_z.cpu().numpy()[:Mp].copy()
    if "rs" in case:
        fs_in, fs_out = case["rs"]
        d_r = torch.zeros(int(Mp * fs_out / fs_in) + 8, dtype=torch.complex64, device=dev)
        n_r, _cons = direct_resample_device(gpu, d_z.data_ptr(), 0, Mp, fs_in, fs_out, 0, d_r.data_ptr(), d_r.numel())
        torch.cuda.synchronize()
        exp = d_r.cpu().numpy()[:n_r].copy()
    else:
        exp = z
    assert len(exp) == _plan(case, n)
    # the oracle over the device FIR's outputs; valid where no decision is marginal
    z_o, mask, orc, fig = walk_oracle(case, y)
    print(name, fig)
    assert fig["margin"] >= 1e-4, (name, fig)
    assert fig["blanked"] >= 0.05 * fig["decided"] and fig["decided"] - fig["blanked"] >= 0.5 * fig["decided"], (name, fig)
    assert fig["estimated"] >= 3 and fig["after_blank"] >= 3 and fig["resets"] >= 3, (name, fig)
    assert np.array_equal(_bits(z_o), _bits(z)), name
    exp_o = oracle.direct_resampler(z_o, *case["rs"]) if "rs" in case else z_o
    assert np.array_equal(_bits(exp_o), _bits(exp)), name
    assert state[0] == float(orc.noise_power_estimation) and state[1:3] == (orc.n_segments, bool(orc.last_filtered)), (name, state)
    exp.setflags(write=False)
    mask.setflags(write=False)
    _EXPECTED[name] = (case, raw, per_unit, exp, state, mask)
    return _EXPECTED[name]


def _cuts(case, pattern, n_units, per_unit):
    """block sizes in units"""
    L, D = case["L"], case.get("D", 1)
    if pattern == "one":
        return [n_units]
    ratio = min(1.0, case["rs"][0] / case["rs"][1]) if "rs" in case else 1.0
    most = max(1, min(int(3000 * D * ratio) // per_unit, n_units // 6))   # at most 3 000 + L - 1 filter outputs, whole segments of them: <= 4 096 ring samples
    blocks, left = [], n_units
    if pattern == "segments":
        seg = L * D // per_unit                                  # L D inputs complete exactly one segment (per_unit divides L D in every case)
        assert seg * per_unit == L * D
        k = 0
        while left > 0:
            b = min(left, seg * (1 + k % max(1, most // seg)))
            blocks.append(b)
            left -= b
            k += 1
        return blocks
    rng = np.random.default_rng(case["seed"] + 77)
    while left > 0:
        kind = int(rng.integers(0, 4))
        b = 1 if kind == 0 else int(rng.integers(1, max(2, L * D // per_unit))) if kind == 1 else int(rng.integers(1, most + 1))
        b = min(b, left)
        blocks.append(b)
        left -= b
        if len(blocks) == 3:
            blocks.append(0)                                     # an empty push: no output, nothing moves
    return blocks


def _run(gpu, gsh, torch, name, pattern):
    """-> the last min(4 096, n) ring samples of the run; everything else is asserted here"""
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    case, raw, per_unit, exp, state, mask = _expected(gpu, torch, name)
    n_units = len(raw)
    blocks = _cuts(case, pattern, n_units, per_unit)
    assert sum(blocks) == n_units
    capacity, base = CAPACITY, BASE
    if pattern == "one":
        capacity = max(CAPACITY, len(exp) + (len(exp) & 1))
        base = capacity - 301
    else:
        assert len(blocks) > 3 and (pattern == "segments" or (1 in blocks and 0 in blocks))
    ring = SampleStream(capacity, WINDOW, device=gpu)
    assert ring.push(np.full(base, 3 - 4j, np.complex64)) == 0
    cond = SignalConditioner(ring, device=gpu, blanking=_blanking(case), **_chain_kw(case))
    dev = torch.device("cuda", gpu)
    d_raw = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    unit_bytes = raw[:1].nbytes
    mm = mmap.mmap(-1, (raw.nbytes + 4095) & ~4095)
    pinned = np.frombuffer(mm, raw.dtype, raw.size).reshape(raw.shape)
    pinned[...] = raw
    assert gsh.gsh_host_register(gpu, C.c_void_p(pinned.ctypes.data), len(mm)) == 0
    try:
        pos, wraps, zero_pushes, flavours = 0, 0, 0, set()
        for i, b in enumerate(blocks):
            j0, j1 = _plan(case, pos * per_unit), _plan(case, (pos + b) * per_unit)
            assert j1 - j0 <= capacity, (name, pattern, i, b)
            flavour = (i + len(name)) % 3
            flavours.add(flavour)
            if flavour == 0:
                first, n_out = cond.push(raw[pos:pos + b], b * per_unit)
            elif flavour == 1:
                first, n_out = cond.push_device(d_raw.data_ptr() + pos * unit_bytes, b * per_unit, hip_stream=side.cuda_stream)
                side.synchronize()
            else:
                first, n_out = cond.push_pinned_async(pinned[pos:pos + b], b * per_unit)
                ring.wait_copied_upto(first + n_out)
            pos += b
            assert (first, n_out) == (base + j0, j1 - j0), (name, pattern, i, first, n_out, j0, j1)
            assert cond.position() == (pos * per_unit, j1), (name, pattern, i)
            zero_pushes += n_out == 0
            if n_out:
                got = ring.read(first, n_out)
                assert np.array_equal(_bits(got), _bits(exp[j0:j1])), (name, pattern, i, int(np.argmax(got != exp[j0:j1])))
                wraps += first // capacity != (first + n_out - 1) // capacity
        assert pos == n_units and j1 == len(exp)
        assert wraps >= 1, (name, pattern, wraps)
        if pattern != "one":
            assert flavours == {0, 1, 2} and (zero_pushes >= 1 or pattern == "segments")
        st = cond.blanking_state()
        noise, n_segments, last_filtered, thres = state
        assert st["noise_power_estimation"].view(np.uint32) == np.float32(noise).view(np.uint32), (name, pattern, st, state)
        assert (st["n_segments"], st["last_filtered"]) == (n_segments, last_filtered), (name, pattern, st, state)
        assert st["thres"].view(np.uint32) == thres.view(np.uint32)
        assert (st["n_decided"], st["n_blanked"]) == (len(mask), int(mask.sum())), (name, pattern, st)
        lo, hi = ring.range()
        lo = max(lo, base, hi - CAPACITY)
        tail = ring.read(lo, hi - lo)
        assert np.array_equal(_bits(tail), _bits(exp[lo - base:hi - base]))
        return tail
    finally:
        cond.close()
        assert gsh.gsh_host_unregister(C.c_void_p(pinned.ctypes.data)) == 0
        ring.close()


@pytest.mark.parametrize("name", list(CASES))
def test_ring_equals_the_loose_chain_and_the_oracle_whatever_the_cuts(gpu, gsh, name):
    import torch
    tails = [_run(gpu, gsh, torch, name, pattern) for pattern in ("one", "random", "segments")]
    assert np.array_equal(_bits(tails[0]), _bits(tails[1])) and np.array_equal(_bits(tails[0]), _bits(tails[2]))
    case, raw, per_unit, exp, state, mask = _expected(gpu, torch, name)
    assert len(mask) >= 40 and np.any(exp != 0)
    if name.startswith("7"):
        assert len(exp) == case["n"]            # M is a multiple of L: the last segment is emitted


def test_refusals_move_nothing(gpu, gsh):
    """set_blanking after a push, a push larger than the ring, a foreign push in between, no bound ring: after each refusal the next good push gives the
    ring what the uncut run gives (neither position, history, carry nor the blanking state moved)"""
    import torch
    from gnss_sdr_amd import GshError, SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "2 ibyte inverted xlating K33 D2 L5"
    case, raw, per_unit, exp, state, mask = _expected(gpu, torch, name)
    plan = lambda n: _plan(case, n)
    ring = SampleStream(1201, WINDOW, device=gpu)
    cond = SignalConditioner(ring, device=gpu, blanking=_blanking(case), **_chain_kw(case))
    try:
        assert cond.push(raw[:503]) == (0, plan(503))
        done = plan(503)
        with pytest.raises(GshError) as e:
            cond.set_blanking(dict(length=7))
        assert e.value.code == 4
        with pytest.raises(GshError) as e:
            cond.set_blanking(None)
        assert e.value.code == 4
        assert plan(3503) - done > 1202
        with pytest.raises(GshError) as e:
            cond.push(raw[503:3503])
        assert e.value.code == 1 and "capacity" in str(e.value)
        assert cond.position() == (503, done) and ring.range() == (0, done)
        first, n_out = cond.push(raw[503:1204])
        assert (first, n_out) == (done, plan(1204) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        done += n_out
        assert ring.push(np.zeros(10, np.complex64)) == done
        with pytest.raises(GshError) as e:
            cond.push(raw[1204:2000])
        assert e.value.code == 4 and "someone else" in str(e.value)
        with pytest.raises(GshError) as e:
            cond.push_pinned_async(raw[1204:2000])
        assert e.value.code == 4
        assert cond.position() == (1204, done) and ring.range() == (0, done + 10)
        cond.bind(ring)
        first, n_out = cond.push(raw[1204:2001])
        assert (first, n_out) == (done + 10, plan(2001) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        done += n_out
        cond.bind(None)
        with pytest.raises(GshError) as e:
            cond.push(raw[2001:2100])
        assert e.value.code == 1
        cond.bind(ring)
        first, n_out = cond.push(raw[2001:])
        assert (first, n_out) == (done + 10, len(exp) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:]))
        st = cond.blanking_state()
        assert (float(st["noise_power_estimation"]), st["n_segments"], st["last_filtered"]) == state[:3]
        assert (st["n_decided"], st["n_blanked"]) == (len(mask), int(mask.sum()))
    finally:
        cond.close()
        ring.close()
    # bad values are refused before anything is allocated, and leave a handle that still works without the stage
    cond = SignalConditioner(None, device=gpu)
    try:
        for bad in (dict(pfa=0.0), dict(length=0), dict(length=4097), dict(segments_est=-1), dict(segments_reset=-1)):
            with pytest.raises(GshError) as e:
                cond.set_blanking(bad)
            assert e.value.code == 1
        with pytest.raises(GshError) as e:
            cond.blanking_state()
        assert e.value.code == 4
    finally:
        cond.close()


def test_time_push_leaves_everything_alone(gpu):
    import torch
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "3 ishort K65 25to4 L100"
    case, raw, per_unit, exp, state, mask = _expected(gpu, torch, name)
    plan = lambda n: _plan(case, n)
    ring = SampleStream(CAPACITY, WINDOW, device=gpu)
    cond = SignalConditioner(ring, device=gpu, blanking=_blanking(case), **_chain_kw(case))
    d_raw = torch.from_numpy(raw).to(torch.device("cuda", gpu))
    torch.cuda.synchronize()
    try:
        first, done = cond.push(raw[:5151])          # leaves a carry of 51 filter outputs and a history
        held, st0 = ring.read(0, done), cond.blanking_state()
        assert st0["n_decided"] == 51
        ms = cond.time_push(d_raw.data_ptr() + 4 * 5151, 9000, reps=3)
        assert ms > 0.0
        assert cond.position() == (5151, done) and ring.range() == (0, done)
        assert np.array_equal(_bits(ring.read(0, done)), _bits(held))
        assert cond.blanking_state() == st0
        pos = 5151
        while pos < len(raw):
            b = min(20000, len(raw) - pos)
            first, n_out = cond.push(raw[pos:pos + b])
            pos += b
            assert (first, n_out) == (done, plan(pos) - done)
            assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
            done += n_out
        st = cond.blanking_state()
        assert (float(st["noise_power_estimation"]), st["n_segments"], st["last_filtered"]) == state[:3]
    finally:
        cond.close()
        ring.close()


@pytest.mark.parametrize("name", ["3 ibyte inverted K33 D2 xlating decimating", "6 packed four-bit complex K33 D2"])
def test_a_handle_with_the_stage_turned_off_gives_the_plain_rings(gpu, gsh, name):
    """set_blanking(...) then set_blanking(NULL) before the first push: the rings of the plain conditioner (tests/test_conditioner_gpu.py's table)"""
    import torch
    import test_conditioner_gpu as plain
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    case, raw, per_unit, exp = plain._expected(gpu, torch, name)
    ring = SampleStream(3001, WINDOW, device=gpu)
    cond = plain._conditioner(gpu, ring, case)
    try:
        cond.set_blanking(dict(length=5, segments_est=2, segments_reset=3))
        cond.set_blanking(None)
        with pytest.raises(GshError):
            cond.blanking_state()
        pos = 0
        for b in [1, 7, 100, 4099, 3] + [2000] * 4:
            b = min(b, len(raw) - pos)
            j0, j1 = plain._count_after(case, pos * per_unit), plain._count_after(case, (pos + b) * per_unit)
            assert cond.push(raw[pos:pos + b], b * per_unit) == (j0, j1 - j0)
            pos += b
            if j1 > j0:
                assert np.array_equal(_bits(ring.read(j0, j1 - j0)), _bits(exp[j0:j1])), (name, pos)
        assert pos == len(raw) and j1 == len(exp)
    finally:
        cond.close()
        ring.close()
