"""GPU tests of the signal conditioner (gsh_cond_*): adapter, FIR and resampler in one pass per block, straight into a ring.

Yardstick: the loose chain the project already holds to float64 and to the reference -- gsh_convert_samples_device or gsh_unpack_device ->
FirFilter.process_device -> direct_resample_device -- run ONCE over the whole stream.  After every push the ring must hold those samples index
for index and BIT FOR BIT (array_equal on the uint32 views, no tolerance), wherever the stream is cut.

Blocks: [1, 7, 100, 4099, 3, 5000, rest] -- shorter than D and than K - 1, a history that spans several pushes, pushes of several 1 024-output tiles.
The ring is short (capacity 3 001, window 512) so that it wraps inside pushes.  Two departures, both forced by rules the conditioner keeps:
  * a push that yields more samples than the ring's capacity is refused (tested below), so the cases whose 5 000-sample block yields more than
    3 001 outputs (no decimation, or one output per packed byte) run on a ring of 5 003, which still wraps inside the 5 000-sample push;
  * a packed block is whole input items; for the family with four samples per byte (NSR) the block list counts bytes, the smallest whole unit.
"""
import ctypes as C
import mmap

import numpy as np
import pytest

import oracle
from helpers import synth_gps_l1_stream

pytestmark = pytest.mark.gpu

BLOCKS = [1, 7, 100, 4099, 3, 5000]
N_UNITS = 12007
WINDOW = 512
BASE = 2000         # samples already in the ring when the conditioner is bound: every case then wraps the ring inside a push


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _taps(K, D):
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (2.5 * D))).astype(np.float32)
    return t / t.sum()


def _packed(name, **kw):
    from gnss_sdr_amd.sample_stream import PackedFormat
    return PackedFormat.from_signal_source(name, **kw)


def _cases():
    return {
        "1 gr_complex as it is": dict(kind="gr_complex"),
        "2 gr_complex K5": dict(kind="gr_complex", K=5, D=1, fc=0.0, fs=4e6),
        "3 ibyte inverted K33 D2 xlating decimating": dict(kind="ibyte", inv=True, K=33, D=2, fc=1.2e6, fs=8e6, rs=(4e6, 2.5e6)),
        "4 ishort K257 D8 xlating interpolating": dict(kind="ishort", K=257, D=8, fc=-3.3e6, fs=32e6, rs=(4e6, 4.092e6)),
        "5 ibyte resampler alone": dict(kind="ibyte", rs=(25e6, 4e6)),
        "6 packed four-bit complex K33 D2": dict(kind=_packed("Four_Bit_Cpx_File_Signal_Source"), K=33, D=2, fc=0.0, fs=8e6),
        "7 packed real NSR K65 D4 IF fs/4": dict(kind=_packed("Nsr_File_Signal_Source"), K=65, D=4, fc=4e6, fs=16e6),
        "8 real int16 K33 D2 xlating": dict(kind="short", K=33, D=2, fc=1e6, fs=8e6),
    }


def _raw(case, seed, n_units=N_UNITS):
    """(raw array sliced by units, samples per unit)"""
    rng = np.random.default_rng(seed)
    kind = case["kind"]
    if kind == "gr_complex":
        return (rng.standard_normal(n_units) + 1j * rng.standard_normal(n_units)).astype(np.complex64), 1
    if kind == "ibyte":
        return rng.integers(-100, 101, (n_units, 2)).astype(np.int8), 1
    if kind == "ishort":
        return rng.integers(-2000, 2001, (n_units, 2)).astype(np.int16), 1
    if kind == "short":
        return rng.integers(-2000, 2001, n_units).astype(np.int16), 1
    return rng.integers(0, 256, n_units).astype(np.uint8), kind.samples_per_byte


def _loose_chain(gpu, torch, case, raw, per_unit):
    """the expected ring content: one call per stage over the whole stream"""
    from gnss_sdr_amd.sample_stream import FirFilter, PackedFormat, convert_samples_device, direct_resample_device, unpack_device
    dev = torch.device("cuda", gpu)
    kind = case["kind"]
    n = len(raw) * per_unit
    d_raw = torch.from_numpy(raw).to(dev)
    fir_kind = "gr_complex"
    if isinstance(kind, PackedFormat):
        cplx = kind.is_complex
        d_x = torch.zeros(n, dtype=torch.complex64 if cplx else torch.float32, device=dev)
        unpack_device(gpu, kind, d_raw.data_ptr(), 0, n, d_x.data_ptr(), inverted_spectrum=case.get("inv", False))
        fir_kind = "gr_complex" if cplx else "float"
    elif kind == "short":
        d_x, fir_kind = d_raw, "short"
    else:
        d_x = torch.zeros(n, dtype=torch.complex64, device=dev)
        convert_samples_device(gpu, d_raw.data_ptr(), kind, d_x.data_ptr(), n, inverted_spectrum=case.get("inv", False))
    torch.cuda.synchronize()
    if "K" in case:
        D = case["D"]
        d_y = torch.zeros(n // D + 2, dtype=torch.complex64, device=dev)
        f = FirFilter(_taps(case["K"], D), D, case["fc"], case["fs"], fir_kind, device=gpu)
        n_f = f.process_device(d_x.data_ptr(), n, d_y.data_ptr(), d_y.numel())
        f.close()
        assert n_f == (n + D - 1) // D
    else:
        d_y, n_f = d_x, n
    if "rs" in case:
        fs_in, fs_out = case["rs"]
        d_z = torch.zeros(int(n_f * fs_out / fs_in) + 8, dtype=torch.complex64, device=dev)
        n_z, _cons = direct_resample_device(gpu, d_y.data_ptr(), 0, n_f, fs_in, fs_out, 0, d_z.data_ptr(), d_z.numel())
        torch.cuda.synchronize()
        assert n_z < d_z.numel()
        return d_z.cpu().numpy()[:n_z].copy()
    torch.cuda.synchronize()
    return d_y.cpu().numpy()[:n_f].copy()


def _filter_index(case, j):
    """resampler.hip's head: the filter output that ring sample j takes (exact integers)"""
    if "rs" not in case:
        return j
    fs_in, fs_out = case["rs"]
    two_32 = 1 << 32
    if fs_in >= fs_out:
        step = int(np.floor(two_32 * fs_out / fs_in))
        return -((-j * two_32) // step)
    step = int(np.floor(two_32 * fs_in / fs_out))
    return ((j + 1) * step) >> 32


def _count_after(case, n_in):
    """ring samples complete after n_in input samples: those whose filter output has its newest input"""
    D = case.get("D", 1)
    m = (n_in + D - 1) // D
    j = 0 if "rs" not in case else max(0, int(m * case["rs"][1] / case["rs"][0]) - 3)
    if "rs" not in case:
        return m
    while _filter_index(case, j) < m:
        j += 1
    return j


def _conditioner(gpu, ring, case):
    from gnss_sdr_amd import SignalConditioner
    kw = dict(input_kind=case["kind"], inverted_spectrum=case.get("inv", False), device=gpu)
    if "K" in case:
        kw.update(taps=_taps(case["K"], case["D"]), decimation=case["D"], center_freq_hz=case["fc"], sampling_freq_hz=case["fs"])
    if "rs" in case:
        kw.update(fs_in=case["rs"][0], fs_out=case["rs"][1])
    return SignalConditioner(ring, **kw)


_EXPECTED = {}


def _expected(gpu, torch, name, n_units=N_UNITS):
    """(case, raw, samples per unit, the loose chain's output) -- computed once per case and shared"""
    if (name, n_units) not in _EXPECTED:
        case = _cases()[name]
        raw, per_unit = _raw(case, seed=sum(map(ord, name)), n_units=n_units)
        exp = _loose_chain(gpu, torch, case, raw, per_unit)
        exp.setflags(write=False)
        _EXPECTED[(name, n_units)] = (case, raw, per_unit, exp)
    return _EXPECTED[(name, n_units)]


@pytest.mark.parametrize("name", list(_cases()))
def test_ring_equals_the_loose_chain_bit_for_bit_whatever_the_cuts(gpu, gsh, name):
    import torch
    from gnss_sdr_amd.sample_stream import SampleStream
    case, raw, per_unit, exp = _expected(gpu, torch, name)
    assert len(exp) == _count_after(case, len(raw) * per_unit) and len(exp) > 700 and np.any(exp != 0)
    blocks = BLOCKS + [len(raw) - sum(BLOCKS)]
    most = max(_count_after(case, (sum(blocks[:i + 1])) * per_unit) - _count_after(case, sum(blocks[:i]) * per_unit) for i in range(len(blocks)))
    capacity = 3001 if most <= 3001 else 5003
    ring = SampleStream(capacity, WINDOW, device=gpu)
    twin = SampleStream(capacity, WINDOW, device=gpu) if name.startswith("1") else None
    capacity += capacity & 1   # (gsh_stream_create keeps an even number of samples)
    junk = np.full(BASE, 3 - 4j, np.complex64)
    assert ring.push(junk) == 0
    cond = _conditioner(gpu, ring, case)
    dev = torch.device("cuda", gpu)
    d_raw = torch.from_numpy(raw).to(dev)
    unit_bytes = raw[:1].nbytes
    # the page-locked copy of the stream for the asynchronous pushes: whole pages of its own (registering the pages around a heap array would lock
    # its neighbours too)
    mm = mmap.mmap(-1, (raw.nbytes + 4095) & ~4095)
    pinned = np.frombuffer(mm, raw.dtype, raw.size).reshape(raw.shape)
    pinned[...] = raw
    assert gsh.gsh_host_register(gpu, C.c_void_p(pinned.ctypes.data), len(mm)) == 0
    try:
        if twin is not None:
            twin.push(junk)
        pos, wrapped_inside = 0, 0
        for i, b in enumerate(blocks):
            j0, j1 = _count_after(case, pos * per_unit), _count_after(case, (pos + b) * per_unit)
            if i % 3 == 0:
                first, n_out = cond.push(raw[pos:pos + b], b * per_unit)
            elif i % 3 == 1:
                first, n_out = cond.push_device(d_raw.data_ptr() + pos * unit_bytes, b * per_unit)
            else:
                first, n_out = cond.push_pinned_async(pinned[pos:pos + b], b * per_unit)
                ring.wait_copied_upto(first + n_out)
            pos += b
            assert (first, n_out) == (BASE + j0, j1 - j0), (name, i, first, n_out, j0, j1)
            assert cond.position() == (pos * per_unit, j1), (name, i)
            assert ring.range() == (max(0, BASE + j1 - capacity), BASE + j1), (name, i)
            if n_out:
                got = ring.read(first, n_out)
                assert np.array_equal(_bits(got), _bits(exp[j0:j1])), (name, i, int(np.argmax(got != exp[j0:j1])))
                wrapped_inside += first // capacity != (first + n_out - 1) // capacity
            if twin is not None:
                assert twin.push(raw[pos - b:pos]) == first
                assert np.array_equal(_bits(twin.read(first, n_out)), _bits(ring.read(first, n_out)))
        assert pos == len(raw) and j1 == len(exp)
        assert wrapped_inside >= 1, name
        # everything of the conditioner's that is still resident, in one read over the ring's end
        lo_i, hi_i = ring.range()
        lo_i = max(lo_i, BASE)
        assert np.array_equal(_bits(ring.read(lo_i, hi_i - lo_i)), _bits(exp[lo_i - BASE:hi_i - BASE]))
        if twin is not None:
            assert np.array_equal(_bits(exp), _bits(raw))   # case 1 is the input itself
    finally:
        cond.close()
        assert gsh.gsh_host_unregister(C.c_void_p(pinned.ctypes.data)) == 0
        ring.close()
        if twin is not None:
            twin.close()


def test_refusals_move_nothing(gpu, gsh):
    """each refusal is followed by a successful push whose result still matches the loose chain: neither position nor history moved"""
    import torch
    from gnss_sdr_amd import GshError, SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "3 ibyte inverted K33 D2 xlating decimating"
    case, raw, per_unit, exp = _expected(gpu, torch, name)
    ring = SampleStream(3001, WINDOW, device=gpu)
    cond = _conditioner(gpu, ring, case)
    try:
        assert cond.push(raw[:1000]) == (0, _count_after(case, 1000))
        done = _count_after(case, 1000)
        # more outputs than the ring's capacity: 11 000 samples -> 3 438
        assert _count_after(case, 12000) - done > 3001
        with pytest.raises(GshError) as e:
            cond.push(raw[1000:12000])
        assert e.value.code == 1 and "capacity" in str(e.value)
        assert cond.position() == (1000, done) and ring.range() == (0, done)
        first, n_out = cond.push(raw[1000:2000])
        assert (first, n_out) == (done, _count_after(case, 2000) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        done += n_out
        # someone else pushes into the ring between two conditioner pushes
        assert ring.push(np.zeros(10, np.complex64)) == done
        with pytest.raises(GshError) as e:
            cond.push(raw[2000:3000])
        assert e.value.code == 4 and "someone else" in str(e.value)
        with pytest.raises(GshError) as e:
            cond.push_pinned_async(raw[2000:3000])
        assert e.value.code == 4
        assert cond.position() == (2000, done) and ring.range() == (0, done + 10)
        cond.bind(ring)   # the next output goes where the ring stands now
        first, n_out = cond.push(raw[2000:3000])
        assert (first, n_out) == (done + 10, _count_after(case, 3000) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        # no ring bound
        cond.bind(None)
        with pytest.raises(GshError) as e:
            cond.push(raw[3000:3100])
        assert e.value.code == 1
    finally:
        cond.close()
        ring.close()
    # a partial packed item: six samples of a family with four per byte
    name = "7 packed real NSR K65 D4 IF fs/4"
    case, raw, per_unit, exp = _expected(gpu, torch, name)
    ring = SampleStream(5003, WINDOW, device=gpu)
    cond = _conditioner(gpu, ring, case)
    try:
        assert cond.push(raw[:50]) == (0, 50)
        with pytest.raises(GshError) as e:
            cond.push(raw[50:52], 6)
        assert e.value.code == 1
        assert cond.position() == (200, 50) and ring.range() == (0, 50)
        assert cond.push(raw[50:150]) == (50, 100)
        assert np.array_equal(_bits(ring.read(0, 150)), _bits(exp[:150]))
    finally:
        cond.close()
        ring.close()
    # real input without a filter is refused when the handle is created
    for kind in ("short", _packed("Nsr_File_Signal_Source")):
        with pytest.raises(GshError) as e:
            SignalConditioner(None, input_kind=kind, device=gpu)
        assert e.value.code == 1 and "without a filter" in str(e.value)


def test_time_push_leaves_the_state_alone(gpu):
    import torch
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "3 ibyte inverted K33 D2 xlating decimating"
    case, raw, per_unit, exp = _expected(gpu, torch, name)
    ring = SampleStream(3001, WINDOW, device=gpu)
    cond = _conditioner(gpu, ring, case)
    d_raw = torch.from_numpy(raw).to(torch.device("cuda", gpu))
    try:
        first, done = cond.push(raw[:1501])
        held = ring.read(0, done)
        ms = cond.time_push(d_raw.data_ptr() + 2 * 1501, 4000, reps=3)
        assert ms > 0.0
        assert cond.position() == (1501, done) and ring.range() == (0, done)
        assert np.array_equal(_bits(ring.read(0, done)), _bits(held))
        first, n_out = cond.push(raw[1501:5501])
        assert (first, n_out) == (done, _count_after(case, 5501) - done)
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
    finally:
        cond.close()
        ring.close()


def test_tracking_loop_on_a_conditioned_ring(gpu):
    """GPS L1 C/A at a +2 MHz IF, 8 Msps, 8-bit items -> xlating low-pass, decimation 2 -> a 4 Msps ring that a tracking loop follows.  The records
    equal, byte for byte, those of a loop fed from a ring filled with the loose chain's output, and the loop locks (the project's bar for the loop:
    mean Doppler of the last 80 periods within 1.5 Hz, test_tracking_loop_gpu.py)."""
    import torch
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import FirFilter, SampleStream, convert_samples_device, firdes_low_pass
    from gnss_sdr_amd.tracking_loop import TrackingLoop, trk_conf
    fs_in, fs, n, epochs, D = 8e6, 4e6, 4000, 300, 2
    prn, fd, cph = 9, 1350.0, 417.3
    total_in = (epochs + 3) * n * D
    x = synth_gps_l1_stream(total_in, fs_in, [prn], [fd], [cph], cn0_dbhz=47.0, seed_noise=41)
    x = x * (1j ** (np.arange(total_in) % 4)).astype(np.complex64)            # exp(j 2 pi 2e6 / 8e6 t): the +2 MHz IF
    x8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 25.0), -127, 127).astype(np.int8)
    taps = firdes_low_pass(1.0, fs_in, 1.6e6, 1.0e6)
    delay = (len(taps) - 1) / 2.0 / D                                           # group delay in ring samples
    f_code = 1.023e6 * (1 + fd / 1575.42e6)
    start = int(round((1023.0 - cph) / f_code * fs + delay))
    dev = torch.device("cuda", gpu)
    d_x8 = torch.from_numpy(x8).to(dev)
    # the loose chain over the whole stream
    d_x = torch.zeros(total_in, dtype=torch.complex64, device=dev)
    convert_samples_device(gpu, d_x8.data_ptr(), "ibyte", d_x.data_ptr(), total_in)
    d_y = torch.zeros(total_in // D + 2, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    f = FirFilter(taps, D, 2e6, fs_in, "gr_complex", device=gpu)
    total = f.process_device(d_x.data_ptr(), total_in, d_y.data_ptr(), d_y.numel())
    f.close()
    assert total == total_in // D
    kw = dict(fs_in=fs, vector_length=n, pll_bw_hz=35.0, dll_bw_hz=3.0, enable_lock_detectors=1)
    recs = []
    for fused in (True, False):
        ring = SampleStream(23 * n + 7, 2 * n, device=gpu)
        loop = TrackingLoop(trk_conf(**kw), 1, 1023, device=gpu)
        cond = SignalConditioner(ring, input_kind="ibyte", taps=taps, decimation=D, center_freq_hz=2e6, sampling_freq_hz=fs_in, device=gpu) if fused else None
        try:
            loop.set_stream_ring(ring)
            loop.start(0, oracle.ca_code(prn), start, 0, fd + 6.0)
            rec, pushed, blk = [], 0, (9 * n + n // 2) * D + 1
            while pushed < total_in:
                m = min(blk, total_in - pushed)
                if fused:
                    first, n_out = cond.push(x8[pushed:pushed + m])
                else:
                    j0, j1 = (pushed + D - 1) // D, (pushed + m + D - 1) // D
                    first, n_out = ring.push_device(d_y.data_ptr() + 8 * j0, j1 - j0), j1 - j0
                assert (first, n_out) == ((pushed + D - 1) // D, (pushed + m + D - 1) // D - (pushed + D - 1) // D)
                pushed += m
                r, done = loop.run(12)
                rec += r[0]
        finally:
            if cond is not None:
                cond.close()
            loop.close()
            ring.close()
        recs.append(rec)
    assert len(recs[0]) == len(recs[1]) >= epochs - 10
    a = b"".join(bytes(memoryview(r)) for r in recs[0])
    b = b"".join(bytes(memoryview(r)) for r in recs[1])
    assert a == b, "records of the loop on the conditioned ring differ from those on the loose chain's output"
    err = np.mean([r.carrier_doppler_hz for r in recs[0][-80:]]) - fd
    print(f"mean Doppler error of the last 80 periods: {err:+.3f} Hz")
    assert abs(err) < 1.5
