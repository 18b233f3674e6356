"""GPU tests of the packed front-end ingest (gsh_packed_format: csrc/packed_unpack.hip, the packed pushes of csrc/sample_stream.hip and
csrc/stream_group.hip, the packed FIR of csrc/fir_filter.hip).  The checker is tests/packed_reference.py, the numpy restatement of the
reference's unpack blocks and GNU Radio conversions (pinned to the reference's own blocks by tests/test_packed_formats.py).  Every comparison
is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import packed_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_RCCL = os.path.join(ROOT, "tests", "host", "libfake_rccl.so")


def _fmt(src, channel=None):
    from gnss_sdr_amd.sample_stream import PackedFormat
    f = PackedFormat.from_signal_source(src[0], **src[1])
    return f if channel is None else f.with_channel(channel)


def _pattern(src, rng, random_bytes):
    """every byte value (every 16-bit item for short items), then random bytes"""
    every = np.arange(65536, dtype="<u2").view(np.uint8) if src[1].get("item_type") == "short" else np.arange(256, dtype=np.uint8)
    return np.concatenate([every, rng.integers(0, 256, random_bytes, dtype=np.uint8)])


def _expect(src, data, inverted=False):
    x = R.source_output(src[0], data, **src[1])
    return np.conj(x).astype(np.complex64) if inverted else x


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("inverted", [False, True], ids=["plain", "inverted_spectrum"])
@pytest.mark.parametrize("src", R.COMPLEX_SOURCES, ids=R.source_id)
def test_push_packed_equals_reference_and_unpacked_pairs(gpu, src, inverted):
    from gnss_sdr_amd.sample_stream import SampleStream
    fmt = _fmt(src)
    data = _pattern(src, np.random.default_rng(11), 4 << 20)
    exp = _expect(src, data, inverted)
    n = exp.size
    assert n == data.size * fmt.samples_per_byte
    ring = SampleStream(n + 2, 4096, device=gpu)
    assert ring.push_packed(fmt, data, inverted) == 0
    got = ring.read(0, n)
    assert np.array_equal(_bits(got), _bits(exp))
    # today's path: the host unpacks to int8 / int16 pairs and pushes those (ibyte / ishort, conjugate for inverted_spectrum)
    plain = R.source_output(src[0], data, **src[1])
    wide = src[0] != "Two_Bit_Packed_File_Signal_Source"
    pairs = np.stack([plain.real, plain.imag], axis=1).astype(np.int16 if wide else np.int8)
    ref = SampleStream(n + 2, 4096, device=gpu)
    ref.push(pairs, "ishort" if wide else "ibyte", inverted)
    assert np.array_equal(_bits(ref.read(0, n)), _bits(got))
    ring.close()
    ref.close()


def _whole_item_blocks(fmt, rng, total_bytes, sizes):
    """uneven block sizes in bytes, whole items"""
    isz = 2 if (fmt.item_size == 2 and fmt.big_endian_items) else 1
    out, pos = [], 0
    for s in sizes:
        s = min(s - s % isz, total_bytes - pos)
        out.append((pos, s))
        pos += s
    return out


@pytest.mark.parametrize("src", [R.COMPLEX_SOURCES[7], R.COMPLEX_SOURCES[-3], R.COMPLEX_SOURCES[-1]], ids=R.source_id)
def test_uneven_pushes_wrap_an_odd_ring(gpu, src):
    from gnss_sdr_amd.sample_stream import SampleStream
    fmt = _fmt(src)
    rng = np.random.default_rng(3)
    cap, win = 40001, 9000                       # not a multiple of 4 (the ring rounds it to 40002): wraps fall inside packed bytes
    data = rng.integers(0, 256, 200000, dtype=np.uint8)
    exp = _expect(src, data)
    spb = fmt.samples_per_byte
    sizes = [4501, 2, 0, 8191, 3333, 16384, 7, 20000] * 10
    blocks = _whole_item_blocks(fmt, rng, data.size, sizes)
    ring, ref = SampleStream(cap, win, device=gpu), SampleStream(cap, win, device=gpu)
    total = 0
    for pos, nbytes in blocks:
        if pos >= data.size:
            break
        assert ring.push_packed(fmt, data[pos:pos + nbytes]) == total
        total += nbytes * spb
        lo, hi = ring.range()
        assert hi == total and lo == max(0, total - cap - (cap & 1))
        for start in sorted({lo, hi - min(win, hi - lo), max(lo, hi - win // 3 - 1)}):
            m = min(win, hi - start)
            assert np.array_equal(_bits(ring.read(start, m)), _bits(exp[start:start + m])), (pos, start)
    assert total > 4 * cap                       # wrapped several times
    # one-shot pushes of the same stretch into a second ring: identical resident windows, also across the capacity boundary and the mirror
    ref.seek(total - cap // 2 - cap // 2 % 4)
    first = ref.range()[1]
    ref.push_packed(fmt, data[first // spb:total // spb])
    lo, hi = ref.range()
    for start in range(max(lo, ring.range()[0]), hi - win, 3777):
        assert np.array_equal(_bits(ring.read(start, win)), _bits(ref.read(start, win))), start
    ring.close()
    ref.close()


def test_device_and_pinned_pushes_equal_the_host_push(gpu, gsh):
    torch = pytest.importorskip("torch")
    import ctypes as C
    from gnss_sdr_amd.sample_stream import SampleStream
    src = R.COMPLEX_SOURCES[-2]                  # Four_Bit_Cpx iq
    fmt = _fmt(src)
    rng = np.random.default_rng(9)
    cap, win = 300000, 20000
    page = 4096
    raw = np.zeros(600000 + 2 * page, np.uint8)
    off = (-raw.ctypes.data) % page
    data = raw[off:off + 600000]                 # page-aligned, registered once (a GNU Radio buffer re-used for the whole run)
    data[:] = rng.integers(0, 256, data.size, dtype=np.uint8)
    locked = (data.size + page - 1) // page * page
    assert gsh.gsh_host_register(gpu, C.c_void_p(data.ctypes.data), locked) == 0
    d_data = torch.from_numpy(data.copy()).to(torch.device("cuda", gpu))
    host, dev, pinned = (SampleStream(cap, win, device=gpu) for _ in range(3))
    try:
        pos = 0
        for k, nb in enumerate([70001, 1, 0, 129999, 50000, 99999, 150000, 100000]):
            blk = data[pos:pos + nb]
            a = host.push_packed(fmt, blk, bool(k & 1))
            b = dev.push_packed_device(fmt, d_data.data_ptr() + pos, nb, bool(k & 1))
            c = pinned.push_packed_pinned_async(fmt, blk, bool(k & 1))
            assert a == b == c == pos
            pos += nb
            if k % 3 == 2:
                assert pinned.wait_copied_upto(pos) >= pos   # the DMA out of `data` below pos is done
        pinned.wait_copied()
        pinned.wait()
        torch.cuda.synchronize()
        lo, hi = host.range()
        assert dev.range() == pinned.range() == (lo, hi) == (pos - cap, pos)
        for start in (lo, lo + 12345, hi - win):
            h = host.read(start, win)
            assert np.array_equal(_bits(dev.read(start, win)), _bits(h)) and np.array_equal(_bits(pinned.read(start, win)), _bits(h))
        exp = _expect(src, data[hi - win:hi], inverted=True)   # (the last block was pushed with inverted_spectrum)
        assert np.array_equal(_bits(host.read(hi - win, win)), _bits(exp))
    finally:
        for s in (host, dev, pinned):
            s.close()
        assert gsh.gsh_host_unregister(C.c_void_p(data.ctypes.data)) == 0


@pytest.mark.parametrize("src", R.REAL_SOURCES + R.COMPLEX_SOURCES[-3:], ids=R.source_id)
def test_unpack_device_equals_reference(gpu, src):
    torch = pytest.importorskip("torch")
    from gnss_sdr_amd.sample_stream import unpack_device
    dev = torch.device("cuda", gpu)
    data = _pattern(src, np.random.default_rng(21), 1 << 20)
    exp = R.source_output(src[0], data, **src[1])
    d_src = torch.from_numpy(data).to(dev)
    channels = range(4) if src[0].startswith("NTLab") else [None]
    for ch in channels:
        fmt = _fmt(src, ch)
        e = exp[ch] if ch is not None else exp
        n = e.size
        for first, m in ((0, n), (3, n - 7), (n // 2 + 1, 13), (5, 2)):   # starts and ends inside a byte; blocks shorter than a dword
            # destination 8 (complex) / 4 (real) bytes past a 16-byte boundary: the lanes fall back from 16-byte stores
            out = torch.zeros(m * (2 if fmt.is_complex else 1) + 4, dtype=torch.float32, device=dev)
            lead = 2 if fmt.is_complex else 1
            unpack_device(gpu, fmt, d_src.data_ptr(), first, m, out.data_ptr() + 4 * lead)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            got = o[lead:lead + 2 * m].view(np.complex64) if fmt.is_complex else o[lead:lead + m]
            assert np.array_equal(_bits(got), _bits(e[first:first + m])), (ch, first, m)


FIR_SOURCES = [R.REAL_SOURCES[0], R.REAL_SOURCES[-2], R.REAL_SOURCES[-1]]   # Two_Bit_Packed real (byte), Nsr, NTLab


@pytest.mark.parametrize("D,fc", [(1, 0.0), (8, 0.0), (1, 3.3e6), (8, 5.5e6)])
@pytest.mark.parametrize("src", FIR_SOURCES, ids=R.source_id)
def test_packed_fir_equals_float_fir(gpu, src, D, fc):
    torch = pytest.importorskip("torch")
    from gnss_sdr_amd.sample_stream import FirFilter, firdes_low_pass
    dev = torch.device("cuda", gpu)
    fs = 20.48e6
    taps = firdes_low_pass(1.0, fs, 1.0e6, 0.5e6)
    data = np.random.default_rng(D).integers(0, 256, 150000, dtype=np.uint8)   # one buffer shared by every NTLab channel
    exp = R.source_output(src[0], data, **src[1])
    d_data = torch.from_numpy(data).to(dev)
    for ch in (range(4) if src[0].startswith("NTLab") else [None]):
        fmt = _fmt(src, ch)
        x = exp[ch] if ch is not None else exp
        spb = fmt.samples_per_byte
        d_x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        outs = []
        for packed in (True, False):
            f = FirFilter(taps, D, fc, fs, fmt if packed else "float", device=gpu)
            cap = x.size // D + 2
            d_y = torch.zeros(cap, dtype=torch.complex64, device=dev)
            pos, out = 0, 0
            for nb in [1, 2, 17, 3000, 5, 40000, 1, 77777, 29197]:   # uneven blocks (bytes), the first ones shorter than the filter
                nb = min(nb, data.size - pos)
                if packed:
                    out += f.process_device(d_data.data_ptr() + pos, nb * spb, d_y.data_ptr() + 8 * out, cap - out)
                else:
                    out += f.process_device(d_x.data_ptr() + 4 * pos * spb, nb * spb, d_y.data_ptr() + 8 * out, cap - out)
                pos += nb
            assert pos == data.size
            torch.cuda.synchronize()
            outs.append(d_y.cpu().numpy()[:out])
            f.close()
        assert outs[0].size == (x.size + D - 1) // D
        assert np.array_equal(_bits(outs[0]), _bits(outs[1])), ch


def _group_blocks(rng):
    return [rng.integers(0, 256, nb, dtype=np.uint8) for nb in (4500, 1, 4095, 10000, 0, 389, 16666, 2048, 12001)]


@pytest.mark.parametrize("rccl", [False, True], ids=["no_exchange", "one_rank_rccl"])
@pytest.mark.parametrize("mode", ["broadcast", "scatter_allgather"])
def test_group_of_one_packed_push_equals_local_push(gpu, mode, rccl):
    from gnss_sdr_amd.sample_stream import SampleStream, StreamGroup
    fmt = _fmt(R.COMPLEX_SOURCES[-3])            # Two_Bit_Cpx: 2 samples per byte
    cap, win = 40001, 9000
    g = StreamGroup.local([gpu], cap, win, mode=mode, force_rccl=rccl)
    ring, ref = g.ring(0), SampleStream(cap, win, device=gpu)
    total, blocks = 0, 0
    for b in _group_blocks(np.random.default_rng(4)):
        assert g.push_packed(fmt, b, inverted_spectrum=bool(b.size & 1)) == total == ref.push_packed(fmt, b, bool(b.size & 1))
        total += 2 * b.size
        blocks += b.size > 0
        g.wait()
        lo, hi = ring.range()
        assert (lo, hi) == ref.range()
        for start in (lo, hi - min(win, hi - lo)):
            n = min(win, hi - start)
            assert np.array_equal(_bits(ring.read(start, n)), _bits(ref.read(start, n)))
    assert total > cap
    assert g.rccl_info()["collectives"] == (0 if not rccl else blocks * (1 if mode == "broadcast" else 3))
    g.close()
    ref.close()


@pytest.mark.parametrize("mode", ["broadcast", "scatter_allgather"])
def test_stub_ranks_packed_push_equals_local_push(gpu, monkeypatch, mode):
    """three ranks on one device through the test stand-in for librccl (tests/host/libfake_rccl.so), as tests/test_stream_group_multi_gpu.py runs them"""
    assert os.path.exists(FAKE_RCCL), "tests/host/libfake_rccl.so was not built (__graft_entry__.build)"
    monkeypatch.setenv("GSH_RCCL_LIBRARY", FAKE_RCCL)
    from gnss_sdr_amd.sample_stream import SampleStream, StreamGroup
    assert os.path.samefile(StreamGroup.library(), FAKE_RCCL)
    fmt = _fmt(R.COMPLEX_SOURCES[0])             # Two_Bit_Packed byte iq
    cap, win = 40001, 9000
    devices = [gpu] * 3
    g = StreamGroup.local(devices, cap, win, mode=mode)
    refs = [SampleStream(cap, win, device=d) for d in devices]
    total = 0
    for b in _group_blocks(np.random.default_rng(6)):
        assert g.push_packed(fmt, b) == total
        for r in refs:
            assert r.push_packed(fmt, b) == total
        total += 2 * b.size
        g.wait()
        for i in range(3):
            ring = g.ring(i)
            lo, hi = ring.range()
            assert (lo, hi) == refs[i].range()
            for start in (lo, hi - min(win, hi - lo)):
                n = min(win, hi - start)
                assert np.array_equal(_bits(ring.read(start, n)), _bits(refs[i].read(start, n))), (i, start)
    g.close()


def _if_capture(fs, if_hz, fd, code_phase_chips, n, seed):
    """GPS L1 C/A PRN 1 at a real IF, quantised to 2 bits (2 s + 1, s = -2 .. 1) and packed as Two_Bit_Packed_File_Signal_Source defaults"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    f_code = 1.023e6 * (1.0 + fd / 1575.42e6)
    chip = np.floor(t * (f_code / fs) + code_phase_chips).astype(np.int64) % 1023
    r = 0.25 * oracle.ca_code(1).astype(np.float64)[chip] * np.cos(2.0 * np.pi * (if_hz + fd) / fs * t) + rng.standard_normal(n)
    s = np.clip(np.floor(r), -2, 1).astype(np.int64)          # the 2-bit field
    f = (s & 3).reshape(-1, 4)
    return (f[:, 0] | f[:, 1] << 2 | f[:, 2] << 4 | f[:, 3] << 6).astype(np.uint8)


def test_two_bit_if_capture_acquires_and_tracks(gpu):
    torch = pytest.importorskip("torch")
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank
    from gnss_sdr_amd.sample_stream import FirFilter, PackedFormat, SampleStream, firdes_low_pass
    from gnss_sdr_amd.tracking_loop import TrackingLoop, trk_conf
    dev = torch.device("cuda", gpu)
    fs, if_hz, D = 16e6, 4e6, 4
    fd, cph = 1830.0, 211.25
    bb = int(fs / D)                               # 4 Msps after the filter
    N, epochs = bb // 1000, 200
    n_in = (epochs + 10) * N * D
    data = _if_capture(fs, if_hz, fd, cph, n_in, seed=77)
    src = ("Two_Bit_Packed_File_Signal_Source", {})
    fmt = PackedFormat.from_signal_source(src[0], **src[1])
    x = R.source_output(src[0], data)            # the host-unpacked floats (today's path)
    taps = firdes_low_pass(1.0, fs, 1.7e6, 0.6e6)
    d_data, d_x = torch.from_numpy(data).to(dev), torch.from_numpy(x).to(dev)
    kw = dict(fs_in=bb, fft_size=N, doppler_max=5000, doppler_step=250, samples_per_chip=4, samples_per_code=float(N))
    results = []
    for packed in (True, False):
        fir = FirFilter(taps, D, if_hz, fs, fmt if packed else "float", device=gpu)
        ring = SampleStream(n_in // D + 2, 2 * N, device=gpu)
        d_y = torch.zeros(8 * N + 2, dtype=torch.complex64, device=dev)
        pos = 0
        for k, nb in enumerate([20 * N + 4, 7 * N, 33 * N - 4] * 100):     # ragged whole-byte blocks of the capture
            nb = min(nb, data.size - pos)
            if nb <= 0:
                break
            ptr = d_data.data_ptr() + pos if packed else d_x.data_ptr() + 4 * 4 * pos
            m = 4 * nb
            done = 0
            while done < m:                                                  # the filter's output buffer holds 8 ms at a time
                step = min(m - done, 7 * N * D)
                if packed:
                    step -= step % 4
                o = fir.process_device(ptr + (done // 4 if packed else 4 * done), step, d_y.data_ptr(), d_y.numel())
                ring.push_device(d_y.data_ptr(), o)
                done += step
            pos += nb
        hi = ring.range()[1]
        contents = ring.read(0, hi)
        acq = PcpsAcquisitionBank(device=gpu, max_prn=1, **kw)
        acq.set_local_code(0, oracle.ca_code_complex_sampled(1, bb))
        res = acq.dwell_ring(ring, N, 1)[0]
        acq.close()
        conf_kw = dict(fs_in=float(bb), vector_length=N, pll_bw_hz=40.0, dll_bw_hz=4.0, early_late_space_chips=0.5)
        loop = TrackingLoop(trk_conf(**conf_kw), 1, 1023, device=gpu)
        loop.set_stream_ring(ring)
        stamp = 2 * N
        loop.start(0, oracle.ca_code(1), stamp + int(round(res["acq_delay_samples"])), stamp, float(res["doppler_hz"]))
        rec, done_epochs = loop.run(epochs)
        loop.close()
        results.append((contents, res, b"".join(bytes(memoryview(r)) for r in rec[0]), rec[0], done_epochs))
        fir.close()
        ring.close()
    (c0, r0, b0, rec, done0), (c1, r1, b1, _, done1) = results
    assert c0.size == c1.size == n_in // D and np.array_equal(_bits(c0), _bits(c1))
    assert r0 == r1 and b0 == b1 and done0[0] == done1[0] == epochs
    # acquisition finds the injected PRN at its Doppler and code phase (the filter's group delay is (K - 1) / 2 input samples)
    assert abs(r0["doppler_hz"] - fd) <= 250, r0
    delay = (len(taps) - 1) / 2 / D
    code_start = ((1023.0 - cph) / (1.023e6 * (1 + fd / 1575.42e6)) * bb + delay) % N
    err = (r0["acq_delay_samples"] - code_start + N / 2) % N - N / 2
    assert abs(err) <= 2.0, (r0, code_start)
    # the loop pulls in from the acquisition's Doppler bin towards the injected Doppler (200 periods are a pull-in, not a steady state)
    tail = rec[-50:]
    assert abs(np.mean([r.carrier_doppler_hz for r in tail]) - fd) < 0.5 * abs(r0["doppler_hz"] - fd) + 1.0


def test_packed_ring_host_program(gpu):
    prog = os.path.join(ROOT, "tests", "host", "test_packed_ring")
    assert os.path.exists(prog), "tests/host/test_packed_ring was not built (__graft_entry__.build)"
    env = dict(os.environ)
    env.pop("GSH_RCCL_LIBRARY", None)
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PACKED RING OK" in r.stdout, r.stdout + r.stderr
    env["GSH_RCCL_LIBRARY"] = FAKE_RCCL
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "three stub ranks" in r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())
