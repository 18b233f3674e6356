"""GPU tests of the ION_GSMS ingest: unpack_ion_kernel (csrc/ion_unpack.hip) behind gsh_ion_unpack_device and the three ring pushes gsh_stream_push_ion,
_device and _pinned_async.  The checker of the kernel is gsh_ion_decode_host, the host build of the same decoder, which tests/test_ion_gsms_formats.py
holds to the numpy restatement; the checker of the pushes is gsh_stream_push of the host-decoded samples and, for the layout that expresses GSS6450
4-bit with three bands, gsh_stream_push_packed_multi.  Every comparison is bit for bit; blocks come from fixed seeds.
Shapes: 1 500 cycles of 3 samples (4 500 samples: two work-groups of a complex stream, the last one partial), windows that start inside a cycle and
hold 1 sample, 2 rate - 1 samples, and a count that leaves a partial last work-group; 1, 3 and 8 selected streams with unselected ones between them;
destinations 16-byte aligned and 8 (4 for real streams) bytes past such a boundary, with guard words around each."""
import functools

import numpy as np
import pytest

import ion_gsms_reference as R

pytestmark = pytest.mark.gpu

GUARD = 16                       # floats of sentinel in front of and behind every destination
SENTINEL = np.float32(-77.25)
CYCLES, RATE = 1500, 3
WIDTHS = (1, 2, 3, 5, 8, 12, 16)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _layout(chunks):
    from gnss_sdr_amd.ion_gsms import IonLayout
    return IonLayout(chunks, R.flat(chunks))


def _chunk(size_word, big, w, kind, n_sel=9, rate=RATE, head=1):
    """n_sel streams of field width w and equal rate, encodings and alignments cycling, an unselected 5-bit stream behind each: stream 2 i is
    selectable, stream 2 i + 1 lies between"""
    per = 1 if kind == R.REAL else 2
    streams = []
    for i in range(n_sel):
        enc = (i + w) % 11
        alignment = (i + w) % 3
        if enc == R.SIGN and w > 1 and alignment == 0:
            alignment = 1
        q = 1 if enc == R.SIGN else w if alignment == 0 else max(1, w - i % 3)
        streams.append(R.stream(w * per * rate, rate, q, enc, kind, alignment, 0, (i + w) % (4 if per == 2 else 2)))
        streams.append(R.stream(5, 1, 3, R.OB, R.REAL, 2))
    used = sum(s["packed_bits"] for s in streams)
    word = 8 * size_word
    return R.chunk(size_word, (used + 3 + word - 1) // word, streams, big, head)


@functools.lru_cache(maxsize=None)
def _block(nbytes, seed) -> np.ndarray:
    data = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
    data.setflags(write=False)
    return data


@pytest.fixture(scope="module")
def torch_dev(gpu):
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", gpu)


def _unpack(torch_dev, gpu, lay, d_block, first, n, sel, cplx, inverted=False, leads=None, src_shift=0):
    """gsh_ion_unpack_device of the selected streams into guarded destinations, destination i `leads[i]` floats past a 16-byte boundary
    -> (samples per stream, guards intact)"""
    torch, dev = torch_dev
    per = 2 if cplx else 1
    leads = leads or [0] * len(sel)
    span = (n * per + 2 * GUARD + 8 + 3) // 4 * 4
    out = torch.full((len(sel), span), float(SENTINEL), dtype=torch.float32, device=dev)
    assert out.data_ptr() % 16 == 0
    offs = [GUARD + l for l in leads]
    lay.unpack_device(gpu, d_block.data_ptr() + src_shift, first, n, sel, [out.data_ptr() + 4 * (i * span + offs[i]) for i in range(len(sel))], inverted)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    got, intact = [], True
    for i in range(len(sel)):
        o = offs[i]
        intact = intact and bool(np.all(h[i, :o] == SENTINEL) and np.all(h[i, o + n * per:] == SENTINEL))
        got.append(h[i, o:o + n * per].copy())
    return got, intact


def _expect(lay, data, stream, first, n, inverted=False):
    x = lay.decode_host(stream, data, first, n)
    if inverted:
        x = np.conj(x)
    return np.ascontiguousarray(x).view(np.float32)


def _windows(rate, total):
    return [(0, total), (1, 1), (rate + 1, 2 * rate - 1), (rate - 1, total - 7), (total - 1, 1)]


@pytest.mark.parametrize("kind", [R.REAL, R.IQ, R.QI], ids=["real", "iq", "qi"])
@pytest.mark.parametrize("big", [0, 1], ids=["little", "big"])
@pytest.mark.parametrize("size_word", [1, 2, 4, 8])
def test_unpack_device_equals_the_host_decoder(gpu, torch_dev, size_word, big, kind):
    torch, dev = torch_dev
    cplx = kind != R.REAL
    for w in WIDTHS:
        chunks = [_chunk(size_word, big, w, kind)]
        if size_word == 8 and w >= 12:  # a field across a 64-bit word boundary (the selected streams lie 5 bits apart)
            pos, crossed = 8 * R.cycle_bytes(chunks) - sum(s["packed_bits"] for s in R.flat(chunks)), False
            for s in R.flat(chunks):
                crossed |= any((pos + j * R.field_bits(s)) // 64 != (pos + (j + 1) * R.field_bits(s) - 1) // 64 for j in range(R.fields_per_cycle(s)))
                pos += s["packed_bits"]
            assert crossed
        lay = _layout(chunks)
        data = _block(CYCLES * lay.cycle_bytes, 100 * size_word + 10 * big + w)
        d_block = torch.from_numpy(data.copy()).to(dev)
        total = CYCLES * RATE
        try:
            for k, (first, n) in enumerate(_windows(RATE, total)):
                for sel in ([8], [0, 8, 4], [0, 2, 4, 6, 8, 10, 12, 14]):
                    if len(sel) == 8 and k not in (0, 3):
                        continue
                    inverted = cplx and (k + len(sel)) % 2 == 1
                    leads = [2 * ((i + k) & 1) if cplx else (i + k) % 4 for i in range(len(sel))]
                    got, intact = _unpack(torch_dev, gpu, lay, d_block, first, n, sel, cplx, inverted, leads)
                    for g, s in zip(got, sel):
                        assert np.array_equal(_bits(g), _bits(_expect(lay, data, s, first, n, inverted))), (w, first, n, sel, s)
                    assert intact, (w, first, n, sel)
        finally:
            lay.close()


@pytest.mark.parametrize("nbytes", [3, 20, 4096])
def test_unpack_device_cycle_sizes(gpu, torch_dev, nbytes):
    """cycles of 3 bytes (12-bit complex TC across 8-bit words), 20 bytes (head padding in 32-bit words) and 4096 bytes (the largest: a work-group
    stages 4 cycles at the most), the block based at an address that is aligned to the word and to nothing more"""
    torch, dev = torch_dev
    if nbytes == 3:
        chunks, cycles, sels = [R.chunk(1, 3, [R.stream(24, 1, 12, R.TC, R.IQ)])], 3001, [[0]]
    elif nbytes == 20:
        chunks = [R.chunk(4, 5, [R.stream(70, 7, 5, R.OBA, R.IQ), R.stream(9, 1, 3, R.SM, R.REAL, 1), R.stream(75, 15, 5, R.MS, R.REAL)], padding=1)]
        cycles, sels = 601, [[0], [2], [1]]
    else:
        chunks = [R.chunk(8, 512, [R.stream(16384, 1024, 16, R.OG, R.REAL), R.stream(5, 1, 5, R.OB), R.stream(16368, 1023, 8, R.SMA, R.QI, 2, 0, 3),
                                   R.stream(11, 1, 11, R.TC)])]
        cycles, sels = 5, [[0], [2], [1, 3]]
    lay = _layout(chunks)
    assert lay.cycle_bytes == nbytes
    align = max(c["size_word"] for c in chunks)
    data = _block(cycles * nbytes, nbytes)
    shifted = np.zeros(data.size + 16, np.uint8)
    shifted[align:align + data.size] = data
    d_block = torch.from_numpy(shifted).to(dev)
    try:
        for sel in sels:
            rate, cplx, _ = lay.stream_info(sel[0])
            total = cycles * rate
            for k, (first, n) in enumerate(_windows(rate, total)):
                if n < 1 or first + n > total:
                    continue
                got, intact = _unpack(torch_dev, gpu, lay, d_block, first, n, sel, cplx, cplx and k & 1, [(k + i) % 4 & (2 if cplx else 3) for i in range(len(sel))], align)
                for g, s in zip(got, sel):
                    assert np.array_equal(_bits(g), _bits(_expect(lay, data, s, first, n, cplx and k & 1))), (sel, s, first, n)
                assert intact, (sel, first, n)
    finally:
        lay.close()


# ---- the layout that expresses GSS6450 4-bit, endian 0, three bands: one chunk of three 32-bit little-endian words, a stream per word, 4 samples of
# 4-bit TC each, Q in front of I
def _gss_chunks():
    return [R.chunk(4, 3, [R.stream(32, 4, 4, R.TC, R.QI, name=f"band{b}") for b in range(3)])]


def _gss_format(channel=0):
    from gnss_sdr_amd.sample_stream import PackedFormat as P
    return P(P.GSS6450_4BIT, P.IQ, 4, rf_channels=3, channel=channel)


CAPS, WIN, SEEKS = (4102, 5006, 6150), 1024, (3, 1001, 37)     # capacity - seek is odd everywhere: the rings wrap inside a cycle of 4 samples
PUSHES = [1024, 8, 0, 2048, 520, 4096, 16, 3000, 1024, 2048, 4000, 1504]


def _rings(gpu, n=3):
    from gnss_sdr_amd.sample_stream import SampleStream
    rings = [SampleStream(c, WIN, device=gpu) for c in CAPS[:n]]
    for r, s in zip(rings, SEEKS):
        r.seek(s)
    return rings


def _page_locked(torch, nbytes):
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    return t, t.numpy()


def test_gss6450_layout_reading_is_confirmed_by_the_host_decoders(gsh):
    from gnss_sdr_amd.sample_stream import packed_decode_host
    lay = _layout(_gss_chunks())
    data = _block(12 * 300, 6450)
    try:
        for b in range(3):
            assert np.array_equal(_bits(lay.decode_host(b, data)), _bits(packed_decode_host(_gss_format(b), data, 0, 1200))), b
    finally:
        lay.close()


def test_pushes_equal_the_gss6450_multi_push_and_the_push_of_decoded_samples(gpu, torch_dev):
    """all three forms of gsh_stream_push_ion into three rings of different capacity and next index, pushes of unequal size that wrap every ring inside
    a cycle: after each push every ring holds what gsh_stream_push_packed_multi of the same bytes as GSS6450 left, and what gsh_stream_push of the
    host-decoded samples left -- resident range, contents, first index"""
    from gnss_sdr_amd.sample_stream import push_packed_multi
    torch, dev = torch_dev
    lay = _layout(_gss_chunks())
    bands = [2, 0, 1]
    assert all((c - s) % 4 != 0 for c, s in zip(CAPS, SEEKS)) and all(p % 4 == 0 for p in PUSHES) and max(PUSHES) <= min(CAPS)
    total = sum(PUSHES)
    raw, data = _page_locked(torch, total * 3)
    data[:] = np.random.default_rng(64).integers(0, 256, data.size, dtype=np.uint8)
    original = data.copy()
    d_data = torch.from_numpy(original).to(dev)
    decoded = [lay.decode_host(b, original) for b in bands]
    sets = {name: _rings(gpu) for name in ("gss", "decoded", "host", "device", "pinned")}
    try:
        done = 0
        for k, n in enumerate(PUSHES):
            inv = bool(k & 1)
            b0, nb = done * 3, n * 3
            want = [s + done for s in SEEKS]
            assert push_packed_multi(sets["gss"], bands, _gss_format(), original[b0:b0 + nb], inv, n_samples=n) == want
            for r in range(3):
                if n:
                    assert sets["decoded"][r].push(decoded[r][done:done + n], "gr_complex", inv) == want[r]
            assert lay.push(sets["host"], bands, original[b0:b0 + nb], inv, n_samples=n) == want
            assert lay.push_device(sets["device"], [f"band{b}" for b in bands], d_data.data_ptr() + b0, n, inv) == want
            assert lay.push_pinned_async(sets["pinned"], bands, data[b0:b0 + nb], inv, n_samples=n) == want
            done += n
            if n:
                ring = sets["pinned"][k % 3]          # ANY ring of the call covers the DMA out of `data`
                assert ring.wait_copied_upto(ring.range()[1]) >= ring.range()[1]
                data[b0:b0 + nb] = 0xA5               # the source is free: other bytes
            for r in range(3):
                hi = SEEKS[r] + done
                lo = max(SEEKS[r], hi - CAPS[r])
                for name, rings in sets.items():
                    assert rings[r].range() == (lo, hi), (name, r, k)
                if hi == lo:
                    continue
                for s in sets["pinned"]:
                    s.wait()
                ref = sets["gss"][r].read(lo, hi - lo)    # everything resident, over the ring's end
                for name in ("decoded", "host", "device", "pinned"):
                    assert np.array_equal(_bits(sets[name][r].read(lo, hi - lo)), _bits(ref)), (name, r, k, lo, hi)
        sets["pinned"][1].wait_copied()
        wraps = [(s + total) // c for s, c in zip(SEEKS, CAPS)]
        assert min(wraps) >= 2
    finally:
        for rings in sets.values():
            for s in rings:
                s.close()
        lay.close()


def test_refused_pushes_leave_every_ring_untouched(gpu, torch_dev):
    from gnss_sdr_amd import GshError
    torch, dev = torch_dev
    chunks = [R.chunk(4, 4, [R.stream(32, 4, 4, R.TC, R.QI), R.stream(32, 4, 4, R.TC, R.IQ), R.stream(32, 2, 8, R.OB, R.IQ), R.stream(32, 4, 8, R.OB)])]
    lay = _layout(chunks)
    data = _block(16 * 256, 9)
    d_data = torch.from_numpy(data.copy()).to(dev)
    raw, pinned = _page_locked(torch, data.size)
    pinned[:] = data
    rings = _rings(gpu)
    try:
        assert lay.push(rings[:2], [0, 1], data) == list(SEEKS[:2])
        before = [(r.range(), r.read(r.range()[0], r.range()[1] - r.range()[0]) if r.range()[1] > r.range()[0] else None) for r in rings]
        big = np.zeros((CAPS[0] // 4 + 1) * 16, np.uint8)
        refused = [
            ("a partial cycle", rings[:2], [0, 1], data, 1022, "whole number of cycles"),
            ("streams of unequal rate", rings[:2], [0, 2], data, None, "2 samples per cycle"),
            ("a real stream", rings[:1], [3], data, None, "real IF samples"),
            ("complex and real", rings[:2], [0, 3], data, None, "complex and real"),
            ("a ring twice", [rings[0], rings[0]], [0, 1], data, None, "named twice"),
            ("a stream twice", rings[:2], [1, 1], data, None, "named twice"),
            ("a stream out of range", rings[:2], [0, 4], data, None, "outside 0..3"),
            ("larger than the smallest ring", rings[:2], [0, 1], big, None, "exceeds the ring capacity"),
        ]
        for what, rr, sel, d, n, text in refused:
            for push in (lay.push, lay.push_pinned_async):
                with pytest.raises(GshError) as e:
                    push(rr, sel, pinned if (d is data and push == lay.push_pinned_async) else d, False, n)
                assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
            with pytest.raises(GshError) as e:
                lay.push_device(rr, sel, d_data.data_ptr(), n if n is not None else d.size // 16 * 4, False)
            assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
        with pytest.raises(GshError) as e:
            lay.push_device(rings[:2], [0, 1], d_data.data_ptr() + 2, 64)
        assert e.value.code == 1 and "4-byte aligned" in str(e.value)
        for r, (rg, contents) in zip(rings, before):
            assert r.range() == rg
            if contents is not None:
                assert np.array_equal(_bits(r.read(rg[0], rg[1] - rg[0])), _bits(contents))
        # and the rings still take the next block where they stood
        assert lay.push(rings[:2], [0, 1], data) == [s + 1024 for s in SEEKS[:2]]
    finally:
        for r in rings:
            r.close()
        lay.close()


def test_a_live_tracking_channel_in_the_way_refuses_the_push(gpu):
    """three antennas of 8-bit I/Q as one ION cycle of 6 bytes; a live tracking channel follows the first ring: a push that would overwrite its next
    window is refused with GSH_ERR_STATE by all three forms and no ring advances"""
    import oracle
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    from test_tracking_live_gpu import KW, N, _drain, _loop, _scenario
    torch = pytest.importorskip("torch")
    prns, dops, starts, total, x8, xf = _scenario(20, seed=9)
    noise = np.random.default_rng(3).integers(-3, 4, (2, total, 2)).astype(np.int8)
    block = np.ascontiguousarray(np.stack([x8, noise[0], noise[1]], axis=1)).view(np.uint8).reshape(-1)      # [sample][antenna][I, Q]
    lay = _layout([R.chunk(1, 6, [R.stream(16, 1, 8, R.TC, R.IQ) for _ in range(3)])])
    rings = [SampleStream(c, 2 * N, device=gpu) for c in (12 * N, 13 * N + 1, 14 * N)]
    live = _loop(gpu, dict(KW, enable_lock_detectors=0), n_channels=1)
    try:
        live.set_stream_ring(rings[0])
        live.start(0, oracle.ca_code(prns[0]), starts[0], 0, dops[0] + 6.0)
        live.live_configure(idle_timeout_us=100000, residency_us=1000000)
        assert lay.push(rings, [0, 1, 2], block[:6 * 8 * N]) == [0, 0, 0]
        assert np.array_equal(rings[0].read(0, 8 * N), x8[:8 * N, 0].astype(np.float32) + 1j * x8[:8 * N, 1].astype(np.float32))
        before = [r.range() for r in rings]
        held = [r.read(lo, hi - lo) for r, (lo, hi) in zip(rings, before)]
        live.live_begin()
        got, lost = [[]], [False]
        _drain(live, got, lost, 2.0, want=[6])
        assert len(got[0]) >= 6
        # the channel stands below 8 N; the first ring holds 12 N: a push of 12 N more would overwrite its next window
        zeros = np.zeros(6 * 12 * N, np.uint8)
        t = torch.zeros(zeros.size, dtype=torch.uint8, pin_memory=True)
        d = torch.zeros(zeros.size, dtype=torch.uint8, device=torch.device("cuda", gpu))
        for what, call in (("host", lambda: lay.push(rings, [0, 1, 2], zeros)), ("pinned", lambda: lay.push_pinned_async(rings, [0, 1, 2], t.numpy())),
                           ("device", lambda: lay.push_device(rings, [0, 1, 2], d.data_ptr(), 12 * N))):
            with pytest.raises(GshError) as e:
                call()
            assert e.value.code == 4, (what, str(e.value))
            assert [r.range() for r in rings] == before, what
        live.live_quiesce()
        for r, b, h in zip(rings, before, held):
            assert np.array_equal(_bits(r.read(b[0], b[1] - b[0])), _bits(h))
        assert lay.push(rings, [0, 1, 2], block[6 * 8 * N:6 * 9 * N]) == [8 * N] * 3
    finally:
        live.close()
        for r in rings:
            r.close()
        lay.close()
