"""GPU tests of the LabSat 2 / 3, LabSat 3 Wideband (LS3W) and SPIR 1-bit ingest: unpack_register_kernel (csrc/labsat_unpack.hip) behind
gsh_unpack_device, gsh_unpack_device_multi and every ring push that takes a gsh_packed_format, and packed_sample's register half behind the packed FIR
and the signal conditioner.  The checker is tests/labsat_reference.py, the numpy restatement of the layouts (held to the reference's SPIR block, the
worked examples and an independent packer by tests/test_labsat_formats.py).  Every comparison is bit for bit; blocks come from fixed seeds.
Shapes are chosen where the kernel can go wrong: registers of 3, 5, 7, 30 and 32 samples, with and without spare bits; blocks of 1, 600 and 4 099
registers (one lane; several waves and work-groups; an odd count with a grid tail); windows that start and end inside a register; destinations 8 bytes
past a 16-byte boundary; rings whose capacity boundary falls inside a register."""
import functools

import numpy as np
import pytest

import labsat_reference as L
import oracle
from helpers import tracking_params_for

pytestmark = pytest.mark.gpu

# (family, RF channels, digital I/O): spr 3 spare 10 (18-bit frames) / spr 7 spare 8 / spr 30 spare 4 / spr 32 spare 0 / spr 5 spare 4; 8, 4, 1 per item
LAYOUTS = [(L.LS3W_3BIT, 3, False), (L.LS3W_2BIT, 2, True), (L.LS3W_1BIT, 1, True), (L.LS3W_1BIT, 1, False), (L.LS3W_2BIT, 3, False),
           (L.LABSAT_2BIT, 1, False), (L.LABSAT_4BIT, 1, False), (L.SPIR_1BIT, 1, False)]
MULTI = [lay for lay in LAYOUTS if lay[1] > 1]
REGISTERS = (1, 600, 4099)


def _id(lay):
    fam, chn, dio = lay
    name = {L.LABSAT_2BIT: "labsat2", L.LABSAT_4BIT: "labsat4", L.SPIR_1BIT: "spir"}.get(fam)
    return name or f"ls3w-qua{fam - L.LS3W_1BIT + 1}-chn{chn}{'-dio' if dio else ''}"


def _spr(lay):
    return L.samples_per_item(lay[0], lay[1], lay[2])


def _fmt(lay, channel=0):
    from gnss_sdr_amd.sample_stream import PackedFormat as P
    fam, chn, dio = lay
    if fam >= L.LS3W_1BIT and fam <= L.LS3W_3BIT:
        return P(fam, P.IQ, 8, rf_channels=chn, channel=channel, flags=1 if dio else 0)
    return P(fam, P.IQ, L.item_bytes(fam))


@functools.lru_cache(maxsize=None)
def _block(lay) -> np.ndarray:
    """4 099 registers of the layout as the bytes of the file"""
    seed = 100 * lay[0] + 10 * lay[1] + int(lay[2])
    data = np.random.default_rng(seed).integers(0, 256, REGISTERS[-1] * L.item_bytes(lay[0]), dtype=np.uint8)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def _expect(lay, channel, inverted=False) -> np.ndarray:
    x = L.decode(lay[0], _block(lay), lay[1], channel, lay[2])
    x = np.conj(x).astype(np.complex64) if inverted else x
    x.setflags(write=False)
    return x


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _windows(spr):
    """(first, n) inside blocks of 1, 600 and 4 099 registers: starts at and around a register boundary, counts of one sample, one register, a count
    that ends inside a register, and the rest of the block"""
    out = []
    for regs in REGISTERS:
        total = regs * spr
        for first in sorted({0, 1, spr - 1, spr, spr + 1}):
            if first >= total:
                continue
            for n in sorted({1, spr, 2 * spr + spr // 2 + 1, total - first}):
                if first + n <= total and (first, n) not in out:
                    out.append((first, n))
    return out


GUARD = 16                       # complex samples of sentinel in front of and behind every destination
SENTINEL = np.float32(-77.25)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", gpu)


@pytest.fixture(scope="module")
def d_blocks(torch_dev):
    torch, dev = torch_dev
    return {lay: torch.from_numpy(_block(lay).copy()).to(dev) for lay in LAYOUTS}


def _single_pass(torch_dev, gpu, d_block, fmt, first, n, inverted, lead):
    """gsh_unpack_device of one channel into a guarded destination `lead` complex samples past a 16-byte boundary -> (samples, guards intact)"""
    from gnss_sdr_amd.sample_stream import unpack_device
    torch, dev = torch_dev
    out = torch.full((2 * (n + 2 * GUARD + 2),), float(SENTINEL), dtype=torch.float32, device=dev)
    o = GUARD + lead
    unpack_device(gpu, fmt, d_block.data_ptr(), first, n, out.data_ptr() + 8 * o, inverted)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    intact = bool(np.all(h[:2 * o] == SENTINEL) and np.all(h[2 * (o + n):] == SENTINEL))
    return h[2 * o:2 * (o + n)].view(np.complex64), intact


@pytest.mark.parametrize("inverted", [0, 1], ids=["plain", "inverted_spectrum"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=_id)
def test_unpack_device_single_channel(gpu, torch_dev, d_blocks, lay, inverted):
    spr = _spr(lay)
    for ch in range(lay[1]):
        fmt = _fmt(lay, ch)
        exp = _expect(lay, ch, bool(inverted))
        assert exp.size == REGISTERS[-1] * spr
        for k, (first, n) in enumerate(_windows(spr)):
            lead = (k + ch) & 1                     # every other destination 8 bytes past a 16-byte boundary
            got, intact = _single_pass(torch_dev, gpu, d_blocks[lay], fmt, first, n, bool(inverted), lead)
            assert np.array_equal(_bits(got), _bits(exp[first:first + n])), (ch, first, n, lead)
            assert intact, (ch, first, n, lead)


LISTS = {2: [[0], [1, 0], [0, 1]], 3: [[0], [2, 0], [1, 2, 0], [0, 1, 2]]}


@pytest.mark.parametrize("inverted", [0, 1], ids=["plain", "inverted_spectrum"])
@pytest.mark.parametrize("lay", MULTI, ids=_id)
def test_unpack_device_multi_equals_single_channel_passes(gpu, torch_dev, d_blocks, lay, inverted):
    from gnss_sdr_amd.sample_stream import unpack_device_multi
    torch, dev = torch_dev
    spr, chn = _spr(lay), lay[1]
    fmt = _fmt(lay, chn - 1)                          # fmt.channel is not consulted
    d_block = d_blocks[lay]
    for chans in LISTS[chn]:
        for first, n in _windows(spr):
            span = n + 2 * GUARD + 2
            out = torch.full((len(chans), 2 * span), float(SENTINEL), dtype=torch.float32, device=dev)
            offs = [GUARD + (i & 1) for i in range(len(chans))]     # 16- and 8-byte aligned destinations side by side
            ptrs = [out.data_ptr() + 8 * (i * span + offs[i]) for i in range(len(chans))]
            unpack_device_multi(gpu, fmt, d_block.data_ptr(), first, n, chans, ptrs, bool(inverted))
            torch.cuda.synchronize()
            h = out.cpu().numpy()
            for i, ch in enumerate(chans):
                o = offs[i]
                got = h[i, 2 * o:2 * (o + n)].view(np.complex64)
                assert np.array_equal(_bits(got), _bits(_expect(lay, ch, bool(inverted))[first:first + n])), (chans, ch, first, n)
                assert np.all(h[i, :2 * o] == SENTINEL) and np.all(h[i, 2 * (o + n):] == SENTINEL), (chans, ch, first, n)
        # the single-channel pass of the same window into the same kind of destination: the very same bits
        first, n = spr + 1, 100 * spr + 2
        planes = torch.zeros((len(chans), 2 * n), dtype=torch.float32, device=dev)
        unpack_device_multi(gpu, fmt, d_block.data_ptr(), first, n, chans, [planes.data_ptr() + 8 * n * i for i in range(len(chans))], bool(inverted))
        torch.cuda.synchronize()
        for i, ch in enumerate(chans):
            single, _ = _single_pass(torch_dev, gpu, d_block, fmt.with_channel(ch), first, n, bool(inverted), 0)
            assert np.array_equal(_bits(planes[i].cpu().numpy()), _bits(single)), (chans, ch)


def test_unpack_device_refusals(gpu, torch_dev, d_blocks):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import unpack_device, unpack_device_multi
    torch, dev = torch_dev
    out = torch.zeros(4 * 64, dtype=torch.float32, device=dev)
    p = out.data_ptr()
    lay = (L.LS3W_2BIT, 3, False)
    fmt, src = _fmt(lay), d_blocks[lay].data_ptr()
    labsat, spir = (L.LABSAT_2BIT, 1, False), (L.SPIR_1BIT, 1, False)
    for what, chans, ptrs, f, s, text in (
            ("a channel named twice", [0, 0], [p, p + 256], fmt, src, "named twice"),
            ("a channel >= CHN", [3], [p], fmt, src, "outside 0..2"),
            ("four destinations", [0, 1, 2, 0], [p, p + 256, p + 512, p + 768], fmt, src, "4 bands selected of a stream of 3"),
            ("a LabSat 2 / 3 format", [0], [p], _fmt(labsat), d_blocks[labsat].data_ptr(), "carries one band"),
            ("a SPIR format", [0], [p], _fmt(spir), d_blocks[spir].data_ptr(), "carries one band"),
            ("a misaligned source", [0], [p], fmt, src + 4, "8-byte aligned"),
            ("a misaligned destination", [0], [p + 4], fmt, src, "8-byte aligned")):
        with pytest.raises(GshError) as e:
            unpack_device_multi(gpu, f, s, 0, 5, chans, ptrs)
        assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    for lay2, shift, text in ((lay, 4, "8-byte aligned"), (spir, 2, "4-byte aligned"), (labsat, 1, "2-byte aligned")):
        with pytest.raises(GshError) as e:
            unpack_device(gpu, _fmt(lay2), d_blocks[lay2].data_ptr() + shift, 0, 8, p)
        assert e.value.code == 1 and text in str(e.value), (lay2, str(e.value))
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


PUSHES = [1024, 8, 0, 2048, 520, 4096, 16, 3000, 1024, 2048, 4000, 1504]   # samples per channel, cut down to whole registers of the layout
CAPS, WIN = (4102, 5004, 6150), 1024
SEEKS = (3, 1001, 37)            # capacity - seek = 4 099, 4 003, 6 113: a multiple of none of 2, 3, 5, 7, so of no spr above 1
RING_CHANNELS = {1: [0, 0, 0], 2: [1, 0, 1], 3: [2, 0, 1]}


def _pushes(spr):
    return [0 if p == 0 else max(spr, p // spr * spr) for p in PUSHES]


def _wraps_inside_a_register(spr, r):
    """(times ring r wraps, wraps that fall inside a register) over _pushes(spr): plain arithmetic on the chosen numbers"""
    cap, at, inside = CAPS[r], SEEKS[r], 0
    for n in _pushes(spr):
        if n and at // cap != (at + n - 1) // cap and (cap - at % cap) % spr != 0:
            inside += 1
        at += n
    return at // cap, inside


def _rings(gpu, n=3):
    from gnss_sdr_amd.sample_stream import SampleStream
    rings = [SampleStream(c, WIN, device=gpu) for c in CAPS[:n]]
    for r, s in zip(rings, SEEKS):
        r.seek(s)
    return rings


@pytest.mark.parametrize("inverted", [0, 1], ids=["plain", "inverted_spectrum"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=_id)
def test_ring_pushes_wrap_inside_a_register(gpu, lay, inverted):
    from gnss_sdr_amd.sample_stream import push_packed_multi
    from gnss_sdr_amd.tracking import CorrelatorBank
    spr, chn, rb = _spr(lay), lay[1], L.item_bytes(lay[0])
    pushes = _pushes(spr)
    assert all(c % 2 == 0 for c in CAPS) and max(pushes) <= min(CAPS)
    for r in range(3):                              # on the CPU first: the chosen numbers wrap every ring twice, at least once inside a register
        wraps, inside = _wraps_inside_a_register(spr, r)
        assert wraps >= 2 and (inside >= 1 or spr == 1), (r, wraps, inside)
    chans = RING_CHANNELS[chn]
    total = sum(pushes)
    data = np.random.default_rng(7 * lay[0] + chn).integers(0, 256, total // spr * rb, dtype=np.uint8)
    exp = [L.decode(lay[0], data, chn, ch, lay[2]) for ch in chans]
    if inverted:
        exp = [np.conj(x).astype(np.complex64) for x in exp]
    singles = _rings(gpu)
    multi = _rings(gpu, chn) if chn > 1 else []
    # a correlator per ring reads windows through the mirror behind the end; its twin reads the same windows of the restatement in a flat buffer
    n_win = 1000
    banks, flats = [], []
    for r in range(3):
        b, f = CorrelatorBank(1, 1023, device=gpu), CorrelatorBank(1, 1023, device=gpu)
        for k in (b, f):
            k.set_code(0, oracle.ca_code(r + 1))
        b.set_stream_ring(singles[r])
        f.set_stream_host(np.concatenate([np.zeros(SEEKS[r], np.complex64), exp[r]]))
        banks.append(b)
        flats.append(f)
    params = tracking_params_for(4e6, 1000.0, np.random.default_rng(1))
    try:
        done, mirrored = 0, 0
        for n in pushes:
            block = data[done // spr * rb:(done + n) // spr * rb]
            for r in range(3):
                assert singles[r].push_packed(_fmt(lay, chans[r]), block, bool(inverted), n_samples=n) == SEEKS[r] + done
            if multi:
                assert push_packed_multi(multi, chans[:chn], _fmt(lay), block, bool(inverted), n_samples=n) == [s + done for s in SEEKS[:chn]]
            for r in range(3):
                hi = SEEKS[r] + done + n
                lo = max(SEEKS[r], hi - CAPS[r])
                assert singles[r].range() == (lo, hi)
                if hi == lo:
                    continue
                got = singles[r].read(lo, hi - lo)   # everything resident, over the ring's end
                assert np.array_equal(_bits(got), _bits(exp[r][lo - SEEKS[r]:hi - SEEKS[r]])), (r, lo, hi)
                if r < len(multi):                    # the ring of the one-pass push: what the single-ring push of that channel leaves, index for index
                    assert multi[r].range() == (lo, hi)
                    assert np.array_equal(_bits(multi[r].read(lo, hi - lo)), _bits(got)), (r, lo, hi)
                edge = hi // CAPS[r] * CAPS[r]
                off = edge - n_win // 3
                if edge > 0 and off >= lo and off + n_win <= hi:   # a window that runs out of the ring's end into the mirror
                    job = [dict(sample_offset=off, n_samples=n_win, code_slot=0, shifts_chips=[-0.5, 0.0, 0.5], **params)]
                    assert np.array_equal(_bits(banks[r].correlate(job)), _bits(flats[r].correlate(job))), (r, off)
                    mirrored += 1
            done += n
        assert mirrored >= 3, mirrored
    finally:
        for k in banks + flats:
            k.close()
        for s in singles + multi:
            s.close()


def _page_locked(torch, nbytes):
    """page-locked host memory from the allocator that owns it for the whole process"""
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    return t, t.numpy()


@pytest.mark.parametrize("lay", [(L.LS3W_2BIT, 2, True), (L.LABSAT_2BIT, 1, False), (L.SPIR_1BIT, 1, False)], ids=_id)
def test_push_device_and_pinned_async_equal_host_push(gpu, torch_dev, lay):
    torch, dev = torch_dev
    spr, rb, ch = _spr(lay), L.item_bytes(lay[0]), lay[1] - 1
    fmt = _fmt(lay, ch)
    pushes = _pushes(spr)
    raw, data = _page_locked(torch, sum(pushes) // spr * rb)
    data[:] = np.random.default_rng(45).integers(0, 256, data.size, dtype=np.uint8)
    original = data.copy()
    d_data = torch.from_numpy(original).to(dev)
    host, devr, pinned = _rings(gpu, 1)[0], _rings(gpu, 1)[0], _rings(gpu, 1)[0]
    try:
        done = 0
        for k, n in enumerate(pushes):
            b0, nb = done // spr * rb, n // spr * rb
            a = host.push_packed(fmt, original[b0:b0 + nb], bool(k & 1), n_samples=n)
            b = devr.push_packed_device(fmt, d_data.data_ptr() + b0, n, bool(k & 1))
            c = pinned.push_packed_pinned_async(fmt, data[b0:b0 + nb], bool(k & 1), n_samples=n)
            assert a == b == c == SEEKS[0] + done
            done += n
            if n:
                assert pinned.wait_copied_upto(pinned.range()[1]) >= pinned.range()[1]
                data[b0:b0 + nb] = 0xA5               # the source is free: other bytes
        pinned.wait_copied()
        pinned.wait()
        torch.cuda.synchronize()
        lo, hi = host.range()
        assert devr.range() == pinned.range() == (lo, hi)
        h = host.read(lo, hi - lo)
        assert np.array_equal(_bits(devr.read(lo, hi - lo)), _bits(h)) and np.array_equal(_bits(pinned.read(lo, hi - lo)), _bits(h))
        m = pushes[-1]                                # the last block: pushed with inverted_spectrum (k = 11)
        exp = L.decode(lay[0], original, lay[1], ch, lay[2])
        assert np.array_equal(_bits(h[-m:]), _bits(np.conj(exp[-m:]).astype(np.complex64)))
    finally:
        for s in (host, devr, pinned):
            s.close()


def test_multi_push_device_and_pinned_async_equal_host_push(gpu, torch_dev):
    from gnss_sdr_amd.sample_stream import push_packed_multi, push_packed_multi_device, push_packed_multi_pinned_async
    torch, dev = torch_dev
    lay, chans = (L.LS3W_2BIT, 3, False), [1, 2, 0]
    spr, fmt = _spr(lay), _fmt(lay)
    pushes = _pushes(spr)
    raw, data = _page_locked(torch, sum(pushes) // spr * 8)
    data[:] = np.random.default_rng(46).integers(0, 256, data.size, dtype=np.uint8)
    original = data.copy()
    d_data = torch.from_numpy(original).to(dev)
    host, devr, pinned = _rings(gpu), _rings(gpu), _rings(gpu)
    try:
        done = 0
        for k, n in enumerate(pushes):
            b0, nb = done // spr * 8, n // spr * 8
            a = push_packed_multi(host, chans, fmt, original[b0:b0 + nb], bool(k & 1), n_samples=n)
            b = push_packed_multi_device(devr, chans, fmt, d_data.data_ptr() + b0, n, bool(k & 1))
            c = push_packed_multi_pinned_async(pinned, chans, fmt, data[b0:b0 + nb], bool(k & 1), n_samples=n)
            assert a == b == c == [s + done for s in SEEKS]
            done += n
            if n:
                ring = pinned[k % 3]                  # ANY ring of the call covers the DMA out of `data`
                assert ring.wait_copied_upto(ring.range()[1]) >= ring.range()[1]
                data[b0:b0 + nb] = 0xA5
        pinned[1].wait_copied()
        for s in pinned:
            s.wait()
        torch.cuda.synchronize()
        for r in range(3):
            lo, hi = host[r].range()
            assert devr[r].range() == pinned[r].range() == (lo, hi)
            h = host[r].read(lo, hi - lo)
            assert np.array_equal(_bits(devr[r].read(lo, hi - lo)), _bits(h)) and np.array_equal(_bits(pinned[r].read(lo, hi - lo)), _bits(h)), r
            exp = L.decode(lay[0], original, 3, chans[r], False)
            m = pushes[-1]
            assert np.array_equal(_bits(h[-m:]), _bits(np.conj(exp[-m:]).astype(np.complex64))), r
    finally:
        for s in host + devr + pinned:
            s.close()


def test_push_refusals_leave_every_ring_untouched(gpu, torch_dev):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import push_packed_multi, push_packed_multi_device, push_packed_multi_pinned_async
    torch, dev = torch_dev
    lay = (L.LS3W_2BIT, 3, False)
    spr, fmt = _spr(lay), _fmt(lay)
    data = _block(lay)[:512 * 8].copy()
    d_data = torch.from_numpy(data).to(dev)
    rings = _rings(gpu)
    assert push_packed_multi(rings, [0, 1, 2], fmt, data) == list(SEEKS)
    before = [(r.range(), r.read(r.range()[0], r.range()[1] - r.range()[0])) for r in rings]
    labsat = _fmt((L.LABSAT_4BIT, 1, False))
    too_long = (CAPS[0] // spr + 1) * spr
    refused = [
        ("a partial register", rings, [0, 1, 2], fmt, 2 * spr + 1, "whole number of 8-byte registers"),
        ("a ring twice", [rings[0], rings[1], rings[0]], [0, 1, 2], fmt, None, "named twice"),
        ("a channel twice", rings, [0, 1, 0], fmt, None, "named twice"),
        ("a channel out of range", rings, [0, 1, 3], fmt, None, "outside 0..2"),
        ("more rings than channels", rings + [rings[0]], [0, 1, 2, 0], fmt, None, "4 rings"),
        ("a single-band family", rings[:1], [0], labsat, 8, "carries one band"),
        ("larger than the smallest ring", rings, [0, 1, 2], fmt, too_long, "exceeds the ring capacity"),
    ]
    for push in (push_packed_multi, push_packed_multi_pinned_async):
        for what, rr, ch, f, n, text in refused:
            with pytest.raises(GshError) as e:
                push(rr, ch, f, data if n is None or n <= 512 * spr else np.zeros(too_long // spr * 8, np.uint8), n_samples=n)
            assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    for what, ptr, n, text in (("a misaligned block", d_data.data_ptr() + 4, 5 * spr, "8-byte aligned"), ("a partial register", d_data.data_ptr(), 7, "whole number")):
        with pytest.raises(GshError) as e:
            push_packed_multi_device(rings, [0, 1, 2], fmt, ptr, n)
        assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    for what, f, ptr, n, text in (("a misaligned block", fmt, d_data.data_ptr() + 4, 5 * spr, "8-byte aligned"), ("a partial register", fmt, d_data.data_ptr(), 7, "whole number"),
                                  ("a misaligned item", labsat, d_data.data_ptr() + 1, 8, "2-byte aligned")):
        with pytest.raises(GshError) as e:
            rings[0].push_packed_device(f, ptr, n)
        assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    for r, (rg, contents) in zip(rings, before):
        assert r.range() == rg
        assert np.array_equal(_bits(r.read(rg[0], rg[1] - rg[0])), _bits(contents))
    # and the rings still take the next block where they stood
    assert push_packed_multi(rings, [0, 1, 2], fmt, data) == [s + 512 * spr for s in SEEKS]
    for r in rings:
        r.close()


def test_group_of_one_packed_push(gpu):
    from gnss_sdr_amd.sample_stream import StreamGroup
    lay, ch = (L.LS3W_2BIT, 3, False), 1
    spr, fmt = _spr(lay), _fmt(lay, ch)
    cap, win = 4102, 1024
    g = StreamGroup.local([gpu], cap, win, mode="broadcast")
    ring = g.ring(0)
    data = _block(lay)
    exp = _expect(lay, ch)
    try:
        done = 0
        for regs in (301, 1, 0, 777, 500, 820, 641):   # 301 registers = 2 408 bytes: not a multiple of the staging buffers' 16-byte padding
            n = regs * spr
            assert g.push_packed(fmt, data[done // spr * 8:(done + n) // spr * 8], n_samples=n) == done
            done += n
            g.wait()
            lo, hi = ring.range()
            assert (lo, hi) == (max(0, done - cap), done)
            assert np.array_equal(_bits(ring.read(lo, hi - lo)), _bits(exp[lo:hi]))
        assert done > 2 * cap
    finally:
        g.close()


def test_packed_fir_equals_fir_of_the_unpacked_samples(gpu, torch_dev):
    from gnss_sdr_amd.sample_stream import FirFilter, firdes_low_pass
    torch, dev = torch_dev
    lay, ch, D, fc, fs = (L.LS3W_3BIT, 3, False), 2, 2, 1.1e6, 16.0e6
    spr, fmt = _spr(lay), _fmt(lay, 2)
    taps = firdes_low_pass(1.0, fs, 2.0e6, 1.0e6)
    x = _expect(lay, ch)
    d_data = torch.from_numpy(_block(lay).copy()).to(dev)
    d_x = torch.from_numpy(x.copy()).to(dev)
    outs = []
    for packed in (True, False):
        f = FirFilter(taps, D, fc, fs, fmt if packed else "gr_complex", device=gpu)
        cap = x.size // D + 2
        d_y = torch.zeros(cap, dtype=torch.complex64, device=dev)
        pos, out = 0, 0
        for regs in (1, 2, 5, 1000, 3, 3088):            # uneven blocks (registers), the first ones shorter than the filter
            src = d_data.data_ptr() + 8 * pos if packed else d_x.data_ptr() + 8 * pos * spr
            out += f.process_device(src, regs * spr, d_y.data_ptr() + 8 * out, cap - out)
            pos += regs
        assert pos == REGISTERS[-1]
        torch.cuda.synchronize()
        outs.append(d_y.cpu().numpy()[:out])
        f.close()
    assert outs[0].size == (x.size + D - 1) // D and np.any(outs[0] != 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("filtered", [False, True], ids=["adapter_only", "filter"])
def test_conditioner_takes_the_register_families(gpu, torch_dev, filtered):
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import FirFilter, SampleStream, firdes_low_pass
    torch, dev = torch_dev
    lay, ch, D, fs = (L.LS3W_2BIT, 2, True), 1, 2, 16.0e6
    spr, fmt = _spr(lay), _fmt(lay, 1)
    x = np.conj(_expect(lay, ch)).astype(np.complex64)    # pushed with inverted_spectrum
    if filtered:
        taps = firdes_low_pass(1.0, fs, 2.0e6, 1.0e6)
        d_x = torch.from_numpy(x).to(dev)
        d_y = torch.zeros(x.size // D + 2, dtype=torch.complex64, device=dev)
        f = FirFilter(taps, D, 0.9e6, fs, "gr_complex", device=gpu)
        n_f = f.process_device(d_x.data_ptr(), x.size, d_y.data_ptr(), d_y.numel())
        torch.cuda.synchronize()
        f.close()
        exp = d_y.cpu().numpy()[:n_f].copy()
        kw = dict(taps=taps, decimation=D, center_freq_hz=0.9e6, sampling_freq_hz=fs)
    else:
        exp, kw = x, {}
    ring = SampleStream(5004, WIN, device=gpu)
    cond = SignalConditioner(ring, input_kind=fmt, inverted_spectrum=True, device=gpu, **kw)
    data = _block(lay)
    d_data = torch.from_numpy(data.copy()).to(dev)
    try:
        pos, made = 0, 0
        for k, regs in enumerate((1, 2, 300, 5, 311, 700, 700, 700, 700, 680)):   # each block below the ring's capacity
            if k & 1:
                first, n_out = cond.push_device(d_data.data_ptr() + 8 * pos, regs * spr)
            else:
                first, n_out = cond.push(data[8 * pos:8 * (pos + regs)], regs * spr)
            pos += regs
            assert first == made
            made += n_out
            lo, hi = ring.range()
            assert hi == made
            assert np.array_equal(_bits(ring.read(lo, hi - lo)), _bits(exp[lo:hi])), (k, lo, hi)
        assert pos == REGISTERS[-1] and made == exp.size and made > 2 * 5004
    finally:
        cond.close()
        ring.close()
