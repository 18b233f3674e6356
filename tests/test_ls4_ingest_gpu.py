"""GPU tests of the LabSat 4 ingest: unpack_ls4_kernel (csrc/labsat_unpack.hip) behind gsh_unpack_device, gsh_unpack_device_multi and every ring push
that takes a gsh_packed_format, and packed_sample's LabSat 4 branch behind the packed FIR and the signal conditioner.  The checker is
tests/ls4_reference.py, the numpy restatement of the layout (held to the worked examples and an independent packer by tests/test_ls4_formats.py).
Every comparison is bit for bit; blocks come from fixed seeds.
Shapes: every QUA x the layouts (6,0,0), (6,6,6), (0,6,0) and the unequal (12,6,3) x every recorded slot, 5 rounds, with windows that start at 1,
inside a register, at samples 2 and 5 of a QUA 12 triple and one before / after a round boundary, and counts that end inside a register; destinations
8 bytes past a 16-byte boundary; rings whose capacity boundary falls inside a register or triple.  One further test takes the launcher's other paths:
S = 1 024 samples a round, the largest that lanes divide by, with 4 200 rounds (two launches: a launch ends where t S reaches 2^32); S = 1 056 and
1 032, the first above it at QUA 1 and QUA 12 (a grid row per round, with a head and a tail launch inside a round); S = 32 768 and 32 800 (many
work-groups a row); and 4 099 rounds of one triple (many work-groups, a grid tail)."""
import functools

import numpy as np
import pytest

import ls4_reference as L

pytestmark = pytest.mark.gpu

CASES = [(q, regs) for q in L.QUAS for regs in L.LAYOUTS]
LONG = 600                       # rounds of the blocks behind the ring pushes, the FIR and the conditioner
GUARD = 16                       # complex samples of sentinel in front of and behind every destination
SENTINEL = np.float32(-77.25)


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _slots(regs):
    return [s for s in range(3) if regs[s]]


def _fmt(qua, regs, channel=None):
    from gnss_sdr_amd.sample_stream import PackedFormat as P
    return P.ls4(qua, regs, _slots(regs)[0] if channel is None else channel)


@functools.lru_cache(maxsize=None)
def _block(qua, regs, rounds=L.ROUNDS) -> np.ndarray:
    seed = 1000 * qua + sum(r << (5 * i) for i, r in enumerate(regs)) + rounds
    data = np.random.default_rng(seed).integers(0, 256, rounds * L.round_bytes(regs), dtype=np.uint8)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def _expect(qua, regs, slot, rounds=L.ROUNDS, inverted=False) -> np.ndarray:
    x = L.decode(_block(qua, regs, rounds), qua, regs, slot)
    x = np.conj(x).astype(np.complex64) if inverted else x
    x.setflags(write=False)
    return x


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _windows(qua, S, total):
    """as the host test's: first at 1, inside a register, at samples 2 and 5 of a triple, around a round boundary; counts that end mid-register"""
    spr = L.samples_per_register(qua)
    out = []
    for first in sorted({0, 1, 2, 5, spr - 1, spr + 1, S - 1, S + 1, 2 * S + 5}):
        for n in sorted({1, 2, spr + 1, S, S + spr // 2 + 1, total - first}):
            if 0 < n and first + n <= total:
                out.append((first, n))
    return out


@pytest.fixture(scope="module")
def torch_dev(gpu):
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", gpu)


def _single_pass(torch_dev, gpu, d_block, fmt, first, n, inverted, lead):
    """gsh_unpack_device of one slot into a guarded destination `lead` complex samples past a 16-byte boundary -> (samples, guards intact)"""
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
@pytest.mark.parametrize("qua,regs", CASES, ids=_id)
def test_unpack_device_single_channel(gpu, torch_dev, qua, regs, inverted):
    torch, dev = torch_dev
    d_block = torch.from_numpy(_block(qua, regs).copy()).to(dev)
    for slot in _slots(regs):
        fmt = _fmt(qua, regs, slot)
        exp = _expect(qua, regs, slot, inverted=bool(inverted))
        S = L.samples_per_round(qua, regs, slot)
        assert exp.size == L.ROUNDS * S
        for k, (first, n) in enumerate(_windows(qua, S, exp.size)):
            lead = (k + slot) & 1                   # every other destination 8 bytes past a 16-byte boundary
            got, intact = _single_pass(torch_dev, gpu, d_block, fmt, first, n, bool(inverted), lead)
            assert np.array_equal(_bits(got), _bits(exp[first:first + n])), (slot, first, n, lead)
            assert intact, (slot, first, n, lead)


@pytest.mark.parametrize("inverted", [0, 1], ids=["plain", "inverted_spectrum"])
@pytest.mark.parametrize("qua", L.QUAS)
def test_unpack_device_multi_equals_single_channel_passes(gpu, torch_dev, qua, inverted):
    from gnss_sdr_amd.sample_stream import unpack_device_multi
    torch, dev = torch_dev
    regs = (6, 6, 6)
    S = L.samples_per_round(qua, regs, 0)
    d_block = torch.from_numpy(_block(qua, regs).copy()).to(dev)
    for chans in ([0, 1, 2], [2, 1, 0], [1], [2, 0]):
        fmt = _fmt(qua, regs, 2 - chans[0])         # fmt.channel is not consulted
        for first, n in _windows(qua, S, L.ROUNDS * S):
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
                single, _ = _single_pass(torch_dev, gpu, d_block, fmt.with_channel(ch), first, n, bool(inverted), offs[i] - GUARD)
                assert np.array_equal(_bits(got), _bits(single)), (chans, ch, first, n)
                assert np.array_equal(_bits(got), _bits(_expect(qua, regs, ch, inverted=bool(inverted))[first:first + n])), (chans, ch, first, n)
                assert np.all(h[i, :2 * o] == SENTINEL) and np.all(h[i, 2 * (o + n):] == SENTINEL), (chans, ch, first, n)
    # the equal slots of an unequal layout cannot be paired, but two equal ones beside a third can
    regs = (6, 3, 6)
    d_block = torch.from_numpy(_block(qua, regs).copy()).to(dev)
    n = L.ROUNDS * S
    out = torch.zeros((2, 2 * n), dtype=torch.float32, device=dev)
    unpack_device_multi(gpu, _fmt(qua, regs, 1), d_block.data_ptr(), 0, n, [2, 0], [out.data_ptr(), out.data_ptr() + 8 * n], bool(inverted))
    torch.cuda.synchronize()
    for i, ch in enumerate((2, 0)):
        assert np.array_equal(_bits(out[i].cpu().numpy()), _bits(_expect(qua, regs, ch, inverted=bool(inverted)))), ch


# (QUA, regs, rounds): S = 1 024 with more rounds than one dividing launch takes; the first S above 1 024 that the layout allows; large S; many small rounds
PATHS = [(1, (32, 0, 0), 4200), (1, (0, 33, 3), 7), (12, (3, 387, 0), 7), (12, (384, 0, 0), 5), (1, (1024, 0, 0), 5), (2, (0, 2050, 6), 3),
         (12, (3, 0, 0), 4099), (8, (1, 2, 0), 4099)]


@pytest.mark.parametrize("qua,regs,rounds", PATHS, ids=_id)
def test_unpack_device_launch_paths(gpu, torch_dev, qua, regs, rounds):
    from gnss_sdr_amd.sample_stream import unpack_device
    torch, dev = torch_dev
    slot = int(np.argmax(regs))
    S = L.samples_per_round(qua, regs, slot)
    assert S in (1024, 1056, 1032, 32768, 32800, 8)
    d_block = torch.from_numpy(_block(qua, regs, rounds).copy()).to(dev)
    exp = _expect(qua, regs, slot, rounds)
    fmt = _fmt(qua, regs, slot)
    for first, n in ((0, exp.size), (S - 3, exp.size - S), (5, 2 * S + 1)):
        out = torch.full((2 * (n + 2 * GUARD),), float(SENTINEL), dtype=torch.float32, device=dev)
        unpack_device(gpu, fmt, d_block.data_ptr(), first, n, out.data_ptr() + 8 * GUARD)
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert np.array_equal(_bits(h[2 * GUARD:2 * (GUARD + n)]), _bits(exp[first:first + n])), (first, n)
        assert np.all(h[:2 * GUARD] == SENTINEL) and np.all(h[2 * (GUARD + n):] == SENTINEL), (first, n)


def test_unpack_device_refusals(gpu, torch_dev):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import PackedFormat as P, unpack_device, unpack_device_multi
    torch, dev = torch_dev
    out = torch.zeros(4 * 64, dtype=torch.float32, device=dev)
    p = out.data_ptr()
    d = torch.from_numpy(_block(2, (12, 6, 3)).copy()).to(dev)
    src = d.data_ptr()
    equal, unequal = _fmt(2, (6, 6, 6)), _fmt(2, (12, 6, 3))
    ls3w = P(P.LS3W_2BIT, P.IQ, 8, rf_channels=3)
    for what, chans, ptrs, f, s, texts in (
            ("unequal register counts", [0, 2], [p, p + 256], unequal, src, ("channels 0 and 2 hold 12 and 3 registers",)),
            ("unequal register counts", [1, 0], [p, p + 256], unequal, src, ("channels 1 and 0 hold 6 and 12 registers",)),
            ("a slot named twice", [0, 0], [p, p + 256], equal, src, ("named twice",)),
            ("a slot >= rf_channels", [3], [p], equal, src, ("outside 0..2",)),
            ("a slot that is not recorded", [1, 0], [p, p + 256], _fmt(2, (6, 0, 6)), src, ("channel 1 (slot B) is not recorded",)),
            ("four destinations", [0, 1, 2, 0], [p, p + 256, p + 512, p + 768], equal, src, ("4 bands selected of a stream of 3",)),
            ("QUA 12 without whole triples", [0], [p], P.ls4(12, (4,)), src, ("QUA 12 with 4 registers",)),
            ("a misaligned source", [0], [p], equal, src + 4, ("8-byte aligned",)),
            ("a misaligned destination", [0], [p + 4], equal, src, ("8-byte aligned",)),
            ("the LS3W text stands", [0, 0], [p, p + 256], ls3w, src, ("named twice",))):
        with pytest.raises(GshError) as e:
            unpack_device_multi(gpu, f, s, 0, 16, chans, ptrs)
        assert e.value.code == 1 and all(t in str(e.value) for t in texts), (what, str(e.value))
    for f, shift, text in ((equal, 4, "8-byte aligned"), (_fmt(2, (0, 6, 0), 0), 0, "slot A) is not recorded"), (P.ls4(2, (-1,)), 0, "register count -1")):
        with pytest.raises(GshError) as e:
            unpack_device(gpu, f, src + shift, 0, 16, p)
        assert e.value.code == 1 and text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()


PUSHES = [1024, 8, 0, 2048, 520, 4096, 16, 3000, 1024, 2048, 4000, 1504]   # samples per slot, cut down to whole rounds of the layout
CAPS, WIN = (4102, 5006, 6150), 1024
SEEKS = (3, 1001, 37)            # capacity - seek = 4 099, 4 005, 6 113: odd, and every push is a whole number of registers (4 .. 32 samples)
RING_CHANNELS = [2, 0, 1]
EQUAL = (6, 6, 6)


def _pushes(S):
    return [0 if p == 0 else max(S, p // S * S) for p in PUSHES]


def _wraps_inside_a_register(qua, S, r):
    """(times ring r wraps, wraps that fall inside a register, or inside a triple at QUA 12) over _pushes(S): arithmetic on the chosen numbers"""
    spr, cap, at, inside = L.samples_per_register(qua), CAPS[r], SEEKS[r], 0
    for n in _pushes(S):
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
@pytest.mark.parametrize("qua", L.QUAS)
def test_ring_pushes_wrap_inside_a_register(gpu, qua, inverted):
    """three single-ring pushes and one multi push into three rings of different capacity, several pushes of unequal size: after each the resident
    range of every ring equals the restatement, and the rings of the multi push equal those of the single pushes"""
    from gnss_sdr_amd.sample_stream import push_packed_multi
    S, rb = L.samples_per_round(qua, EQUAL, 0), L.round_bytes(EQUAL)
    pushes = _pushes(S)
    assert all(c % L.samples_per_register(qua) != 0 for c in CAPS) and max(pushes) <= min(CAPS)
    for r in range(3):                              # on the CPU first: the chosen numbers wrap every ring twice, each time inside a register / triple
        wraps, inside = _wraps_inside_a_register(qua, S, r)
        assert wraps >= 2 and inside >= 2, (r, wraps, inside)
    total = sum(pushes)
    data = np.random.default_rng(7 * qua).integers(0, 256, total // S * rb, dtype=np.uint8)
    exp = [L.decode(data, qua, EQUAL, ch) for ch in RING_CHANNELS]
    if inverted:
        exp = [np.conj(x).astype(np.complex64) for x in exp]
    singles, multi = _rings(gpu), _rings(gpu)
    try:
        done = 0
        for n in pushes:
            block = data[done // S * rb:(done + n) // S * rb]
            for r in range(3):
                assert singles[r].push_packed(_fmt(qua, EQUAL, RING_CHANNELS[r]), block, bool(inverted), n_samples=n) == SEEKS[r] + done
            assert push_packed_multi(multi, RING_CHANNELS, _fmt(qua, EQUAL, 1), block, bool(inverted), n_samples=n) == [s + done for s in SEEKS]
            for r in range(3):
                hi = SEEKS[r] + done + n
                lo = max(SEEKS[r], hi - CAPS[r])
                assert singles[r].range() == multi[r].range() == (lo, hi)
                if hi == lo:
                    continue
                got = singles[r].read(lo, hi - lo)   # everything resident, over the ring's end
                assert np.array_equal(_bits(got), _bits(exp[r][lo - SEEKS[r]:hi - SEEKS[r]])), (r, lo, hi)
                assert np.array_equal(_bits(multi[r].read(lo, hi - lo)), _bits(got)), (r, lo, hi)
            done += n
    finally:
        for s in singles + multi:
            s.close()


def _page_locked(torch, nbytes):
    """page-locked host memory from the allocator that owns it for the whole process"""
    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    return t, t.numpy()


@pytest.mark.parametrize("qua,regs,slot", [(2, (6, 6, 6), 1), (12, (12, 6, 3), 2), (12, (12, 6, 3), 0)], ids=_id)
def test_push_device_and_pinned_async_equal_host_push(gpu, torch_dev, qua, regs, slot):
    torch, dev = torch_dev
    S, rb = L.samples_per_round(qua, regs, slot), L.round_bytes(regs)
    fmt = _fmt(qua, regs, slot)
    pushes = _pushes(S)
    raw, data = _page_locked(torch, sum(pushes) // S * rb)
    data[:] = np.random.default_rng(45).integers(0, 256, data.size, dtype=np.uint8)
    original = data.copy()
    d_data = torch.from_numpy(original).to(dev)
    host, devr, pinned = _rings(gpu, 1)[0], _rings(gpu, 1)[0], _rings(gpu, 1)[0]
    try:
        done = 0
        for k, n in enumerate(pushes):
            b0, nb = done // S * rb, n // S * rb
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
        exp = L.decode(original, qua, regs, slot)
        assert np.array_equal(_bits(h[-m:]), _bits(np.conj(exp[-m:]).astype(np.complex64)))
    finally:
        for s in (host, devr, pinned):
            s.close()


def test_multi_push_device_and_pinned_async_equal_host_push(gpu, torch_dev):
    from gnss_sdr_amd.sample_stream import push_packed_multi, push_packed_multi_device, push_packed_multi_pinned_async
    torch, dev = torch_dev
    qua, chans = 12, [1, 2, 0]
    S, rb, fmt = L.samples_per_round(qua, EQUAL, 0), L.round_bytes(EQUAL), _fmt(qua, EQUAL)
    pushes = _pushes(S)
    raw, data = _page_locked(torch, sum(pushes) // S * rb)
    data[:] = np.random.default_rng(46).integers(0, 256, data.size, dtype=np.uint8)
    original = data.copy()
    d_data = torch.from_numpy(original).to(dev)
    host, devr, pinned = _rings(gpu), _rings(gpu), _rings(gpu)
    try:
        done = 0
        for k, n in enumerate(pushes):
            b0, nb = done // S * rb, n // S * rb
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
            exp = L.decode(original, qua, EQUAL, chans[r])
            m = pushes[-1]
            assert np.array_equal(_bits(h[-m:]), _bits(np.conj(exp[-m:]).astype(np.complex64))), r
    finally:
        for s in host + devr + pinned:
            s.close()


def test_push_refusals_leave_every_ring_untouched(gpu, torch_dev):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import PackedFormat as P, push_packed_multi, push_packed_multi_device, push_packed_multi_pinned_async
    torch, dev = torch_dev
    qua = 12
    S, rb, fmt = L.samples_per_round(qua, EQUAL, 0), L.round_bytes(EQUAL), _fmt(qua, EQUAL)
    data = _block(qua, EQUAL, LONG)[:128 * rb].copy()
    d_data = torch.from_numpy(data).to(dev)
    rings = _rings(gpu)
    assert push_packed_multi(rings, [0, 1, 2], fmt, data) == list(SEEKS)
    before = [(r.range(), r.read(r.range()[0], r.range()[1] - r.range()[0])) for r in rings]
    unequal = _fmt(qua, (12, 6, 3))
    too_long = (CAPS[0] // S + 1) * S
    big = np.zeros(too_long // S * rb, np.uint8)
    refused = [
        ("a partial triple", rings, [0, 1, 2], fmt, data, 2 * S + 4, "whole number of 24-byte triples"),
        ("unequal register counts", rings, [0, 1, 2], unequal, data, 8, "channels 0 and 1 hold 12 and 6 registers"),
        ("a ring twice", [rings[0], rings[1], rings[0]], [0, 1, 2], fmt, data, None, "named twice"),
        ("a slot twice", rings, [0, 1, 0], fmt, data, None, "named twice"),
        ("a slot out of range", rings, [0, 1, 3], fmt, data, None, "outside 0..2"),
        ("a slot that is not recorded", rings[:2], [0, 1], _fmt(qua, (6, 0, 6)), data, 8, "slot B) is not recorded"),
        ("more rings than slots", rings + [rings[0]], [0, 1, 2, 0], fmt, data, None, "4 rings"),
        ("QUA 12 without whole triples", rings[:1], [0], P.ls4(12, (4,)), data, 8, "QUA 12 with 4 registers"),
        ("larger than the smallest ring", rings, [0, 1, 2], fmt, big, too_long, "exceeds the ring capacity"),
    ]
    for push in (push_packed_multi, push_packed_multi_pinned_async):
        for what, rr, ch, f, d, n, text in refused:
            with pytest.raises(GshError) as e:
                push(rr, ch, f, d, n_samples=n)
            assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    for what, ptr, n, text in (("a misaligned block", d_data.data_ptr() + 4, S, "8-byte aligned"), ("a partial triple", d_data.data_ptr(), 12, "whole number")):
        with pytest.raises(GshError) as e:
            push_packed_multi_device(rings, [0, 1, 2], fmt, ptr, n)
        assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
        with pytest.raises(GshError) as e:
            rings[0].push_packed_device(fmt, ptr, n)
        assert e.value.code == 1 and text in str(e.value), (what, str(e.value))
    with pytest.raises(GshError) as e:
        rings[0].push_packed(_fmt(2, (0, 6, 0), 0), data, n_samples=16)
    assert "slot A) is not recorded" in str(e.value)
    for r, (rg, contents) in zip(rings, before):
        assert r.range() == rg
        assert np.array_equal(_bits(r.read(rg[0], rg[1] - rg[0])), _bits(contents))
    # and the rings still take the next block where they stood
    assert push_packed_multi(rings, [0, 1, 2], fmt, data) == [s + 128 * S for s in SEEKS]
    for r in rings:
        r.close()


def test_group_of_one_packed_push(gpu):
    from gnss_sdr_amd.sample_stream import StreamGroup
    qua, regs, slot = 12, (12, 6, 3), 1
    S, rb, fmt = L.samples_per_round(qua, regs, slot), L.round_bytes(regs), _fmt(qua, regs, slot)
    cap, win = 4102, 1024
    g = StreamGroup.local([gpu], cap, win, mode="broadcast")
    ring = g.ring(0)
    data = _block(qua, regs, LONG)
    exp = _expect(qua, regs, slot, LONG)
    try:
        done = 0
        for rounds in (101, 1, 0, 177, 100, 120, 101):   # 101 rounds = 16 968 bytes: not a multiple of the staging buffers' 16-byte padding
            n = rounds * S
            assert g.push_packed(fmt, data[done // S * rb:(done + n) // S * rb], n_samples=n) == done
            done += n
            g.wait()
            lo, hi = ring.range()
            assert (lo, hi) == (max(0, done - cap), done)
            assert np.array_equal(_bits(ring.read(lo, hi - lo)), _bits(exp[lo:hi]))
        assert done == LONG * S and done > 2 * cap
    finally:
        g.close()


@pytest.mark.parametrize("qua", [4, 12])
def test_packed_fir_equals_fir_of_the_unpacked_samples(gpu, torch_dev, qua):
    from gnss_sdr_amd.sample_stream import FirFilter, firdes_low_pass
    torch, dev = torch_dev
    regs, slot, D, fc, fs = (12, 6, 3), 1, 2, 1.1e6, 16.0e6
    S, rb, fmt = L.samples_per_round(qua, regs, slot), L.round_bytes(regs), _fmt(qua, regs, slot)
    taps = firdes_low_pass(1.0, fs, 2.0e6, 1.0e6)
    x = _expect(qua, regs, slot, LONG)
    d_data = torch.from_numpy(_block(qua, regs, LONG).copy()).to(dev)
    d_x = torch.from_numpy(x.copy()).to(dev)
    outs = []
    for packed in (True, False):
        f = FirFilter(taps, D, fc, fs, fmt if packed else "gr_complex", device=gpu)
        cap = x.size // D + 2
        d_y = torch.zeros(cap, dtype=torch.complex64, device=dev)
        pos, out = 0, 0
        for rounds in (1, 2, 5, 300, 3, 289):           # uneven blocks (whole rounds), the first ones shorter than the filter
            src = d_data.data_ptr() + rb * pos if packed else d_x.data_ptr() + 8 * pos * S
            out += f.process_device(src, rounds * S, d_y.data_ptr() + 8 * out, cap - out)
            pos += rounds
        assert pos == LONG
        torch.cuda.synchronize()
        outs.append(d_y.cpu().numpy()[:out])
        f.close()
    assert outs[0].size == (x.size + D - 1) // D and np.any(outs[0] != 0)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("filtered", [False, True], ids=["adapter_only", "filter"])
@pytest.mark.parametrize("qua", [4, 12])
def test_conditioner_takes_the_ls4_families(gpu, torch_dev, qua, filtered):
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import FirFilter, SampleStream, firdes_low_pass
    torch, dev = torch_dev
    regs, slot, D, fs = (12, 6, 3), 1, 2, 16.0e6
    S, rb, fmt = L.samples_per_round(qua, regs, slot), L.round_bytes(regs), _fmt(qua, regs, slot)
    x = np.conj(_expect(qua, regs, slot, LONG)).astype(np.complex64)    # pushed with inverted_spectrum
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
    data = _block(qua, regs, LONG)
    d_data = torch.from_numpy(data.copy()).to(dev)
    try:
        pos, made = 0, 0
        for k, rounds in enumerate((1, 2, 40, 5, 52, 100, 100, 100, 100, 100)):   # each block below the ring's capacity (QUA 4: 48 samples a round)
            if k & 1:
                first, n_out = cond.push_device(d_data.data_ptr() + rb * pos, rounds * S)
            else:
                first, n_out = cond.push(data[rb * pos:rb * (pos + rounds)], rounds * S)
            pos += rounds
            assert first == made
            made += n_out
            lo, hi = ring.range()
            assert hi == made
            assert np.array_equal(_bits(ring.read(lo, hi - lo)), _bits(exp[lo:hi])), (k, lo, hi)
        assert pos == LONG and made == exp.size
    finally:
        cond.close()
        ring.close()


def test_recording_pushes_into_rings(gpu, tmp_path):
    """LabSatRecording.push: a LabSat 4 file with seconds_to_skip into a triple's neighbourhood, two slots through the multi push, to the end of the data"""
    from gnss_sdr_amd.labsat import LabSatRecording
    from gnss_sdr_amd.sample_stream import SampleStream
    qua, regs, rounds = 12, (6, 6, 6), 40
    data = _block(qua, regs, rounds)
    (tmp_path / "r.ls4").write_bytes(data.tobytes())
    (tmp_path / "r.ini").write_text("[config]\nSMP=10000000\nQUA=12\nCHN=3\n" + "".join(f"[channel {x}]\nBUF_SIZE_{x}=48\n" for x in "ABC"))
    rec = LabSatRecording(str(tmp_path / "r.ls4"), (3, 1), seconds_to_skip=21.5e-7)    # 21 samples = 63 bytes: 1 buffer and 15 bytes: sample 16
    assert rec.position == 16 and rec.samples_per_round == 16 and rec.sample_rate == 1e7
    rec.position = 24                                   # inside round 1, at a triple boundary: the head of the first push is decoded on the host
    rings = [SampleStream(2048, 512, device=gpu) for _ in range(2)]
    try:
        got = 0
        for n in (20, 7, 100, 1000):
            got += rec.push(rings, n)
        assert got == 16 + 0 + 96 + (rounds * 16 - 24 - 112) and rec.remaining == 0 and rec.push(rings, 8) == 0
        for ring, slot in zip(rings, (2, 0)):
            assert ring.range() == (0, got)
            assert np.array_equal(_bits(ring.read(0, got)), _bits(_expect(qua, regs, slot, rounds)[24:]))
    finally:
        for r in rings:
            r.close()
