"""GPU test of the single-ring item entries of the sample ring (gsh_stream_push, _push_device on the ring's own and on a caller's stream, _push_async,
_push_staged, _push_pinned, _push_pinned_async; csrc/sample_stream.hip): fed the same blocks, every entry leaves the same ring behind.

One ring per entry, capacity 4098 and window 1024, and one block plan for all of them: 2600 is more than 1.5 times anything before it (every staging
buffer is outgrown and replaced once), 700 wraps, 4098 fills the ring and wraps, and the tail brings the four-slot and the two-slot staging rotations round
at least twice.  After every block each ring is compared bit for bit with the numpy model "the last 4098 samples of everything pushed"; at the end a
correlator bank bound to each ring correlates a window that straddles the capacity boundary (it reads the mirror) and must return the same bits on all
of them.  The argument checks every entry shares (capacity, item type, the empty push) are exercised on every entry."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import tracking_params_for

pytestmark = pytest.mark.gpu

CAP, WIN = 4098, 1024
PLAN = (1000, 1, 2600, 700, 0, 4098, 37, 512, 3, 900, 64)
ENTRIES = ("push", "push_device", "push_device_torch_stream", "push_async", "push_staged", "push_pinned", "push_pinned_async")
PAGE = 4096
_DTYPE = {"gr_complex": np.complex64, "ishort": np.int16, "ibyte": np.int8}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _blocks(item, rng):
    """the plan's blocks as host arrays (complex64 [n], or integer [n, 2] interleaved I,Q with the extremes in) and the complex64 samples they stand for"""
    out = []
    for n in PLAN:
        if item == "gr_complex":
            x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
            c = x
        else:
            info = np.iinfo(_DTYPE[item])
            x = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(_DTYPE[item])
            if n >= 2:
                x[:2] = [[info.min, info.max], [info.max, info.min]]
            c = (x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64)
        out.append((x, c))
    return out


class _Pinned:
    """page-aligned host memory, registered once (a GNU Radio buffer re-used for the whole run): every block of the plan lies in it behind the others"""

    def __init__(self, gsh, gpu, nbytes):
        self.gsh = gsh
        self.raw = np.zeros(nbytes + 2 * PAGE, np.uint8)
        off = (-self.raw.ctypes.data) % PAGE
        self.mem = self.raw[off:off + (nbytes + PAGE - 1) // PAGE * PAGE]
        assert gsh.gsh_host_register(gpu, C.c_void_p(self.mem.ctypes.data), self.mem.size) == 0
        self.used = 0

    def place(self, x):
        b = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        at = self.mem[self.used:self.used + b.size]
        at[:] = b
        self.used += b.size
        return at.view(x.dtype).reshape(x.shape)

    def release(self):
        assert self.gsh.gsh_host_unregister(C.c_void_p(self.mem.ctypes.data)) == 0


def _push_pinned(gsh, ring, a, item, inv):
    """gsh_stream_push_pinned on memory that is page-locked already (SampleStream.push_pinned registers its argument itself)"""
    from gnss_sdr_amd._lib import check
    from gnss_sdr_amd.sample_stream import ITEM_TYPES
    n = a.size if item == "gr_complex" else a.size // 2
    first = C.c_uint64(0)
    check(gsh.gsh_stream_push_pinned(ring._h, C.c_void_p(a.ctypes.data) if n else None, n, ITEM_TYPES[item], int(inv), C.byref(first)))
    return int(first.value)


@pytest.mark.parametrize("item,inv", [("gr_complex", False), ("gr_complex", True), ("ishort", False), ("ibyte", True)],
                         ids=["gr_complex", "gr_complex_inverted", "ishort", "ibyte_inverted"])
def test_every_item_entry_leaves_the_same_ring(gpu, gsh, item, inv):
    torch = pytest.importorskip("torch")
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking import CorrelatorBank
    dev = torch.device("cuda", gpu)
    blocks = _blocks(item, np.random.default_rng(23))
    pinned = _Pinned(gsh, gpu, sum(x.nbytes for x, _ in blocks))
    side = torch.cuda.Stream(device=dev)
    rings = {e: SampleStream(CAP, WIN, device=gpu) for e in ENTRIES}
    banks = []
    try:
        model = np.zeros(0, np.complex64)
        for x, c in blocks:
            d_x = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
            torch.cuda.synchronize()
            p_x = pinned.place(x)
            n = len(x)
            first = {
                "push": rings["push"].push(x, item, inv),
                "push_device": rings["push_device"].push_device(d_x.data_ptr(), n, item, inv),
                "push_device_torch_stream": rings["push_device_torch_stream"].push_device(d_x.data_ptr(), n, item, inv, hip_stream=side.cuda_stream),
                "push_async": rings["push_async"].push_async(x, item, inv),
                "push_staged": rings["push_staged"].push_staged(x, item, inv),
                "push_pinned": _push_pinned(gsh, rings["push_pinned"], p_x, item, inv),
                "push_pinned_async": rings["push_pinned_async"].push_pinned_async(p_x, item, inv),
            }
            # what each entry asks for before its samples are read
            side.synchronize()
            rings["push_async"].wait()
            rings["push_staged"].wait_copied()
            rings["push_pinned_async"].wait_copied()
            model = np.concatenate([model, np.conj(c) if inv else c])
            lo, hi = max(0, len(model) - CAP), len(model)
            for e in ENTRIES:
                assert first[e] == hi - n, (e, n)
                assert rings[e].range() == (lo, hi), (e, n)
                assert np.array_equal(_bits(rings[e].read(lo, hi - lo)), _bits(model[lo:hi])), (e, n)
        # a window across the capacity boundary runs into the mirror behind the ring's end
        hi = len(model)
        off = hi // CAP * CAP - WIN // 2 - 12
        assert hi - CAP <= off and off + WIN <= hi and off % CAP + WIN > CAP
        job = dict(sample_offset=off, n_samples=WIN, code_slot=0, shifts_chips=[-0.5, 0.0, 0.5], **tracking_params_for(4e6, 1000.0, np.random.default_rng(2)))
        outs = {}
        for e in ENTRIES:
            bank = CorrelatorBank(1, 1023, device=gpu)
            banks.append(bank)
            bank.set_code(0, oracle.ca_code(1))
            bank.set_stream_ring(rings[e])
            outs[e] = bank.correlate([job])
        assert np.any(outs["push"] != 0)
        for e in ENTRIES:
            assert np.array_equal(_bits(outs[e]), _bits(outs["push"])), e
    finally:
        for b in banks:
            b.close()
        for r in rings.values():
            r.close()
        pinned.release()


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_of_every_item_entry(gpu, gsh, entry):
    torch = pytest.importorskip("torch")
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd._lib import GSH_ITEM_GR_COMPLEX, check
    from gnss_sdr_amd.sample_stream import SampleStream
    dev = torch.device("cuda", gpu)
    host = np.zeros(CAP + 2, np.complex64)
    d_mem = torch.zeros(2 * (CAP + 2), dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ring = SampleStream(CAP, WIN, device=gpu)
    fn = getattr(gsh, "gsh_stream_" + entry.replace("_torch_stream", ""))

    def call(ptr, n, item_type):
        first = C.c_uint64(1 << 40)
        args = [ring._h, C.c_void_p(ptr) if ptr else None, n, item_type, 0]
        if entry.startswith("push_device"):
            args.append(C.c_void_p(side.cuda_stream) if entry.endswith("torch_stream") else None)
        check(fn(*args, C.byref(first)))
        return int(first.value)

    try:
        ptr = d_mem.data_ptr() if entry.startswith("push_device") else host.ctypes.data
        assert ring.push(np.ones(10, np.complex64)) == 0
        with pytest.raises(GshError):
            call(ptr, CAP + 2, GSH_ITEM_GR_COMPLEX)       # larger than the ring
        assert ring.range() == (0, 10)
        with pytest.raises(GshError):
            call(ptr, 4, 99)                              # no such item type
        assert ring.range() == (0, 10)
        assert call(0, 0, GSH_ITEM_GR_COMPLEX) == 10      # the empty push: the index the next sample will get, and nothing else
        assert ring.range() == (0, 10)
        assert np.array_equal(ring.read(0, 10), np.ones(10, np.complex64))
    finally:
        ring.close()
