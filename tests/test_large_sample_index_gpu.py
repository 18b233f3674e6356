"""GPU tests of everything that addresses the sample ring by absolute 64-bit index, at indices around and far past 2^31 and 2^32: the ring's pushes,
residency checks and mirror, the correlator banks, acquisition from a ring, the launched and the live tracking loop, the direct resampler's in0 / out0,
and the producers that write into a ring (conditioner, beamformer, signal generator).

Method: same ring layout, different high bits.  gsh_stream_seek positions an idle ring anywhere, so nothing here streams more than ~250 000 samples.
Every case runs twice with the same data and the same push sizes: once on a ring sought to the base B (every index handed in or got back is B + k), once
-- the control -- on a ring of the same capacity and window sought to b0 = B mod C (every index b0 + k; C is the capacity the ring really keeps:
gsh_stream_create rounds an odd one up).  Every sample then lies at the same ring position, address alignment and mirror position in both runs and
every window wraps at the same place: only the high part of the index differs.  The bar is therefore BIT EQUALITY of every output, index fields
shifted by B - b0; there is no tolerance in this file.  The control path itself is held to the oracles by the existing tests of each component.

Bases (n: the window length of the case): 2^31 - 5 n - 3 and 2^32 - 5 n - 3 (pushes and windows straddle the boundary -- each such case asserts that a
push and a window really contain the boundary index), 2^40 + 1, and 2^53 + 1 (odd and past the integers a double holds).

The one legitimate exception to "equal to the control": the signal generator's carrier phase depends on the absolute index, so its ring content is
held to tests/siggen_reference.py's exact model at B under test_siggen_gpu.py's bar.

Out of scope: the conditioner's and the FIR's own INPUT counters cannot be sought, so their arithmetic past 2^32 input samples is not reached here (the
double phase rev_per_sample * n of fetch_translated is the open item there); tests/test_large_sample_index.py covers the conditioner's host bookkeeping
at such counts."""
import ctypes as C
import functools
import os
import struct
import time

import numpy as np
import pytest

import oracle
from helpers import synth_gps_l1_stream, tracking_params_for

pytestmark = pytest.mark.gpu

N = 4000
BASE_IDS = ["2^31-5n-3", "2^32-5n-3", "2^40+1", "2^53+1"]


def _bases(n):
    """[(base, boundary index the case must straddle or None)] for a case whose window is n samples"""
    return [(2 ** 31 - 5 * n - 3, 2 ** 31), (2 ** 32 - 5 * n - 3, 2 ** 32), (2 ** 40 + 1, None), (2 ** 53 + 1, None)]


def _kept(cap):
    return cap + (cap & 1)


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _as_complex(a):
    a = np.asarray(a)
    return (a[:, 0].astype(np.float32) + 1j * a[:, 1].astype(np.float32)).astype(np.complex64)


def _inside(first, n, boundary):
    """does [first, first + n) hold the boundary index with at least one sample below it"""
    return boundary is not None and first < boundary < first + n


def _pair(gpu, cap, win, base):
    """(ring sought to base, control ring sought to b0, b0)"""
    from gnss_sdr_amd.sample_stream import SampleStream
    b0 = base % _kept(cap)
    rt, rc = SampleStream(cap, win, device=gpu), SampleStream(cap, win, device=gpu)
    rt.seek(base)
    rc.seek(b0)
    assert rt.range() == (base, base) and rc.range() == (b0, b0)
    return rt, rc, b0


# ---- 1. the ring itself against a numpy model -----------------------------------------------------------------------------------------------------
RING_PLAN = [("push", "ibyte", False, 1), ("push", "ishort", True, 2), ("push", "gr_complex", False, 3), ("push", "ibyte", True, 1023),
             ("push_pinned", "gr_complex", False, 4096), ("push_pinned", "gr_complex", True, 3333), ("push_pinned", "ishort", False, 2048),
             ("push_async", "ibyte", False, 7777), ("push_staged", "ishort", True, 4100), ("push_staged", "gr_complex", False, 0),
             ("push_device", "ibyte", True, 5000), ("push_device", "gr_complex", False, 31), ("push", "gr_complex", True, 8000),
             ("push_pinned", "gr_complex", False, 9000), ("push_async", "gr_complex", True, 5555), ("push_device", "ishort", False, 6001),
             ("push_staged", "ibyte", False, 4999), ("push_pinned", "ibyte", True, 777)]


@functools.lru_cache(maxsize=None)
def _ring_items():
    """the items of RING_PLAN and what the ring must hold of them, made once"""
    rng = np.random.default_rng(1117)
    items, model = [], []
    for _how, item, inv, n in RING_PLAN:
        if item == "gr_complex":
            x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
            c = x
        else:
            dt, lo, hi = (np.int8, -128, 128) if item == "ibyte" else (np.int16, -32768, 32768)
            x = rng.integers(lo, hi, size=(n, 2)).astype(dt)
            if n >= 2:
                x[:2] = [[lo, hi - 1], [hi - 1, lo]]
            c = _as_complex(x)
        x.setflags(write=False)
        items.append(x)
        model.append(np.conj(c) if inv else c)
    model = np.concatenate(model)
    model.setflags(write=False)
    return items, model


def _ring_run(gpu, start, boundary):
    """RING_PLAN into a ring sought to `start`, every push checked against the model -> pushes that held the boundary"""
    import torch
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    dev = torch.device("cuda", gpu)
    st = torch.cuda.current_stream().cuda_stream
    cap, win = 9 * N + 2, 2 * N
    items, model = _ring_items()
    s = SampleStream(cap, win, device=gpu)
    s.seek(start)
    pushed, straddled = 0, 0
    try:
        for (how, item, inv, n), x in zip(RING_PLAN, items):
            if how == "push_device":
                d = torch.from_numpy(np.array(x)).to(dev)
                first = s.push_device(d.data_ptr(), n, item, inverted_spectrum=inv, hip_stream=st)
                torch.cuda.synchronize()
            else:
                first = getattr(s, how)(np.array(x), item, inverted_spectrum=inv)
                if how in ("push_async", "push_staged"):
                    s.wait()
            assert first == start + pushed, (how, item, n, first - start, pushed)
            straddled += _inside(first, n, boundary)
            pushed += n
            lo, hi = s.range()
            assert (lo, hi) == (max(start, start + pushed - cap), start + pushed), (how, item, n)
            got = s.read(lo, hi - lo)
            assert np.array_equal(_bits(got), _bits(model[lo - start:hi - start])), (how, item, n, int(np.argmax(got != model[lo - start:hi - start])))
        assert pushed > cap + win       # the ring has wrapped, the mirror has been rewritten
        lo, hi = s.range()
        for index, n in ((lo - 1, 2), (hi - 1, 2), (lo - 1, 1), (hi, 1)):
            with pytest.raises(GshError):
                s.read(index, n)        # one sample below the oldest, one past the newest
        # back to a small index: empty there, and the next push lands there
        s.seek(17)
        assert s.range() == (17, 17)
        with pytest.raises(GshError):
            s.read(17, 1)
        assert s.push(np.array(items[4])) == 17 and s.range() == (17, 17 + len(items[4]))
        assert np.array_equal(_bits(s.read(17, len(items[4]))), _bits(items[4]))
    finally:
        s.close()
    return straddled


@pytest.mark.parametrize("base,boundary", _bases(N), ids=BASE_IDS)
def test_ring_pushes_reads_and_ranges_against_the_model(gpu, base, boundary):
    straddled = _ring_run(gpu, base, boundary)
    if boundary is not None:
        assert straddled == 1                                # one push begins below the boundary index and ends above it
    _ring_run(gpu, base % _kept(9 * N + 2), None)           # the control: the same ring positions at a small index


PACKED_WIN = 1024
PACKED_PUSHES = [1024, 8, 0, 2048, 520, 4096, 16, 3000, 1024, 2048, 4000, 1504]   # samples per band: whole words
PACKED_CAPS = (4102, 5004, 6150)                                                   # two rings of the multi push, one of the single push


@pytest.mark.parametrize("base,boundary", _bases(PACKED_WIN), ids=BASE_IDS)
def test_packed_pushes_into_sought_rings(gpu, base, boundary):
    """gsh_stream_push_packed and the two-ring gsh_stream_push_packed_multi (GSS6450, 4-bit, two bands) against tests/gss6450_reference.py"""
    import gss6450_reference as R
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import PackedFormat, SampleStream, push_packed_multi
    nch, spw, chans, single_ch = 2, 4, [1, 0], 0
    fmt = PackedFormat.from_signal_source("Spir_GSS6450_File_Signal_Source", adc_bits=4, total_channels=nch, sel_ch=1, endian=False)
    total = sum(PACKED_PUSHES)
    data = np.random.default_rng(64).integers(0, 256, total // spw * 4 * nch, dtype=np.uint8)
    exp = [np.conj(R.source_output(data, 4, nch, ch + 1, False)).astype(np.complex64) for ch in chans + [single_ch]]   # inverted spectrum
    caps = [_kept(c) for c in PACKED_CAPS]
    straddled = 0
    for control in (False, True):
        starts = [base % c if control else base for c in caps]
        rings = [SampleStream(c, PACKED_WIN, device=gpu) for c in PACKED_CAPS]
        for r, s0 in zip(rings, starts):
            r.seek(s0)
        done = 0
        try:
            for n in PACKED_PUSHES:
                nb = n // spw * 4 * nch
                block = data[done // spw * 4 * nch:done // spw * 4 * nch + nb]
                first = push_packed_multi(rings[:2], chans, fmt, block, True, n_samples=n)
                first.append(rings[2].push_packed(fmt.with_channel(single_ch), block, True, n_samples=n))
                for r in range(3):
                    assert first[r] == starts[r] + done, (control, r, n)
                    straddled += (not control) and _inside(first[r], n, boundary)
                    hi = starts[r] + done + n
                    lo = max(starts[r], hi - caps[r])
                    assert rings[r].range() == (lo, hi), (control, r, n)
                    got = rings[r].read(lo, hi - lo)
                    assert np.array_equal(_bits(got), _bits(exp[r][lo - starts[r]:hi - starts[r]])), (control, r, n)
                done += n
            assert done > 3 * max(caps)
            for r in range(3):
                lo, hi = rings[r].range()
                with pytest.raises(GshError):
                    rings[r].read(lo - 1, 1)
                with pytest.raises(GshError):
                    rings[r].read(hi, 1)
        finally:
            for r in rings:
                r.close()
    if boundary is not None:
        assert straddled == 3    # the same push in each of the three rings


# ---- 2. correlator banks bound to the ring --------------------------------------------------------------------------------------------------------
FS = 4e6
BANK_CAP, BANK_WIN, BANK_BLOCK = 9 * N + 2, 2 * N, 3 * N + 17
EPL = [-0.5, 0.0, 0.5]


@functools.lru_cache(maxsize=None)
def _bank_stream():
    total = 40 * N
    x = synth_gps_l1_stream(total, FS, [1, 2, 3], [1000.0, -2000.0, 300.0], [5.0, 300.0, 800.0], seed_noise=8)
    x8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 30.0), -127, 127).astype(np.int8)   # what an 8-bit front-end delivers
    rng = np.random.default_rng(2)
    params = [tracking_params_for(FS, d, rng) for d in (1000.0, -2000.0, 300.0)]
    x8.setflags(write=False)
    return x8, params


def _banks(gpu, rings):
    from gnss_sdr_amd.tracking import CorrelatorBank
    banks = []
    for ring in rings:
        b = CorrelatorBank(3, 1023, device=gpu)
        for c in range(3):
            b.set_code(c, oracle.ca_code(c + 1))
        b.set_stream_ring(ring)
        banks.append(b)
    return banks


def _resident_windows(lo, hi, n, b0, cap):
    """(channel, offset relative to the ring's start) of a few resident windows of n samples per channel, newest first, and per channel the newest
    resident window that runs over the ring's end into the mirror (the ring's end lies where (b0 + offset) mod cap is 0)"""
    out = []
    for c in range(3):
        for k in range(3):
            off = hi - n - k * (n // 2 + 3) - c
            if off >= lo:
                out.append((c, off))
        over = (hi - n - c) - ((b0 + hi - n - c) - (cap - n // 2)) % cap      # the newest offset <= hi - n - c with (b0 + offset) mod cap = cap - n / 2
        if over - c >= lo:
            out.append((c, over - c))
    return out


WIDE_SHIFTS = {"wide5": list(np.linspace(-1.0, 1.0, 5)), "wide33": list(np.linspace(-2.0, 2.0, 33))}


@pytest.mark.parametrize("flavour", ["plain", "fusion", "splits4", "walk", "wide5", "wide33"])
@pytest.mark.parametrize("base,boundary", _bases(N), ids=BASE_IDS)
def test_banks_on_a_ring_at_a_large_index_equal_the_control(gpu, gsh, base, boundary, flavour):
    """the pattern of test_sample_stream_gpu.py::test_bank_bound_to_ring_matches_flat_buffer: three channels, windows of 4 000 samples, a few per push,
    newest first.  plain / fusion / splits4: the narrow bank with E/P/L jobs and a single-tap job behind each (its fusion partner); walk: a batch of
    E/P/L jobs large enough for the resident round of work-groups (gsh_mcorr_walk_launches must advance); wide5 / wide33: gsh_bank_correlate_wide."""
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.tracking import make_jobs
    x8, params = _bank_stream()
    total = len(x8)
    # splits4: gsh_bank_set_splits keeps 2 048 samples per work-group, so four splits need windows of 8 192 samples or more
    n_win = 8200 if flavour == "splits4" else N
    max_win = max(BANK_WIN, n_win)
    rt, rc, b0 = _pair(gpu, BANK_CAP, max_win, base)
    cap = _kept(BANK_CAP)
    bank_t, bank_c = _banks(gpu, (rt, rc))
    wide = flavour.startswith("wide")
    for b in (bank_t, bank_c):
        if flavour in ("plain", "walk"):
            b.set_pair_fusion(False)
        elif flavour == "fusion":
            b.set_pair_fusion(True)
        elif flavour == "splits4":
            b.set_splits(4)
    if flavour == "walk":
        assert gsh.gsh_mcorr_walk_capacity() > 0
        n_big = max(5120, 2 * gsh.gsh_mcorr_walk_capacity()) + 3      # two-wave work-groups, and two resident rounds of them
    pushed = n_wrapping = n_boundary = n_push_boundary = n_batches = 0
    try:
        for i, blk in enumerate(range(0, total, BANK_BLOCK)):
            m = min(BANK_BLOCK, total - blk)
            assert rt.push(x8[blk:blk + m], "ibyte") == base + pushed
            assert rc.push(x8[blk:blk + m], "ibyte") == b0 + pushed
            n_push_boundary += _inside(base + pushed, m, boundary)
            pushed += m
            lo, hi = max(0, pushed - cap), pushed
            assert rt.range() == (base + lo, base + hi) and rc.range() == (b0 + lo, b0 + hi)
            windows = _resident_windows(lo, hi, n_win, b0, cap)
            if not windows:
                continue
            holds = any(_inside(base + off, n_win, boundary) for _c, off in windows)
            if flavour == "walk" and not (i % 4 == 1 or holds or blk + m == total):
                continue        # a few of the large batches: every fourth block, the ones with the boundary index, the last block
            rows = []
            for c, off in windows:
                if wide:
                    rows.append(dict(sample_offset=off, n_samples=n_win, code_slot=c, shifts_chips=WIDE_SHIFTS[flavour], **params[c]))
                    continue
                rows.append(dict(sample_offset=off, n_samples=n_win, code_slot=c, shifts_chips=EPL, **params[c]))
                if flavour != "walk":
                    rows.append(dict(sample_offset=off, n_samples=n_win, code_slot=c, shifts_chips=[0.25], **params[c]))   # rides on the job in front when fused
            n_wrapping += sum((b0 + off) % cap + n_win > cap for _c, off in windows)
            n_boundary += sum(_inside(base + off, n_win, boundary) for _c, off in windows)
            if flavour == "walk":
                rows = [rows[j % len(rows)] for j in range(n_big)]
            outs = []
            for bank, b in ((bank_t, base), (bank_c, b0)):
                if wide:
                    outs.append(bank.correlate_wide([dict(r, sample_offset=r["sample_offset"] + b) for r in rows]))
                    continue
                jobs = make_jobs(rows)
                for j, r in zip(jobs, rows):
                    j.sample_offset = r["sample_offset"] + b
                assert jobs[0].sample_offset == rows[0]["sample_offset"] + b
                walked = gsh.gsh_mcorr_walk_launches()
                outs.append(bank.correlate(jobs))
                if flavour == "walk":
                    assert gsh.gsh_mcorr_walk_launches() == walked + 1, "the batch did not take the walk"
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (i, int(np.argmax(np.any(outs[0] != outs[1], axis=1))))
            assert np.all(np.any(outs[0] != 0, axis=1))
            n_batches += 1
        assert pushed == total and n_wrapping >= 3 and n_batches >= 3, (n_wrapping, n_batches)
        if boundary is not None:
            assert n_push_boundary == 1 and n_boundary >= 2, (n_push_boundary, n_boundary)
        # the residency refusals of the flat-buffer test, at the base
        corr = (lambda b, rows: b.correlate_wide(rows)) if wide else (lambda b, rows: b.correlate(rows))
        sh = WIDE_SHIFTS[flavour] if wide else [0.0]
        lo, hi = rt.range()
        assert lo > base
        for off, n in ((lo - 1, N), (hi - N + 1, N), (lo, max_win + 1)):      # below the oldest, past the newest, longer than max_window
            with pytest.raises(GshError):
                corr(bank_t, [dict(sample_offset=off, n_samples=n, code_slot=0, shifts_chips=sh)])
        corr(bank_t, [dict(sample_offset=lo, n_samples=max_win, code_slot=0, shifts_chips=sh)])    # ... and what just fits is taken
    finally:
        for b in (bank_t, bank_c):
            b.close()
        rt.close()
        rc.close()


@pytest.mark.parametrize("base,boundary", _bases(N), ids=BASE_IDS)
def test_one_relative_job_table_follows_the_sample_base_block_after_block(gpu, base, boundary):
    """gsh_bank_set_sample_base: the table holds window positions relative to a block's first sample and is staged once, while the ring still stands at
    index 0 and holds block 0 (staging checks residency of the offsets as they are); then the ring is sought and every block is launched with the base
    B + k block."""
    x8, params = _bank_stream()
    rows = []
    for c in range(3):
        for off in [k * (N // 2 + 3) + 7 * c for k in range(4)] + [BANK_BLOCK - N - c]:      # the windows cover the whole block: every wrap position occurs
            rows.append(dict(sample_offset=off, n_samples=N, code_slot=c, shifts_chips=EPL, **params[c]))
    assert max(r["sample_offset"] for r in rows) + N == BANK_BLOCK
    from gnss_sdr_amd.sample_stream import SampleStream
    cap = _kept(BANK_CAP)
    b0 = base % cap
    rt, rc = SampleStream(BANK_CAP, BANK_WIN, device=gpu), SampleStream(BANK_CAP, BANK_WIN, device=gpu)
    bank_t, bank_c = _banks(gpu, (rt, rc))
    n_boundary = n_push_boundary = n_wrapping = 0
    try:
        for ring, bank, b in ((rt, bank_t, base), (rc, bank_c, b0)):
            bank.set_splits(1)
            assert ring.push(x8[:BANK_BLOCK], "ibyte") == 0
            bank.upload_jobs(rows)
            bank.synchronize()
            ring.seek(b)
        for k in range(8):
            blk = x8[k * BANK_BLOCK:(k + 1) * BANK_BLOCK]
            outs = []
            for ring, bank, b in ((rt, bank_t, base), (rc, bank_c, b0)):
                first = ring.push(blk, "ibyte")
                assert first == b + k * BANK_BLOCK
                bank.set_sample_base(first)
                bank.launch()
                bank.synchronize()
                outs.append(bank.read_outputs())
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), k
            assert np.all(np.any(outs[0][:, :3] != 0, axis=1))
            first = base + k * BANK_BLOCK
            n_push_boundary += _inside(first, BANK_BLOCK, boundary)
            for r in rows:
                n_boundary += _inside(first + r["sample_offset"], N, boundary)
                n_wrapping += (b0 + k * BANK_BLOCK + r["sample_offset"]) % cap + N > cap
        assert n_wrapping >= 3
        if boundary is not None:
            assert n_push_boundary == 1 and n_boundary >= 2, (n_push_boundary, n_boundary)
        # a base that points past the newest sample is refused, at the large index as well
        from gnss_sdr_amd import GshError
        bank_t.set_sample_base(base + 8 * BANK_BLOCK)
        with pytest.raises(GshError):
            bank_t.launch()
    finally:
        for b in (bank_t, bank_c):
            b.close()
        rt.close()
        rc.close()


# ---- 3. acquisition from the ring -----------------------------------------------------------------------------------------------------------------
def _result_bits(r):
    return tuple(v if isinstance(v, int) else struct.pack("<f", v) for v in r.values())


@pytest.mark.parametrize("path", ["onchip", "fourstep"])
@pytest.mark.parametrize("base,boundary", _bases(N), ids=BASE_IDS)
def test_acquisition_from_a_ring_at_a_large_index_equals_the_control(gpu, base, boundary, path):
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank
    x8, _params = _bank_stream()
    kw = dict(fs_in=int(FS), fft_size=N, doppler_max=5000, doppler_step=250, samples_per_chip=4, samples_per_code=float(N), max_prn=3,
              transform_path=1 if path == "fourstep" else 0)
    rt, rc, b0 = _pair(gpu, BANK_CAP, BANK_WIN, base)
    cap = _kept(BANK_CAP)
    acqs = []
    try:
        for _ in range(2):
            a = PcpsAcquisitionBank(device=gpu, **kw)
            for p in range(3):
                a.set_local_code(p, oracle.ca_code_complex_sampled(p + 1, int(FS)))
            acqs.append(a)
        pushed, n_push_boundary = 0, 0
        for k in range(3):                                       # 36 051 samples through a ring of 36 002: the third push wraps
            blk = x8[k * BANK_BLOCK:(k + 1) * BANK_BLOCK]
            assert rt.push(blk, "ibyte") == base + pushed and rc.push(blk, "ibyte") == b0 + pushed
            n_push_boundary += _inside(base + pushed, len(blk), boundary)
            pushed += len(blk)
        lo = pushed - cap
        assert lo > 0
        # the block that holds the boundary index of the straddling bases (index B + 5 n + 3), the oldest and the newest one, and the one that runs over
        # the ring's end into the mirror when it is resident
        offs = [5 * N + 3 - N // 2, lo, pushed - N]
        over_end = (cap - N // 2 - b0) % cap
        if lo <= over_end <= pushed - N:
            offs.append(over_end)
        for off in offs:
            got = acqs[0].dwell_ring(rt, base + off, 3)
            want = acqs[1].dwell_ring(rc, b0 + off, 3)
            for p in range(3):
                assert _result_bits(got[p]) == _result_bits(want[p]), (off, p, got[p], want[p])
            assert np.array_equal(acqs[0].read_grid(0).view(np.uint32), acqs[1].read_grid(0).view(np.uint32)), off
            assert all(g["peak"] > 0.0 for g in got)
        if boundary is not None:
            assert n_push_boundary == 1 and _inside(base + offs[0], N, boundary)
        # residency at the base: a block that begins below the oldest sample or ends past the newest is refused
        from gnss_sdr_amd import GshError
        for off in (lo - 1, pushed - N + 1):
            with pytest.raises(GshError):
                acqs[0].dwell_ring(rt, base + off, 3)
    finally:
        for a in acqs:
            a.close()
        rt.close()
        rc.close()


# ---- 4. launched tracking loop on the ring --------------------------------------------------------------------------------------------------------
LOOP_EPOCHS = 60
LOOP_CAP = 23 * N + 7


@functools.lru_cache(maxsize=None)
def _loop_scenario():
    """the scenario of test_tracking_loop_gpu.py::test_loop_follows_a_live_ring, 60 periods long"""
    prns, dops, cphs = [5, 18], [-1900.0, 3300.0], [100.0, 900.5]
    total = (LOOP_EPOCHS + 3) * N
    x = synth_gps_l1_stream(total, FS, prns, dops, cphs, cn0_dbhz=47.0, seed_noise=77)
    x8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 25.0), -127, 127).astype(np.int8)
    x8.setflags(write=False)
    starts = [int(round((1023.0 - cph) / (1.023e6 * (1 + fd / 1575.42e6)) * FS)) for fd, cph in zip(dops, cphs)]
    return prns, dops, starts, total, x8


def _shifted_bytes(records, shift):
    """the records' bytes with sample_counter moved down by `shift`"""
    from gnss_sdr_amd._lib import TrkEpoch
    out = []
    for r in records:
        q = TrkEpoch()
        C.memmove(C.byref(q), C.byref(r), C.sizeof(TrkEpoch))
        q.sample_counter = r.sample_counter - shift
        out.append(bytes(memoryview(q)))
    return b"".join(out)


def _loop_run(gpu, start, variant, boundary):
    """the live-ring scenario on a ring sought to `start` -> (records per channel, pushes that held the boundary)"""
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking_loop import TrackingLoop, kf_conf, trk_conf
    prns, dops, starts, total, x8 = _loop_scenario()
    kw = dict(fs_in=FS, vector_length=N, pll_bw_hz=35.0, dll_bw_hz=3.0, enable_lock_detectors=1)
    if variant == "kalman":
        kw.update(early_late_space_chips=0.25, spc=0.25)      # Kf_Conf's spacing
    ring = SampleStream(LOOP_CAP, 2 * N, device=gpu)
    ring.seek(start)
    loop = TrackingLoop(trk_conf(**kw), 2, 1023, device=gpu)
    late = None
    try:
        if variant == "split2":
            loop.set_split(2)
        if variant == "kalman":
            loop.set_kalman(kf_conf())
        loop.set_stream_ring(ring)
        for ch in range(2):
            loop.start(ch, oracle.ca_code(prns[ch]), start + starts[ch], start, dops[ch] + 6.0)
        rec = [[], []]
        pushed, blk, n_calls, n_push_boundary = 0, 9 * N + N // 2, 0, 0
        while pushed < total:
            m = min(blk, total - pushed)
            assert ring.push(x8[pushed:pushed + m], "ibyte") == start + pushed
            n_push_boundary += _inside(start + pushed, m, boundary)
            pushed += m
            got, done = loop.run(12)           # more than a block holds: the loop stops at the newest sample by itself
            n_calls += 1
            for ch in range(2):
                assert done[ch] <= 10
                rec[ch] += got[ch]
        assert n_calls >= 6 and pushed > 2 * _kept(LOOP_CAP)
        for ch in range(2):
            assert len(rec[ch]) >= LOOP_EPOCHS and rec[ch][0].sample_counter == start + starts[ch]
            assert rec[ch][-1].sample_counter + 2 * N > start + total - N      # worked through to the newest samples
        # a channel that falls further behind than the ring holds stops instead of reading overwritten samples
        late = TrackingLoop(trk_conf(**kw), 1, 1023, device=gpu)
        late.set_stream_ring(ring)
        late.start(0, oracle.ca_code(prns[0]), start + starts[0], start, dops[0])
        _rec, done = late.run(5)
        assert done[0] == 0
    finally:
        if late is not None:
            late.close()
        loop.close()
        ring.close()
    return rec, n_push_boundary


LOOP_CASES = [(b, bd, "plain", i) for (b, bd), i in zip(_bases(N), BASE_IDS)] + [(b, bd, "split2", i) for (b, bd), i in zip(_bases(N), BASE_IDS)]
LOOP_CASES.append(_bases(N)[1] + ("kalman", BASE_IDS[1]))


@pytest.mark.parametrize("base,boundary,variant", [c[:3] for c in LOOP_CASES], ids=[f"{c[3]}-{c[2]}" for c in LOOP_CASES])
def test_launched_loop_on_a_ring_at_a_large_index_equals_the_control(gpu, base, boundary, variant):
    b0 = base % _kept(LOOP_CAP)
    rec_t, n_push_boundary = _loop_run(gpu, base, variant, boundary)
    rec_c, _ = _loop_run(gpu, b0, variant, None)
    for ch in range(2):
        assert len(rec_t[ch]) == len(rec_c[ch])
        assert _shifted_bytes(rec_t[ch], base - b0) == _shifted_bytes(rec_c[ch], 0), f"channel {ch}: records at the base differ from the control's"
        if boundary is not None:
            # sample_counter is a window's first sample and the windows follow one another without a gap: the one that begins last below the
            # boundary index holds it
            below = [r for r in rec_t[ch] if r.sample_counter < boundary]
            assert 0 < len(below) < len(rec_t[ch]), ch
    if boundary is not None:
        assert n_push_boundary == 1


# ---- 5. live residency ----------------------------------------------------------------------------------------------------------------------------
LIVE_FS, LIVE_N, LIVE_EPOCHS = 2.046e6, 2046, 60
LIVE_CAP = 23 * LIVE_N + 7
LIVE_KW = dict(fs_in=LIVE_FS, vector_length=LIVE_N, pll_bw_hz=25.0, dll_bw_hz=2.0, enable_lock_detectors=1, pull_in_time_s=0, cn0_min=32, max_code_lock_fail=50)


@functools.lru_cache(maxsize=None)
def _live_scenario():
    """the scenario of test_tracking_live_gpu.py (two satellites and a channel that searches one that is not there), 60 periods long, 8-bit items"""
    prns, dops, cphs = [5, 18], [-1900.0, 3300.0], [100.0, 900.5]
    total = (LIVE_EPOCHS + 3) * LIVE_N
    x = synth_gps_l1_stream(total, LIVE_FS, prns, dops, cphs, cn0_dbhz=47.0, seed_noise=77)
    x8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 25.0), -127, 127).astype(np.int8)
    x8.setflags(write=False)
    starts = [int(round((1023.0 - cph) / (1.023e6 * (1 + fd / 1575.42e6)) * LIVE_FS)) for fd, cph in zip(dops, cphs)]
    return prns + [27], dops + [500.0], starts + [1234], total, x8


def _live_run(gpu, start):
    """records of the three channels, taken with limits that move with `start`; the residency and idle budgets are the defaults the existing test runs with"""
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking_loop import TrackingLoop, trk_conf
    prns, dops, starts, total, x8 = _live_scenario()
    ring = SampleStream(LIVE_CAP, 2 * LIVE_N, device=gpu)
    ring.seek(start)
    live = TrackingLoop(trk_conf(**LIVE_KW), 3, 1023, device=gpu)
    got = [[], [], []]

    def drain(limit, want, deadline_s):
        """poll until every channel has `want` records (None: until nothing arrives any more and no residency is in flight)"""
        t_end = time.time() + deadline_s
        quiet_since = time.time()
        while time.time() < t_end:
            progress = False
            for ch in range(3):
                rec, _pending, nw, _active = live.live_take(ch, 64, limit_end=limit)
                for r in rec:
                    assert start <= r.sample_counter and r.sample_counter + max(LIVE_N, r.prn_length_samples) <= limit
                if rec:
                    got[ch] += rec
                    progress = True
                    assert rec[-1].sample_counter < nw <= start + total
            if progress:
                quiet_since = time.time()
            elif want is not None and all(len(got[ch]) >= want[ch] for ch in range(3)):
                return
            elif time.time() - quiet_since > 0.05 and live.live_in_flight() == 0:
                return
            else:
                time.sleep(0.0005)

    try:
        live.set_stream_ring(ring)
        for ch in range(3):
            live.start(ch, oracle.ca_code(prns[ch]), start + starts[ch], start, dops[ch] + 6.0)
        pushed, blk = 0, 9 * LIVE_N + LIVE_N // 2
        while pushed < total:
            m = min(blk, total - pushed)
            assert ring.push(x8[pushed:pushed + m], "ibyte") == start + pushed
            pushed += m
            if live.live_in_flight() == 0:
                live.live_begin()
            # records are taken up to one period short of what has been pushed: the limit moves with the ring's base
            limit = start + pushed - LIVE_N
            want = [max(0, (pushed - LIVE_N - starts[ch]) // LIVE_N - 1) for ch in range(3)]
            drain(limit, want, 2.0)
            for ch in range(3):
                assert len(got[ch]) >= want[ch], (ch, len(got[ch]), want[ch], pushed)
        # everything the stream holds: until the residency has run out of work and left by itself, so that both runs end with the same record
        want = [max(0, (total - starts[ch]) // LIVE_N - 1) for ch in range(3)]
        drain(2 ** 64 - 1, None, 1.0)
        live.live_quiesce()
        drain(2 ** 64 - 1, None, 0.2)
        for ch in range(3):
            assert len(got[ch]) >= want[ch] >= LIVE_EPOCHS - 2, (ch, len(got[ch]), want[ch])
            assert got[ch][0].sample_counter == start + starts[ch]
    finally:
        live.close()
        ring.close()
    return got


@pytest.mark.parametrize("base", [_bases(LIVE_N)[1][0], _bases(LIVE_N)[3][0]], ids=[BASE_IDS[1], BASE_IDS[3]])
def test_live_records_at_a_large_index_equal_the_control(gpu, base):
    b0 = base % _kept(LIVE_CAP)
    rec_t = _live_run(gpu, base)
    rec_c = _live_run(gpu, b0)
    for ch in range(3):
        assert len(rec_t[ch]) == len(rec_c[ch]), (ch, len(rec_t[ch]), len(rec_c[ch]))
        assert _shifted_bytes(rec_t[ch], base - b0) == _shifted_bytes(rec_c[ch], 0), f"channel {ch}: live records at the base differ from the control's"
    if base < 2 ** 40:
        assert sum(_inside(r.sample_counter, r.prn_length_samples, 2 ** 32) for r in rec_t[0]) == 1


# ---- 6. direct resampler at large in0 / out0 ------------------------------------------------------------------------------------------------------
RATIOS = [(25e6, 4e6), (32e6, 4e6), (50e6, 25e6), (4e6, 4e6), (12.5e6, 2.048e6), (2.048e6, 2.046e6), (5e6, 4999999.0), (3e6, 1e6),
          (4e6, 10e6), (2.046e6, 8.184e6), (1e6, 1.000001e6), (7e6, 2e6)]       # those of tests/test_resampler.py
OUT0S = [2 ** 32 - 7, 2 ** 32 + 12345, 2 ** 52 + 1]                              # the last two put out0 2^32 beyond 64 bits
RS_N = 50021


def _phase_step(fs_in, fs_out):
    """(step, decimating) in the reference's operation order (direct_resampler_conditioner_cc.cc:52-59: floor(2^32 * fs_out / fs_in), the product first);
    step 0 stands for a ratio of one"""
    dec = fs_in >= fs_out
    v = np.floor(4294967296.0 * fs_out / fs_in) if dec else np.floor(4294967296.0 * fs_in / fs_out)
    return (0 if v >= 4294967296.0 else int(v)), dec


def _input_index(j, step, dec):
    """the closed form in Python integers (j: an int or an object array of ints): decimation ceil(j 2^32 / step), interpolation floor((j + 1) step / 2^32)"""
    if step == 0:
        return j
    if dec:
        return -((-j * (1 << 32)) // step)
    return ((j + 1) * step) >> 32


@functools.lru_cache(maxsize=None)
def _rs_input():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(RS_N) + 1j * rng.standard_normal(RS_N)).astype(np.complex64)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("out0", OUT0S, ids=["2^32-7", "2^32+12345", "2^52+1"])
@pytest.mark.parametrize("fs_in,fs_out", RATIOS)
def test_resampler_at_large_in0_and_out0_equals_the_closed_form(gpu, fs_in, fs_out, out0):
    import torch
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import direct_resample_device
    dev = torch.device("cuda", gpu)
    step, dec = _phase_step(fs_in, fs_out)
    x = _rs_input()
    in0 = _input_index(out0, step, dec)          # the input index that feeds out0: x[0]
    assert in0 < 2 ** 63
    d_x = torch.from_numpy(np.array(x)).to(dev)
    cap = int(RS_N * max(1.0, fs_out / fs_in)) + 16
    d_y = torch.full((cap, 2), -77.25, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    # every output index the input can feed, and the input index of each, once
    j_all = np.arange(cap + 8).astype(object) + out0
    i_all = _input_index(j_all, step, dec)
    rel = np.array([int(i) - in0 for i in i_all], dtype=np.int64)
    assert rel[0] == 0 and np.all(np.diff(rel) >= 0) and rel[-1] >= RS_N
    n_done, in_pos, calls = 0, 0, 0              # outputs made, inputs consumed (relative to out0 / in0)
    for blk in (1, 4097, 10000, 33, 20000, RS_N):      # the ragged blocks of tests/test_resampler.py, scaled to a stream of 50 021 samples
        hi = min(RS_N, in_pos + blk)
        if hi <= in_pos:
            break
        n_out, n_cons = direct_resample_device(gpu, d_x.data_ptr() + 8 * in_pos, in0 + in_pos, hi - in_pos, fs_in, fs_out, out0 + n_done,
                                               d_y.data_ptr() + 8 * n_done, cap - n_done, hip_stream=st)
        # the closed form's answer: the outputs from out0 + n_done on whose input lies below in0 + hi; consumed: up to and including the last one's input
        # (decimation) or up to it (interpolation)
        want_out = int(np.searchsorted(rel, hi, side="left")) - n_done
        assert 0 <= want_out <= cap - n_done
        want_cons = 0 if want_out == 0 else int(rel[n_done + want_out - 1]) + (1 if dec else 0) - in_pos
        assert (n_out, n_cons) == (want_out, want_cons), (blk, in_pos, n_done, n_out, n_cons, want_out, want_cons)
        n_done += n_out
        in_pos += n_cons
        calls += 1
        if n_cons == 0 and n_out == 0 and hi == RS_N:
            break
    torch.cuda.synchronize()
    assert calls >= 5 and n_done > 0.9 * RS_N * min(1.0, fs_out / fs_in)
    got = d_y.cpu().numpy().view(np.complex64).reshape(-1)
    assert np.array_equal(_bits(got[:n_done]), _bits(x[rel[:n_done]]))
    assert np.all(got[n_done:] == np.complex64(-77.25 - 77.25j))      # nothing written past the outputs
    # a call whose first output needs an input before the block's first sample is refused
    with pytest.raises(GshError):
        direct_resample_device(gpu, d_x.data_ptr(), in0 + 1, 100, fs_in, fs_out, out0, d_y.data_ptr(), cap, hip_stream=st)
    torch.cuda.synchronize()


# ---- 7. producers into a sought ring --------------------------------------------------------------------------------------------------------------
COND_WIN = 512
COND_BLOCKS = [1, 7, 100, 4099, 3, 5000, 2797]                   # the cuts of tests/test_conditioner_gpu.py over 12 007 input samples
CW = ((1500, 1500, 6.0, 0.071), (5000, 2500, 3.0, -0.19), (9000, 800, 10.0, 0.33))   # (start, length, amplitude, cycles per sample)


def _cond_taps(K, D):
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (2.5 * D))).astype(np.float32)
    return t / t.sum()


def _cond_case(name):
    """-> (raw items, the conditioner's keywords, ring capacity)"""
    n = sum(COND_BLOCKS)
    rng = np.random.default_rng(len(name))
    if name == "fir_resampler":
        raw = rng.integers(-100, 101, (n, 2)).astype(np.int8)
        return raw, dict(input_kind="ibyte", inverted_spectrum=True, taps=_cond_taps(33, 2), decimation=2, center_freq_hz=1.2e6, sampling_freq_hz=8e6,
                         fs_in=4e6, fs_out=2.5e6), 3001
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    if name == "blanked":
        for s in range(700, n, 1900):
            x[s:s + 90] *= 25.0                                  # pulses far above the noise floor
        return x, dict(input_kind="gr_complex", blanking=dict(pfa=0.04, length=32, segments_est=40, segments_reset=100)), 5003
    for s, w, a, f in CW:
        x[s:s + w] += (a * np.exp(2j * np.pi * f * np.arange(w))).astype(np.complex64)
    return x, dict(input_kind="gr_complex", notch=dict(length=32, segments_est=40, segments_reset=100, pfa=0.001, p_c_factor=0.9)), 5003


@pytest.mark.parametrize("name", ["fir_resampler", "blanked", "notched"])
@pytest.mark.parametrize("base,boundary", _bases(COND_WIN), ids=BASE_IDS)
def test_conditioner_into_a_sought_ring_equals_the_control(gpu, base, boundary, name):
    from gnss_sdr_amd import GshError, SignalConditioner
    raw, kw, capacity = _cond_case(name)
    rt, rc, b0 = _pair(gpu, capacity, COND_WIN, base)
    cap = _kept(capacity)
    conds = [SignalConditioner(r, device=gpu, **kw) for r in (rt, rc)]
    try:
        pos = produced = n_push_boundary = wrapped_inside = 0
        for b in COND_BLOCKS:
            first_t, n_t = conds[0].push(raw[pos:pos + b])
            first_c, n_c = conds[1].push(raw[pos:pos + b])
            pos += b
            assert (first_t, n_t) == (base + produced, n_c) and first_c == b0 + produced, (name, b)
            n_push_boundary += _inside(first_t, n_t, boundary)
            produced += n_t
            assert rt.range() == (max(base, base + produced - cap), base + produced)
            assert conds[0].position() == conds[1].position() == (pos, produced)
            if n_t:
                assert np.array_equal(_bits(rt.read(first_t, n_t)), _bits(rc.read(first_c, n_t))), (name, b)
                wrapped_inside += first_c // cap != (first_c + n_t - 1) // cap
        assert produced > 700 and wrapped_inside >= 1
        if name == "blanked":
            assert conds[0].blanking_state() == conds[1].blanking_state() and conds[0].blanking_state()["n_blanked"] > 0
        if name == "notched":
            assert conds[0].notch_state() == conds[1].notch_state() and conds[0].notch_state()["n_filtered"] > 0
        lo, hi = rt.range()
        whole = rt.read(lo, hi - lo)
        assert np.array_equal(_bits(whole), _bits(rc.read(lo - base + b0, hi - lo))) and np.any(whole != 0)
        if boundary is not None:
            assert n_push_boundary == 1
        # the ring is sought by someone else: the conditioner's next output no longer goes to the ring's next index
        rt.seek(base + produced + 10)
        with pytest.raises(GshError) as e:
            conds[0].push(raw[:100])
        assert e.value.code == 4, str(e.value)
        assert conds[0].position() == (pos, produced) and rt.range() == (base + produced + 10, base + produced + 10)
        conds[0].bind(rt)
        first, _n = conds[0].push(raw[:100])
        assert first == base + produced + 10
    finally:
        for c in conds:
            c.close()
        rt.close()
        rc.close()


BEAM_CAPS, BEAM_WINS = (1007, 640, 4096), (100, 64, 512)
BEAM_PUSHES = [500, 137, 640, 1, 333, 600, 64, 639, 480, 512, 555, 421]      # those of tests/test_beamformer_gpu.py: none above the smallest capacity


@pytest.mark.parametrize("base,boundary", _bases(512), ids=BASE_IDS)
def test_beamformer_into_three_sought_rings_equals_the_control(gpu, base, boundary):
    import beamformer_reference as R
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    A = B = 3
    total = sum(BEAM_PUSHES)
    x = np.random.default_rng(23).integers(-32768, 32768, (A, total, 2)).astype(np.int16)
    caps = [_kept(c) for c in BEAM_CAPS]
    b0s = [base % c for c in caps]
    rings = [SampleStream(c, m, device=gpu) for c, m in zip(BEAM_CAPS, BEAM_WINS)]
    twins = [SampleStream(c, m, device=gpu) for c, m in zip(BEAM_CAPS, BEAM_WINS)]
    bfs = [Beamformer(ArrayFormat(A, "ishort", "interleaved", True), B, device=gpu) for _ in range(2)]
    try:
        for r in range(B):
            rings[r].seek(base)
            twins[r].seek(b0s[r])
        for bf in bfs:
            bf.set_weights(R.case_weights(B, A, seed=1))
        done = n_push_boundary = 0
        for k, n in enumerate(BEAM_PUSHES):
            blk = np.ascontiguousarray(x[:, done:done + n].transpose(1, 0, 2))
            inverted = bool(k % 3 == 2)
            first_t = bfs[0].push(rings, blk, inverted)
            first_c = bfs[1].push(twins, blk, inverted)
            n_push_boundary += _inside(base + done, n, boundary)
            for r in range(B):
                assert first_t[r] == base + done and first_c[r] == b0s[r] + done, (k, r)
                hi = done + n
                lo = max(0, hi - caps[r])
                assert rings[r].range() == (base + lo, base + hi) and twins[r].range() == (b0s[r] + lo, b0s[r] + hi), (k, r)
                got = rings[r].read(base + lo, hi - lo)
                assert np.array_equal(_bits(got), _bits(twins[r].read(b0s[r] + lo, hi - lo))) and np.any(got != 0), (k, r)
            done += n
        assert done > max(caps)
        if boundary is not None:
            assert n_push_boundary == 1
    finally:
        for bf in bfs:
            bf.close()
        for s in rings + twins:
            s.close()


@pytest.mark.parametrize("base,boundary", _bases(N), ids=BASE_IDS)
def test_generator_into_a_sought_ring_equals_the_model_at_the_base(gpu, base, boundary):
    """gen.seek(B), gen.push(ring, n): the ring indices are B + produced; the carrier phase legitimately depends on the absolute index, so the content is
    held to the exact model at B under the bar of tests/test_siggen_gpu.py (K 2^-24 sum amplitude), not to the control"""
    import siggen_reference as R
    from gnss_sdr_amd import SignalGenerator
    from gnss_sdr_amd.sample_stream import SampleStream
    from test_siggen_gpu import K, U
    from test_siggen_reference import built_satellites
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "siggen.npz")) as z:
        sats = built_satellites(dict(z), "gps", scaled=True)
    ring = SampleStream(BANK_CAP, BANK_WIN, device=gpu)
    gen = SignalGenerator(4e6, len(sats), device=gpu)
    try:
        for i, s in enumerate(sats):
            gen.set_satellite(i, s)
        ring.seek(base)
        gen.seek(base)
        produced = n_push_boundary = 0
        bar = K * U * R.amplitude_sum(sats)
        worst = 0.0
        for n in (N + 1, 2 * N, 3 * N + 17, 1, 3 * N):          # 36 019 samples: the last push wraps the ring
            first = gen.push(ring, n)
            assert first == base + produced and gen.position() == base + produced + n
            n_push_boundary += _inside(first, n, boundary)
            produced += n
            lo, hi = ring.range()
            assert (lo, hi) == (max(base, base + produced - _kept(BANK_CAP)), base + produced)
            got = ring.read(first, n)
            err = np.abs(got.astype(np.complex128) - R.model(sats, 4e6, first, n))
            worst = max(worst, float(err.max()))
            assert np.all(err <= bar), (n, float(err.max()), bar)
        print(f"generator at {base}: worst |gpu - model| = {worst:.3e}, bar {bar:.3e}")
        assert produced > _kept(BANK_CAP)
        if boundary is not None:
            assert n_push_boundary == 1
    finally:
        gen.close()
        ring.close()
