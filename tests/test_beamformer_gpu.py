"""GPU tests of the antenna-array front end (gsh_beam_*, csrc/beamformer.hip; gnss_sdr_amd.array): the beam kernel against the numpy restatement of the
reference's beamformer block (tests/beamformer_reference.py, pinned to the block's own output by tests/test_beamformer_reference.py), the one-push-B-rings
entry points against plain pushes of the host-computed beams, the consumers of such rings, the FP64 covariance, and the reason the feature exists: a jammed
satellite that one antenna does not acquire and the power-inversion beam does.  Comparisons of beams and rings are bit for bit."""
import functools
import os

import numpy as np
import pytest

import beamformer_reference as R
import oracle
from helpers import tracking_params_for

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beamformer.npz")
GUARD = 16                       # complex samples of sentinel in front of and behind every output
SENTINEL = np.float32(-77.25)
NP_ITEM = R.ITEM_DTYPES


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", gpu)


@functools.lru_cache(maxsize=None)
def _items(item_type, A):
    x = R.case_items(item_type, A)
    x.setflags(write=False)
    return x


def _seen(item_type, A, layout, lead):
    """[A, n_max, 2]: the items antenna a contributes to samples 0.. when every input pointer is advanced by `lead` items.  Planar: antenna a's own
    stream from item `lead`; interleaved: the frames of the sample-major buffer read from item `lead` on."""
    x = _items(item_type, A)
    n_max = R.N_MAX - 1
    if layout == "planar":
        return x[:, lead:lead + n_max]
    flat = np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(-1, 2)       # item k * A + a
    return flat[lead:lead + n_max * A].reshape(n_max, A, 2).transpose(1, 0, 2)


def _expect(item_type, A, B, layout, lead, first_is_q, inverted):
    re, im = R.items_to_complex(_seen(item_type, A, layout, lead), bool(first_is_q), bool(inverted))
    return R.beamform(re, im, R.case_weights(B, A))


def _upload(torch_dev, item_type, A, layout):
    """the case's items on the device -> (tensor kept alive, pointers of the buffers, bytes per item)"""
    torch, dev = torch_dev
    x = _items(item_type, A)
    isz = x.dtype.itemsize * 2
    if layout == "planar":
        t = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(A, -1).copy()).to(dev)
        return t, [t.data_ptr() + a * t.shape[1] for a in range(A)], isz
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2)).view(np.uint8).reshape(-1).copy()).to(dev)
    return t, [t.data_ptr()], isz


# ---- 1. process_device against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("item_type", ["gr_complex", "ishort", "ibyte"])
def test_process_device_equals_the_restatement_bit_for_bit(gpu, torch_dev, item_type, layout):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    torch, dev = torch_dev
    n_max = R.N_MAX - 1
    cases = 0
    for A in (1, 2, 3, 8):
        keep, ptrs, isz = _upload(torch_dev, item_type, A, layout)
        assert all(p % 16 == 0 for p in ptrs) or layout == "planar"
        for B in (1, 3, 8):
            out = torch.empty((B, 2 * (n_max + 2 * GUARD)), dtype=torch.float32, device=dev)
            for first_is_q in (0, 1):
                bf = Beamformer(ArrayFormat(A, item_type, layout, bool(first_is_q)), B, device=gpu)
                w = R.case_weights(B, A)
                bf.set_weights(w)
                assert np.array_equal(_bits(bf.weights), _bits(w))
                for inverted in (0, 1):
                    for lead in (0, 1):            # 1: every input pointer advanced by one item -- no 16-byte load is possible
                        exp = _expect(item_type, A, B, layout, lead, first_is_q, inverted)
                        for n in (1, 63, 64, 65, 1000, 4099):
                            out.fill_(float(SENTINEL))
                            torch.cuda.synchronize()     # the handle works on a stream of its own
                            bf.process_device([p + lead * isz for p in ptrs], n, [out[b].data_ptr() + 8 * GUARD for b in range(B)], bool(inverted))
                            h = out.cpu().numpy()
                            got = h[:, 2 * GUARD:2 * (GUARD + n)]
                            what = (A, B, first_is_q, inverted, lead, n)
                            assert np.array_equal(_bits(got), _bits(exp[:, :n]).reshape(B, -1)), what
                            assert np.all(h[:, :2 * GUARD] == SENTINEL) and np.all(h[:, 2 * (GUARD + n):] == SENTINEL), what
                            cases += 1
                bf.close()
        del keep
    assert cases == 4 * 3 * 2 * 2 * 2 * 6


def test_default_weights_on_the_golden_inputs_equal_the_reference_block(gpu, torch_dev):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    torch, dev = torch_dev
    with np.load(GOLDEN) as z:
        x, y = z["x"], z["y"]
    n = x.shape[1]
    d_x = torch.from_numpy(x).to(dev)
    d_il = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(dev)
    out = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    for layout, ptrs in (("planar", [d_x[a].data_ptr() for a in range(8)]), ("interleaved", [d_il.data_ptr()])):
        bf = Beamformer(ArrayFormat(8, "gr_complex", layout), 1, device=gpu)
        assert np.array_equal(bf.weights, np.ones((1, 8), np.complex64))          # beamformer.h:52
        out.zero_()
        torch.cuda.synchronize()
        bf.process_device(ptrs, n, [out.data_ptr()])
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(y).reshape(-1)), layout
        bf.close()


# ---- 2. rings ------------------------------------------------------------------------------------------------------------------------------------
CAPS, WINS = (1007, 640, 4096), (100, 64, 512)
PUSHES = [500, 137, 640, 1, 333, 600, 64, 639, 480, 512, 555, 421]      # uneven, none above the smallest capacity; 4 882 samples in all


def _array_block(item_type, A, n, seed):
    rng = np.random.default_rng(seed)
    if item_type == "gr_complex":
        return rng.standard_normal((A, n, 2)).astype(np.float32)
    info = np.iinfo(NP_ITEM[item_type])
    return rng.integers(info.min, info.max + 1, (A, n, 2)).astype(NP_ITEM[item_type])


def _host_form(x, layout):
    """[A, n, 2] items as the push takes them"""
    return [np.ascontiguousarray(a) for a in x] if layout == "planar" else np.ascontiguousarray(x.transpose(1, 0, 2))


@pytest.mark.parametrize("item_type,layout,first_is_q", [("ishort", "interleaved", 1), ("gr_complex", "planar", 0), ("ibyte", "planar", 1)])
def test_one_push_fills_three_rings_like_plain_pushes_of_the_host_beams(gpu, torch_dev, item_type, layout, first_is_q):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking import CorrelatorBank
    torch, dev = torch_dev
    A = B = 3
    total = sum(PUSHES)
    x = _array_block(item_type, A, total, 23)
    w1, w2 = R.case_weights(B, A, seed=1), R.case_weights(B, A, seed=2)
    rings = [SampleStream(c, m, device=gpu) for c, m in zip(CAPS, WINS)]
    twins = [SampleStream(c, m, device=gpu) for c, m in zip(CAPS, WINS)]
    rings[1].seek(38)
    twins[1].seek(38)
    seeks = (0, 38, 0)
    caps = [c + (c & 1) for c in CAPS]
    bf = Beamformer(ArrayFormat(A, item_type, layout, bool(first_is_q)), B, device=gpu)
    bf.set_weights(w1)
    banks = []
    for r in range(B):
        pair = [CorrelatorBank(1, 1023, device=gpu) for _ in range(2)]
        for k, ring in zip(pair, (rings[r], twins[r])):
            k.set_code(0, oracle.ca_code(r + 1))
            k.set_stream_ring(ring)
        banks.append(pair)
    params = tracking_params_for(4e6, 1000.0, np.random.default_rng(1))
    isz = x.dtype.itemsize * 2
    done, wrap_push, mirrored = 0, [None] * B, 0
    try:
        for k, n in enumerate(PUSHES):
            if k == 4:
                bf.set_weights(w2)                                           # from this push's first sample on
            w = w1 if k < 4 else w2
            inverted = bool(k % 3 == 2)
            blk = x[:, done:done + n]
            re, im = R.items_to_complex(blk, bool(first_is_q), inverted)
            beams = R.beamform(re, im, w)
            if k == 4:                                                       # the weight change is visible in the data
                other = R.beamform(re, im, w1)
                assert all(beams[r, 0] != other[r, 0] for r in range(B))
            if k & 1:                                                        # every other block is already on the device
                host = _host_form(blk, layout)
                d = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(-1)).to(dev) for h in (host if layout == "planar" else [host])]
                first = bf.push_device(rings, [t.data_ptr() for t in d], n, inverted)
            else:
                first = bf.push(rings, _host_form(blk, layout), inverted)
            for r in range(B):
                assert twins[r].push(beams[r]) == first[r] == seeks[r] + done
                hi = seeks[r] + done + n
                lo = max(seeks[r], hi - caps[r])
                assert rings[r].range() == (lo, hi) == twins[r].range(), (k, r)
                assert np.array_equal(_bits(rings[r].read(lo, hi - lo)), _bits(twins[r].read(lo, hi - lo))), (k, r)
                if hi // caps[r] and wrap_push[r] is None:
                    wrap_push[r] = k
                # a window that starts just below the capacity boundary and runs out of the ring's end into the mirror
                edge = hi // caps[r] * caps[r]
                off, nw = edge - WINS[r] // 3, WINS[r] - 1
                if edge > 0 and off >= lo and off + nw <= hi:
                    job = [dict(sample_offset=off, n_samples=nw, code_slot=0, shifts_chips=[-0.5, 0.0, 0.5], **params)]
                    got, want = banks[r][0].correlate(job), banks[r][1].correlate(job)
                    assert np.array_equal(_bits(got), _bits(want)) and np.any(want != 0), (k, r, off)
                    mirrored += 1
            done += n
        assert None not in wrap_push and len(set(wrap_push)) == B, wrap_push    # each ring wraps at a different push
        assert mirrored >= 3, mirrored
    finally:
        for pair in banks:
            for k in pair:
                k.close()
        bf.close()
        for s in rings + twins:
            s.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_pushes_leave_every_ring_untouched(gpu):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    from test_tracking_live_gpu import KW, N, _drain, _loop, _scenario
    prns, dops, starts, total, x8, xf = _scenario(20, seed=9)
    A = B = 3
    rings = [SampleStream(c, 2 * N, device=gpu) for c in (12 * N, 13 * N + 1, 14 * N)]
    bf = Beamformer(ArrayFormat(A, "ibyte", "planar"), B, device=gpu)
    bf.set_weights(np.eye(3, dtype=np.complex64))
    noise = np.random.default_rng(3).integers(-3, 4, (2, total, 2)).astype(np.int8)
    ant = [x8, noise[0], noise[1]]
    live = _loop(gpu, dict(KW, enable_lock_detectors=0), n_channels=1)
    try:
        live.set_stream_ring(rings[0])
        live.start(0, oracle.ca_code(prns[0]), starts[0], 0, dops[0] + 6.0)
        live.live_configure(idle_timeout_us=100000, residency_us=1000000)
        assert bf.push(rings, [a[:8 * N] for a in ant]) == [0, 0, 0]
        before = [r.range() for r in rings]
        held = [r.read(lo, hi - lo) for r, (lo, hi) in zip(rings, before)]
        live.live_begin()
        got, lost = [[]], [False]
        _drain(live, got, lost, 2.0, want=[6])
        assert len(got[0]) >= 6
        refused = [
            ("a ring named twice", [rings[0], rings[1], rings[0]], 64, 1),
            ("n above the smallest capacity", rings, 12 * N + 2, 1),
            # the channel stands below 8 N; the first ring holds 12 N: a push of 12 N more would overwrite its next window
            ("a ring that a live tracking channel still reads", rings, 12 * N, 4),
        ]
        for what, rr, n, code in refused:
            with pytest.raises(GshError) as e:
                bf.push(rr, [np.zeros((n, 2), np.int8)] * 3)
            assert e.value.code == code, (what, str(e.value))
            assert [r.range() for r in rings] == before, what
        with pytest.raises(GshError) as e:
            bf.push_device([rings[1], rings[1], rings[2]], [0, 0, 0], 0)
        assert e.value.code == 1
        assert [r.range() for r in rings] == before
        live.live_quiesce()
        for r, b, h in zip(rings, before, held):
            assert np.array_equal(_bits(r.read(b[0], b[1] - b[0])), _bits(h))
        # and the rings still take the next block where they stood
        assert bf.push(rings, [a[8 * N:9 * N] for a in ant]) == [8 * N] * 3
    finally:
        live.close()
        bf.close()
        for r in rings:
            r.close()


# ---- 4. consumers see the push -------------------------------------------------------------------------------------------------------------------
def test_correlator_bank_on_a_beam_ring_equals_the_twin_ring(gpu):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking import CorrelatorBank
    A, B, n = 4, 2, 6000
    x = _array_block("ishort", A, n, 31)
    w = R.case_weights(B, A, seed=5)
    re, im = R.items_to_complex(x)
    beams = R.beamform(re, im, w)
    rings = [SampleStream(8192, 2048, device=gpu) for _ in range(B)]
    twins = [SampleStream(8192, 2048, device=gpu) for _ in range(B)]
    bf = Beamformer(ArrayFormat(A, "ishort", "interleaved"), B, device=gpu)
    bf.set_weights(w)
    banks = [CorrelatorBank(1, 1023, device=gpu) for _ in range(2 * B)]
    try:
        assert bf.push(rings, _host_form(x, "interleaved")) == [0, 0]
        rng = np.random.default_rng(2)
        params = tracking_params_for(4e6, -1500.0, rng)
        jobs = [dict(sample_offset=k * 500 + (k % 3), n_samples=2046 - k, code_slot=0, shifts_chips=[-0.5, 0.0, 0.5], **params) for k in range(8)]
        for r in range(B):
            assert twins[r].push(beams[r]) == 0
            for bank, ring in ((banks[2 * r], rings[r]), (banks[2 * r + 1], twins[r])):
                bank.set_code(0, oracle.ca_code(r + 3))
                bank.set_stream_ring(ring)
            got, want = banks[2 * r].correlate(jobs), banks[2 * r + 1].correlate(jobs)
            assert np.array_equal(_bits(got), _bits(want)) and np.any(want != 0), r
    finally:
        for b in banks:
            b.close()
        bf.close()
        for s in rings + twins:
            s.close()


def test_live_tracking_loop_follows_a_beam_ring(gpu):
    """GPS L1, 2.046 Msps, 120 periods (the scenario shape of tests/test_tracking_live_gpu.py): the loop's records over a ring that beam pushes fill must
    equal, byte for byte, those of a launched run over the flat restated beam.  A residency that does not learn of a push idles out by itself: this
    fails by count, it cannot hang."""
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    from test_tracking_live_gpu import KW, N, _bytes, _drain, _flat_run, _loop, _scenario
    epochs = 120
    prns, dops, starts, total, x8, xf = _scenario(epochs, seed=5)
    other = np.random.default_rng(6).integers(-4, 5, (total, 2)).astype(np.int8)
    ant = np.stack([x8, other])
    w = np.array([[1.0, 0.25 - 0.125j], [0.0, 1.0]], np.complex64)
    re, im = R.items_to_complex(ant)
    flat = R.beamform(re, im, w)
    rec_flat, done_flat = _flat_run(gpu, prns, dops, starts, flat[0], epochs)
    assert done_flat[0] >= epochs - 2 and done_flat[1] >= epochs - 2, done_flat
    rings = [SampleStream(40 * N, 2 * N, device=gpu), SampleStream(11 * N + 1, 2 * N, device=gpu)]
    bf = Beamformer(ArrayFormat(2, "ibyte", "planar"), 2, device=gpu)
    bf.set_weights(w)
    live = _loop(gpu, KW, n_channels=3)
    try:
        live.set_stream_ring(rings[0])
        for ch in range(3):
            live.start(ch, oracle.ca_code(prns[ch]), starts[ch], 0, dops[ch] + 6.0)
        got, lost = [[], [], []], [False, False, False]
        pushed, pushes = 0, 0
        blk = total // 12 + 17
        while pushed < total:
            m = min(blk, total - pushed)
            assert bf.push(rings, [ant[0, pushed:pushed + m], ant[1, pushed:pushed + m]]) == [pushed, pushed]
            pushed += m
            pushes += 1
            if live.live_in_flight() == 0:
                live.live_begin()
            want = [min(done_flat[ch], max(0, (pushed - starts[ch]) // N - 1)) for ch in range(3)]
            _drain(live, got, lost, 2.0, want)
        assert pushes == 12
        _drain(live, got, lost, 1.0)
        live.live_quiesce()
        _drain(live, got, lost, 0.2)
        for ch in range(3):
            assert len(got[ch]) >= done_flat[ch], (ch, len(got[ch]), done_flat[ch])
            assert _bytes(got[ch][:done_flat[ch]]) == _bytes(rec_flat[ch][:done_flat[ch]]), f"channel {ch}: live records over the beam ring differ from the launched run"
        lo, hi = rings[1].range()
        assert np.array_equal(_bits(rings[1].read(lo, hi - lo)), _bits(flat[1][lo:hi]))
    finally:
        live.close()
        bf.close()
        for r in rings:
            r.close()


# ---- 5. covariance -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 100003])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_covariance(gpu, torch_dev, A, n):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    torch, dev = torch_dev
    for k, item_type in enumerate(("ibyte", "ishort", "gr_complex")):
        layout = ("planar", "interleaved")[(k + A) & 1]
        first_is_q, inverted = bool(k & 1), bool((k + n) & 1)
        x = _array_block(item_type, A, n, 100 * A + k)
        re, im = R.items_to_complex(x, first_is_q, inverted)
        X = re.astype(np.float64) + 1j * im.astype(np.float64)
        want = X @ X.conj().T
        bf = Beamformer(ArrayFormat(A, item_type, layout, first_is_q), 1, device=gpu)
        host = _host_form(x, layout)
        got = bf.covariance(host, inverted)
        d = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(-1)).to(dev) for h in (host if layout == "planar" else [host])]
        got_d = bf.covariance_device([t.data_ptr() for t in d], n, inverted)
        again = bf.covariance_device([t.data_ptr() for t in d], n, inverted)
        bf.close()
        what = (A, n, item_type, layout)
        assert got.tobytes() == got_d.tobytes() == again.tobytes(), what          # the same data, the same bits
        assert np.array_equal(got, got.conj().T), what                            # exactly Hermitian
        if item_type != "gr_complex":
            assert np.abs(want).max() < 2.0 ** 53
            assert np.array_equal(got, want), what                                # every term and sum is an exact integer
        else:
            mag = np.abs(X)
            bound = 2.0 * n * 2.0 ** -53 * (mag @ mag.T)                          # first order, any summation order of exactly formed products
            err = np.abs(got - want)
            print(f"covariance A={A} n={n}: worst |dR| / bound = {np.max(err / bound):.3g}")
            assert np.all(err <= bound), what


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_power_inversion_beam_acquires_the_jammed_satellite(gpu, torch_dev):
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank, compute_threshold
    from gnss_sdr_amd.array import ArrayFormat, Beamformer, power_inversion_weights
    from gnss_sdr_amd.sample_stream import SampleStream
    torch, dev = torch_dev
    s = R.E2E
    x = R.e2e_block()
    n, A = s["n"], s["n_antennas"]
    d_x = torch.from_numpy(x).to(dev)
    ptrs = [d_x[a].data_ptr() for a in range(A)]
    bf = Beamformer(ArrayFormat(A, "gr_complex", "planar"), 2, device=gpu)
    rings = [SampleStream(8192, n, device=gpu) for _ in range(2)]
    acq = PcpsAcquisitionBank(max_prn=1, device=gpu, **R.E2E_ACQ)
    try:
        Rm = bf.covariance_device(ptrs, n)
        w = power_inversion_weights(Rm)
        bf.set_weights(np.stack([w, np.eye(A, dtype=np.complex64)[0]]))            # the beam, and antenna 0 as it is
        assert bf.push_device(rings, ptrs, n) == [0, 0]
        acq.set_local_code(0, oracle.ca_code_complex_sampled(s["prn"], s["fs"]))
        beam = acq.dwell_ring(rings[0], 0, 1)[0]
        ant0 = acq.dwell_ring(rings[1], 0, 1)[0]
        thr = compute_threshold(R.E2E_PFA, 4000, 40, 1)
        print(f"antenna 0 statistic {ant0['test_statistics']:.2f}, beam {beam['test_statistics']:.1f} at ({beam['index_time']}, {beam['doppler_hz']} Hz), "
              f"threshold {thr:.2f}")
        assert ant0["test_statistics"] < thr
        assert beam["test_statistics"] > 2.0 * thr
        assert (beam["index_time"], beam["doppler_hz"]) == (2826, 1250)
    finally:
        acq.close()
        bf.close()
        for r in rings:
            r.close()


# ---- 7. rate -------------------------------------------------------------------------------------------------------------------------------------
def test_beam_kernel_rate(gpu, gsh):
    import ctypes as C
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    n = 1 << 20
    bf = Beamformer(ArrayFormat(8, "cbyte", "interleaved"), 8, device=gpu)
    try:
        ms = bf.time_process(n, reps=20)
    finally:
        bf.close()
    probe = C.c_double(0.0)
    assert gsh.gsh_probe_read_bandwidth(gpu, 1 << 28, 10, C.byref(probe)) == 0
    gbs = (16 + 64) * n / (ms * 1e-3) / 1e9
    print(f"beam kernel, A = 8, B = 8, cbyte interleaved, n = 2^20: {ms:.4f} ms per block, {gbs:.0f} GB/s over (16 + 64) n bytes, "
          f"{gbs / probe.value:.2f} of the read probe's {probe.value:.0f} GB/s")
    assert ms > 0.0
