"""GPU tests of the beamformer's adaptive mode (gsh_adaptive_beam_set, csrc/beamformer.hip + csrc/array_weights.h; gnss_sdr_amd.array): every comparison is
bit for bit.  What a call must leave is predicted from gsh_beam_covariance_device of the block, taken by a second, non-adaptive handle, run through the
host build of the header (tests/aw_host.py); the beams must be those of a fixed-weight handle set to exactly the predicted weights."""
import ctypes as C

import numpy as np
import pytest

import aw_host
import beamformer_reference as R
import oracle

pytestmark = pytest.mark.gpu

NP_ITEM = R.ITEM_DTYPES


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", gpu)


def _array_block(item_type, A, n, seed):
    rng = np.random.default_rng(seed)
    if item_type == "gr_complex":
        return rng.standard_normal((A, n, 2)).astype(np.float32)
    info = np.iinfo(NP_ITEM[item_type])
    return rng.integers(info.min, info.max + 1, (A, n, 2)).astype(NP_ITEM[item_type])


def _host_form(x, layout):
    """[A, n, 2] items as the push takes them"""
    return [np.ascontiguousarray(a) for a in x] if layout == "planar" else np.ascontiguousarray(x.transpose(1, 0, 2))


def _to_device(torch_dev, x, layout):
    """[A, n, 2] items on the device -> (tensors kept alive, pointers of the buffers)"""
    torch, dev = torch_dev
    host = _host_form(x, layout)
    d = [torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(-1)).to(dev) for h in (host if layout == "planar" else [host])]
    return d, [t.data_ptr() for t in d]


def _constraints(kind, B, A, seed):
    """(keyword arguments of set_adaptive, the constraint vectors [B, A])"""
    if kind == "reference":
        ref = [(seed + b) % A for b in range(B)]
        return dict(reference=ref), np.eye(A, dtype=np.complex128)[ref]
    s = np.exp(2j * np.pi * np.random.default_rng(seed).random((B, A)))
    return dict(steering=s), s


# ---- 1. the chain against the prediction -------------------------------------------------------------------------------------------------------
# per (item type, layout): A in {1, 3, 8} x beams in {1, 8} x lambda in {0, 0.9}, twelve settings over which first_is_q, the inverted spectrum and the
# kind of constraint (steering / reference) rotate; three consecutive blocks per setting, the four sizes dealt over the settings (131073 > 512 x 256:
# the covariance grid strides; 255 / 257: either side of a tile; 1: a rank-one covariance, which only the loading makes solvable)
SIZES = ([255, 1, 257], [131073, 257, 1], [257, 131073, 255], [1, 255, 131073], [131073, 1, 255], [257, 255, 1])


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
@pytest.mark.parametrize("item_type", ["gr_complex", "ishort", "ibyte"])
def test_chain_equals_the_prediction_bit_for_bit(gpu, torch_dev, item_type, layout):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    torch, dev = torch_dev
    calls, seen_sizes, seen_flags = 0, set(), set()
    for setting, (A, B, lam) in enumerate((A, B, lam) for A in (1, 3, 8) for B in (1, 8) for lam in (0.0, 0.9)):
        flip = (setting >> 2) & 1
        first_is_q, inverted = bool(setting & 1), bool((setting >> 1) & 1) ^ bool(flip)
        sizes = SIZES[setting % len(SIZES)]
        seen_sizes.update(sizes)
        seen_flags.add((first_is_q, inverted, flip))
        x = _array_block(item_type, A, sum(sizes), 1000 * A + setting)
        keep, base = _to_device(torch_dev, x, layout)
        isz = x.dtype.itemsize * 2 * (1 if layout == "planar" else A)
        fmt = ArrayFormat(A, item_type, layout, first_is_q)
        bf, ref = Beamformer(fmt, B, device=gpu), Beamformer(fmt, B, device=gpu)
        fixed = R.case_weights(B, A, seed=7)
        bf.set_weights(fixed)
        kw, c = _constraints(("steering", "reference")[flip], B, A, seed=A + setting)
        # no loading where the first block is rank one (A > 1, n = 1): whether rounding lets such a call through or fails it is the prediction's to say
        loading = 0.0 if (A > 1 and sizes[0] == 1) else 1e-6
        bf.set_adaptive(forgetting=lam, loading_rel=loading, **kw)
        host = aw_host.HostAdaptive(A, B, c, fixed, forgetting=lam, loading_rel=loading)
        assert aw_host.same_state(bf.adaptive_state(), host.state())          # before any call: R_acc = 0, the caller's weights
        out = torch.empty((2, B, 2 * max(sizes)), dtype=torch.float32, device=dev)
        try:
            start = 0
            for n in sizes:
                ptrs = [p + start * isz for p in base]
                out.fill_(-77.25)
                torch.cuda.synchronize()                                      # the handles work on streams of their own
                bf.process_device(ptrs, n, [out[0, b].data_ptr() for b in range(B)], inverted)
                host.step(ref.covariance_device(ptrs, n, inverted))
                got, want = bf.adaptive_state(), host.state()
                what = (A, B, lam, first_is_q, inverted, n)
                assert aw_host.same_state(got, want), (what, got, want)
                assert np.array_equal(bf.weights, fixed)                      # gsh_beam_get_weights: still the caller's
                ref.set_weights(want["weights"])
                ref.process_device(ptrs, n, [out[1, b].data_ptr() for b in range(B)], inverted)
                assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)), what
                assert bool(torch.all(out[0, :, 2 * n:] == -77.25)) and not bool(torch.any(out[0, :, :2 * n] == -77.25)), what
                calls += 1
                start += n
            assert want["blocks"] == 3
        finally:
            bf.close()
            ref.close()
        del keep
    assert calls == 36 and seen_sizes == {1, 255, 257, 131073}
    assert {f[0] for f in seen_flags} == {f[1] for f in seen_flags} == {False, True} and {f[2] for f in seen_flags} == {0, 1}


# ---- 2. pushes against plain pushes of the host-computed beams -----------------------------------------------------------------------------------
CAPS, WINS = (1007, 640, 4096), (100, 64, 512)
PUSHES = [500, 137, 640, 1, 333, 600]                       # the 640-sample ring wraps at the second push, the 1007-sample ring at the third


@pytest.mark.parametrize("item_type,layout,first_is_q", [("ishort", "interleaved", 1), ("gr_complex", "planar", 0)])
def test_adaptive_pushes_fill_three_rings_like_plain_pushes(gpu, torch_dev, item_type, layout, first_is_q):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    A = B = 3
    x = _array_block(item_type, A, sum(PUSHES), 23)
    fmt = ArrayFormat(A, item_type, layout, bool(first_is_q))
    bf, ref = Beamformer(fmt, B, device=gpu), Beamformer(fmt, B, device=gpu)
    fixed = R.case_weights(B, A, seed=1)
    bf.set_weights(fixed)
    kw, c = _constraints("steering", B, A, seed=4)
    bf.set_adaptive(forgetting=0.9, loading_rel=1e-6, **kw)
    host = aw_host.HostAdaptive(A, B, c, fixed, forgetting=0.9, loading_rel=1e-6)
    rings = [SampleStream(cap, m, device=gpu) for cap, m in zip(CAPS, WINS)]
    twins = [SampleStream(cap, m, device=gpu) for cap, m in zip(CAPS, WINS)]
    fixed_rings = [SampleStream(cap, m, device=gpu) for cap, m in zip(CAPS, WINS)]
    for group in (rings, twins, fixed_rings):
        group[1].seek(38)
    wrapped = set()
    done = 0
    try:
        for k, n in enumerate(PUSHES):
            inverted = bool(k % 3 == 2)
            blk = x[:, done:done + n]
            if k & 1:                                                             # every other block is already on the device
                keep, ptrs = _to_device(torch_dev, blk, layout)
                first = bf.push_device(rings, ptrs, n, inverted)
                first_fixed = ref.push_device(fixed_rings, ptrs, n, inverted)
            else:
                first = bf.push(rings, _host_form(blk, layout), inverted)
                first_fixed = ref.push(fixed_rings, _host_form(blk, layout), inverted)
            host.step(ref.covariance(_host_form(blk, layout), inverted))
            got, want = bf.adaptive_state(), host.state()
            assert aw_host.same_state(got, want), (k, got, want)
            assert want["failures"] == 0
            re, im = R.items_to_complex(blk, bool(first_is_q), inverted)
            beams = R.beamform(re, im, want["weights"])
            assert first == first_fixed
            for r in range(B):
                assert twins[r].push(beams[r]) == first[r]
                lo, hi = rings[r].range()
                assert (lo, hi) == twins[r].range() == fixed_rings[r].range(), (k, r)
                assert np.array_equal(_bits(rings[r].read(lo, hi - lo)), _bits(twins[r].read(lo, hi - lo))), (k, r)
                if lo > (38 if r == 1 else 0):
                    wrapped.add(r)
            done += n
        assert wrapped == {0, 1}                                                  # two rings wrapped, the large one did not
    finally:
        bf.close()
        ref.close()
        for s in rings + twins + fixed_rings:
            s.close()


# ---- 3. no host synchronisation between two adaptive pushes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", ["one stream", "two streams"])
def test_back_to_back_pushes_need_no_host_synchronisation(gpu, torch_dev, streams):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    torch, dev = torch_dev
    A, B, n = 4, 2, 100000
    x = _array_block("ishort", A, 2 * n, 77)
    fmt = ArrayFormat(A, "ishort", "interleaved")
    bf, ref = Beamformer(fmt, B, device=gpu), Beamformer(fmt, B, device=gpu)
    kw, c = _constraints("reference", B, A, seed=1)
    bf.set_adaptive(forgetting=0.9, loading_rel=1e-6, **kw)
    host = aw_host.HostAdaptive(A, B, c, np.ones((B, A), np.complex64), forgetting=0.9, loading_rel=1e-6)
    rings = [SampleStream(3 * n, 1024, device=gpu) for _ in range(B)]
    keep0, p0 = _to_device(torch_dev, x[:, :n], "interleaved")
    keep1, p1 = _to_device(torch_dev, x[:, n:], "interleaved")
    s0 = torch.cuda.Stream(device=dev)
    s1 = s0 if streams == "one stream" else torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    try:
        first0 = bf.push_device(rings, p0, n, False, hip_stream=s0.cuda_stream)   # both queued before anything is waited for
        first1 = bf.push_device(rings, p1, n, True, hip_stream=s1.cuda_stream)
        assert (first0, first1) == ([0, 0], [n, n])
        s0.synchronize()
        s1.synchronize()
        weights = []
        for ptrs, inverted in ((p0, False), (p1, True)):
            host.step(ref.covariance_device(ptrs, n, inverted))
            weights.append(host.state()["weights"])
        got, want = bf.adaptive_state(), host.state()
        assert aw_host.same_state(got, want), (got, want)
        assert want["blocks"] == 2 and want["failures"] == 0
        for k, (blk, inverted) in enumerate(((x[:, :n], False), (x[:, n:], True))):
            re, im = R.items_to_complex(blk, False, inverted)
            beams = R.beamform(re, im, weights[k])
            for r in range(B):
                assert np.array_equal(_bits(rings[r].read(k * n, n)), _bits(beams[r])), (k, r)
    finally:
        bf.close()
        ref.close()
        for s in rings:
            s.close()
    del keep0, keep1


# ---- 4. the failure path ---------------------------------------------------------------------------------------------------------------------------
def test_a_block_that_cannot_be_solved_keeps_the_callers_weights(gpu, torch_dev):
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    A, B, n = 3, 2, 300
    fmt = ArrayFormat(A, "ishort", "planar")
    bf, ref = Beamformer(fmt, B, device=gpu), Beamformer(fmt, B, device=gpu)
    fixed = R.case_weights(B, A, seed=3)
    bf.set_weights(fixed)
    kw, c = _constraints("steering", B, A, seed=2)
    bf.set_adaptive(**kw)                                                         # no forgetting, no loading
    host = aw_host.HostAdaptive(A, B, c, fixed)
    rings = [SampleStream(1024, 64, device=gpu) for _ in range(B)]
    try:
        zeros = np.zeros((A, n, 2), np.int16)
        assert bf.push(rings, _host_form(zeros, "planar")) == [0, 0]
        assert not host.step(ref.covariance(_host_form(zeros, "planar")))
        st = bf.adaptive_state()
        assert aw_host.same_state(st, host.state())
        assert (st["blocks"], st["failures"]) == (1, 1) and st["weights"].tobytes() == fixed.tobytes()
        for r in range(B):                                                        # the fixed-weight beam of an all-zero block: zeros, and no NaN
            got = rings[r].read(0, n)
            assert not np.any(np.isnan(got.view(np.float32))) and np.all(got == 0)
        x = _array_block("ishort", A, n, 5)
        assert bf.push(rings, _host_form(x, "planar")) == [n, n]
        assert host.step(ref.covariance(_host_form(x, "planar")))
        st = bf.adaptive_state()
        assert aw_host.same_state(st, host.state())
        assert (st["blocks"], st["failures"]) == (2, 1) and st["weights"].tobytes() != fixed.tobytes()
        re, im = R.items_to_complex(x)
        beams = R.beamform(re, im, st["weights"])
        for r in range(B):
            assert np.array_equal(_bits(rings[r].read(n, n)), _bits(beams[r])), r
    finally:
        bf.close()
        ref.close()
        for s in rings:
            s.close()


# ---- 5. the state survives refusals and timing; the mode goes and comes back ---------------------------------------------------------------------
def test_state_survives_refusals_and_timing_and_the_mode_switches_at_call_boundaries(gpu, torch_dev):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    A, B, n = 3, 2, 400
    fmt = ArrayFormat(A, "ibyte", "planar")
    bf, ref = Beamformer(fmt, B, device=gpu), Beamformer(fmt, B, device=gpu)
    fixed = R.case_weights(B, A, seed=9)
    bf.set_weights(fixed)
    kw, c = _constraints("reference", B, A, seed=0)
    conf = dict(forgetting=0.5, loading_rel=1e-6, loading_abs=0.25)
    bf.set_adaptive(**conf, **kw)
    host = aw_host.HostAdaptive(A, B, c, fixed, **conf)
    rings = [SampleStream(1000, 64, device=gpu) for _ in range(B)]
    x = _array_block("ibyte", A, 4 * n, 13)
    blocks = [_host_form(x[:, k * n:(k + 1) * n], "planar") for k in range(4)]

    def beams_of(k, w):
        re, im = R.items_to_complex(x[:, k * n:(k + 1) * n])
        return R.beamform(re, im, w)

    try:
        assert bf.push(rings, blocks[0]) == [0, 0]
        host.step(ref.covariance(blocks[0]))
        before = bf.adaptive_state()
        assert aw_host.same_state(before, host.state()) and before["blocks"] == 1
        held = [r.read(0, n) for r in rings]
        for what, rr, m in (("a ring named twice", [rings[0], rings[0]], 64), ("n above a ring's capacity", rings, 1001)):
            with pytest.raises(GshError) as e:
                bf.push(rr, [np.zeros((m, 2), np.int8)] * A)
            assert e.value.code == 1, (what, str(e.value))
            assert aw_host.same_state(bf.adaptive_state(), before), what
            assert [r.range() for r in rings] == [(0, n)] * B, what
        assert bf.time_process(5000, reps=3) > 0.0                                # the whole chain, on copies of the state
        assert aw_host.same_state(bf.adaptive_state(), before)
        assert np.array_equal(ref.covariance(blocks[1]), bf.covariance(blocks[1]))  # the covariance call of an adaptive handle: as ever, R_acc left alone
        assert aw_host.same_state(bf.adaptive_state(), before)
        for r in range(B):
            assert np.array_equal(_bits(rings[r].read(0, n)), _bits(held[r]))
        # the mode cleared: the caller's weights from the next call's first sample on
        bf.set_adaptive(None)
        with pytest.raises(GshError) as e:
            bf.adaptive_state()
        assert e.value.code == 4                                                  # GSH_ERR_STATE
        assert bf.push(rings, blocks[1]) == [n, n]
        for r, beam in enumerate(beams_of(1, fixed)):
            assert np.array_equal(_bits(rings[r].read(n, n)), _bits(beam)), r
        # the mode set again: from R_acc = 0 and zero counters, whatever the earlier state was
        bf.set_adaptive(**conf, **kw)
        host = aw_host.HostAdaptive(A, B, c, fixed, **conf)
        assert aw_host.same_state(bf.adaptive_state(), host.state())
        assert bf.push(rings, blocks[2]) == [2 * n, 2 * n]
        host.step(ref.covariance(blocks[2]))
        st = bf.adaptive_state()
        assert aw_host.same_state(st, host.state()) and st["blocks"] == 1
        assert np.array_equal(st["r_acc"], ref.covariance(blocks[2]))
        for r, beam in enumerate(beams_of(2, st["weights"])):
            assert np.array_equal(_bits(rings[r].read(2 * n, n)), _bits(beam)), r
    finally:
        bf.close()
        ref.close()
        for s in rings:
            s.close()


def test_invalid_configurations_on_a_handle(gpu, gsh):
    """the refusals of tests/test_beam_adaptive_abi.py on a real handle, and the one that needs a handle: an all-zero constraint vector of a beam it forms"""
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from test_beam_adaptive_abi import GSH_ERR_INVALID, _bad_numbers, _conf
    zero = np.zeros((8, 8), np.complex128)
    zero[:, 0] = 1.0
    zero[1, :4] = 0.0
    zero[1, 4] = 1.0                                 # beam 1 of 2: nothing on the 4 antennas of the array
    b = Beamformer(ArrayFormat(4), 2, device=gpu)
    try:
        for conf, word in _bad_numbers() + [(_conf(c=zero), "all zero")]:
            assert gsh.gsh_adaptive_beam_set(b._h, C.byref(conf)) == GSH_ERR_INVALID, word
            assert word.encode() in gsh.gsh_last_error(), (word, gsh.gsh_last_error())
        from gnss_sdr_amd import GshError
        with pytest.raises(GshError) as e:
            b.adaptive_state()                       # none of them switched the mode on
        assert e.value.code == 4
        unused = np.zeros((8, 8), np.complex128)
        unused[:2, 3] = 1.0                          # beams the handle does not form may be all zero
        assert gsh.gsh_adaptive_beam_set(b._h, C.byref(_conf(c=unused))) == 0
        assert b.adaptive_state()["blocks"] == 0
    finally:
        b.close()


# ---- 6. end to end: the jammed satellite of tests/test_beamformer_gpu.py, without the host in the loop ------------------------------------------
def test_end_to_end_one_adaptive_push_acquires_the_jammed_satellite(gpu, torch_dev):
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank, compute_threshold
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    from gnss_sdr_amd.sample_stream import SampleStream
    torch, dev = torch_dev
    s = R.E2E
    x = R.e2e_block()
    n, A = s["n"], s["n_antennas"]
    d_x = torch.from_numpy(x).to(dev)
    ptrs = [d_x[a].data_ptr() for a in range(A)]
    fmt = ArrayFormat(A, "gr_complex", "planar")
    bf, plain = Beamformer(fmt, 1, device=gpu), Beamformer(fmt, 1, device=gpu)
    rings = [SampleStream(8192, n, device=gpu) for _ in range(2)]
    acq = PcpsAcquisitionBank(max_prn=1, device=gpu, **R.E2E_ACQ)
    try:
        torch.cuda.synchronize()
        bf.set_adaptive(reference=0)                                               # power inversion on the block itself
        assert bf.push_device([rings[0]], ptrs, n) == [0]                          # covariance, solve and beam in the one call
        plain.set_weights(np.eye(A, dtype=np.complex64)[0])                        # antenna 0 as it is
        assert plain.push_device([rings[1]], ptrs, n) == [0]
        st = bf.adaptive_state()
        assert (st["blocks"], st["failures"]) == (1, 0) and st["weights"][0, 0] == 1.0
        acq.set_local_code(0, oracle.ca_code_complex_sampled(s["prn"], s["fs"]))
        beam = acq.dwell_ring(rings[0], 0, 1)[0]
        ant0 = acq.dwell_ring(rings[1], 0, 1)[0]
        thr = compute_threshold(R.E2E_PFA, 4000, 40, 1)
        print(f"antenna 0 statistic {ant0['test_statistics']:.2f}, adaptive beam {beam['test_statistics']:.1f} at ({beam['index_time']}, "
              f"{beam['doppler_hz']} Hz), threshold {thr:.2f}")
        assert ant0["test_statistics"] < thr
        assert beam["test_statistics"] > 2.0 * thr
        assert (beam["index_time"], beam["doppler_hz"]) == (2826, 1250)
    finally:
        acq.close()
        bf.close()
        plain.close()
        for r in rings:
            r.close()
