"""GPU tests of the notch filters as a stage of the signal conditioner's push (gsh_cond_set_notch).

The yardstick, BIT FOR BIT (array_equal on the uint32 views, no tolerance anywhere): the loose chain in one call per stage over the whole stream,
gsh_convert_samples_device / gsh_unpack_device -> gsh_fir_process_device -> ONE gsh_notch_process_device over all M filter outputs ->
gsh_direct_resample_device, and gsh_notch_get_state of that one call.  The counters are those of NotchOracle / NotchLiteOracle walked over the
device FIR's own outputs; the same walk shows, per case, that the input takes the branches that can go wrong (several engagements, a re-entry into
estimation after a reset, filtered runs over several chunks; or one filtered run across nearly the whole stream).

Streams: interfered_stream of tests/test_notch_oracle_pinned.py (unit-variance noise, three continuous-wave interferers), about 12 289 filter outputs.
Every case runs under five cut patterns (CUTS below) with the three push flavours in rotation; the ring holds 4 096 samples and is bound near its
end, so every run wraps; no push completes more outputs than the ring holds; the ring is read back as it goes.
"""
import ctypes as C
import mmap

import numpy as np
import pytest

from oracle.notch_oracle import NotchLiteOracle, NotchOracle
from test_notch_oracle_pinned import interfered_stream

pytestmark = pytest.mark.gpu

CAPACITY = 4096
WINDOW = 512
BASE = CAPACITY - 301   # samples already in the ring when the conditioner is bound: every run wraps early
CHUNK = 128             # NF_CHUNK
M_TOTAL = 12289         # filter outputs per case
SEED = 11
# (start, length, amplitude, cycles per sample) at the filter's output rate; the cases with a filter place them inside its passband
CW = ((1500, 1500, 6.0, 0.071), (5000, 2500, 3.0, -0.19), (9000, 800, 10.0, 0.33))


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _taps(case):
    """a windowed-sinc low-pass with its cutoff at 1 / (2 width D) cycles per input sample"""
    K, D, width = case["K"], case["D"], case.get("width", 2.5)
    t = (np.hamming(K) * np.sinc((np.arange(K) - (K - 1) / 2) / (width * D))).astype(np.float32)
    return t / t.sum()


def _two_bit_cpx():
    from gnss_sdr_amd.sample_stream import PackedFormat
    return PackedFormat.from_signal_source("Two_Bit_Cpx_File_Signal_Source")


def _cw(freqs, D=1):
    """CW's interferers at D times the rate, with these input frequencies"""
    return tuple((s * D, w * D, a, f) for (s, w, a, _f), f in zip(CW, freqs))


CASES = {
    "1 gr_complex Notch L32": dict(kind="gr_complex", cw=CW, notch=dict(length=32, segments_est=40, segments_reset=100, pfa=0.001, p_c_factor=0.9)),
    # conjugated, then translated by -0.15 cycles per sample, cutoff 0.1: the interferers land at -0.02, 0.05, -0.06
    "2 ibyte inverted xlating K33 D2 decimating Notch L100": dict(kind="ibyte", inv=True, K=33, D=2, fc=1.2e6, fs=8e6, rs=(4e6, 2.5e6), cw=_cw((-0.13, -0.2, -0.09), 2),
                                                                  notch=dict(length=100, segments_est=10, segments_reset=30, pfa=0.01, p_c_factor=0.8)),
    "3 ishort K33 D1 interpolating NotchLite L16": dict(kind="ishort", K=33, D=1, fc=0.0, fs=4e6, rs=(4e6, 4.092e6), cw=_cw((0.071, -0.15, 0.12)),
                                                        notch=dict(length=16, segments_coeff=1, segments_est=40, segments_reset=200, pfa=0.01, p_c_factor=0.85)),
    # a half-band filter (cutoff at the output's Nyquist rate) and pfa 1e-5: behind the narrower filter of the other cases, or with pfa 0.001, the
    # energy test of this length fires on every segment of the two-bit noise and the filter never disengages (seen with the oracle on the CPU)
    "4 two-bit packed K33 D2 NotchLite L64": dict(kind="two_bit_cpx", K=33, D=2, width=1.0, fc=0.0, fs=8e6, cw=_cw((0.03, -0.07, 0.05), 2),
                                                  notch=dict(length=64, segments_coeff=3, segments_est=20, segments_reset=60, pfa=1e-5)),
    "5 gr_complex Notch L2": dict(kind="gr_complex", cw=CW, notch=dict(length=2, segments_est=200, segments_reset=2000, pfa=0.01)),
    "6 gr_complex Notch L1024": dict(kind="gr_complex", cw=CW, notch=dict(length=1024, segments_est=2, p_c_factor=0.95)),
}
LONG_RUN = ("2", "6")   # the cases that must show one filtered run of more than 10 000 samples; the others engagements, a re-entry, runs over chunks


def _notch(case):
    from gnss_sdr_amd.conditioner import NOTCH_DEFAULTS
    return dict(NOTCH_DEFAULTS, **case["notch"])


def _n_in(case):
    """input samples that give M_TOTAL filter outputs (a whole number of bytes for the packed case)"""
    D = case.get("D", 1)
    return M_TOTAL * D if case["kind"] == "two_bit_cpx" else (M_TOTAL - 1) * D + 1


def _raw(case):
    """(the raw array sliced by units, samples per unit, the decoded samples as the adapter yields them)"""
    x = interfered_stream(_n_in(case), seed=SEED, cw=case["cw"])
    kind = case["kind"]
    if kind == "gr_complex":
        return x, 1, x
    if kind in ("ibyte", "ishort"):
        scale, top, dt = (4.0, 127, np.int8) if kind == "ibyte" else (100.0, 32767, np.int16)
        raw = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -top, top).astype(dt)
        dec = (raw[:, 0].astype(np.float32) + 1j * raw[:, 1].astype(np.float32)).astype(np.complex64)
        return raw, 1, np.conj(dec) if case.get("inv") else dec
    # Two_Bit_Cpx: values +-1 below two sigma, +-3 above; field = ((v - 1) / 2) & 3, sample 0 = (bits 7:6, bits 5:4), sample 1 = (bits 3:2, bits 1:0)
    q = lambda v: np.where(np.abs(v) < 2.0, 1, 3) * np.where(v < 0, -1, 1)
    vi, vq = q(x.real), q(x.imag)
    f = lambda v: ((v - 1) // 2) & 3
    raw = ((f(vi[0::2]) << 6) | (f(vq[0::2]) << 4) | (f(vi[1::2]) << 2) | f(vq[1::2])).astype(np.uint8)
    return raw, 2, (vi + 1j * vq).astype(np.complex64)


def _chain_kw(case):
    kw = dict(input_kind=_two_bit_cpx() if case["kind"] == "two_bit_cpx" else case["kind"], inverted_spectrum=case.get("inv", False))
    if "K" in case:
        kw.update(taps=_taps(case), decimation=case["D"], center_freq_hz=case["fc"], sampling_freq_hz=case["fs"])
    if "rs" in case:
        kw.update(fs_in=case["rs"][0], fs_out=case["rs"][1])
    return kw


def _loose_filter_outputs(gpu, torch, case, raw, per_unit):
    """adapter and filter of the loose chain, one call each over the whole stream (tests/test_conditioner_gpu.py::_loose_chain with this file's taps)"""
    from gnss_sdr_amd.sample_stream import FirFilter, convert_samples_device, unpack_device
    dev = torch.device("cuda", gpu)
    n = len(raw) * per_unit
    d_raw = torch.from_numpy(raw).to(dev)
    d_x = torch.zeros(n, dtype=torch.complex64, device=dev)
    if case["kind"] == "two_bit_cpx":
        unpack_device(gpu, _two_bit_cpx(), d_raw.data_ptr(), 0, n, d_x.data_ptr(), inverted_spectrum=case.get("inv", False))
    else:
        convert_samples_device(gpu, d_raw.data_ptr(), case["kind"], d_x.data_ptr(), n, inverted_spectrum=case.get("inv", False))
    torch.cuda.synchronize()
    if "K" not in case:
        return d_x.cpu().numpy()
    D = case["D"]
    d_y = torch.zeros(n // D + 2, dtype=torch.complex64, device=dev)
    f = FirFilter(_taps(case), D, case["fc"], case["fs"], "gr_complex", device=gpu)
    n_f = f.process_device(d_x.data_ptr(), n, d_y.data_ptr(), d_y.numel())
    f.close()
    torch.cuda.synchronize()
    assert n_f == (n + D - 1) // D
    return d_y.cpu().numpy()[:n_f].copy()


_PLANS = {}


def _plan(case, n_in):
    from gnss_sdr_amd.conditioner import outputs_after
    key = (id(case), n_in)
    if key not in _PLANS:
        _PLANS[key] = outputs_after(n_in, notch=case["notch"], **_chain_kw(case))
    return _PLANS[key]


def walk_oracle(case, y):
    """NotchOracle / NotchLiteOracle over the filter outputs y, one segment per call (L + 1 items offered): (w, modes, the oracle, figures)"""
    n = _notch(case)
    L = n["length"]
    kw = dict(pfa=n["pfa"], p_c_factor=n["p_c_factor"], length=L, n_segments_est=n["segments_est"], n_segments_reset=n["segments_reset"])
    orc = NotchLiteOracle(n_segments_coeff=n["segments_coeff"], **kw) if n["segments_coeff"] else NotchOracle(**kw)
    n_seg = (len(y) - 1) // L
    out, resets, reentries, pending = [], 0, 0, False
    for s in range(n_seg):
        before = orc.n_segments
        w, done = orc.general_work(y[s * L:(s + 1) * L + 1])
        assert done == L
        out.append(w)
        if orc.n_segments == 1 and before > 0:
            resets += 1
            pending = True
        if orc.modes[-1] == 0 and pending:      # an estimating segment after a reset of the counter
            reentries += 1
            pending = False
    modes = np.array(orc.modes, np.uint8)
    assert len(modes) == n_seg
    filt = modes == 1
    engagements = int(np.sum(filt & ~np.concatenate([[False], filt[:-1]])))
    run = longest = 0
    for f in filt:
        run = run + 1 if f else 0
        longest = max(longest, run)
    fig = dict(segments=n_seg, filtered=int(filt.sum()), engagements=engagements, resets=resets, reentries=reentries, longest_run=longest * L)
    return np.concatenate(out), modes, orc, fig


def check_coverage(name, fig):
    if name[0] in LONG_RUN:
        assert fig["longest_run"] > 10000, (name, fig)
    else:
        assert fig["engagements"] >= 3 and fig["reentries"] >= 1 and fig["longest_run"] > 3 * CHUNK, (name, fig)


_EXPECTED = {}


def _expected(gpu, torch, name):
    """computed once per case and shared, read-only: dict(case, raw, per_unit, y: the filter outputs, w: the loose notch's outputs, exp: the loose
    chain's ring content, state: gsh_notch_get_state of the one call + the threshold, w_o / modes / fig: the oracle walk over y)"""
    if name in _EXPECTED:
        return _EXPECTED[name]
    from gnss_sdr_amd.sample_stream import NotchFilter, direct_resample_device
    case = CASES[name]
    n = _notch(case)
    L = n["length"]
    raw, per_unit, _dec = _raw(case)
    n_in = len(raw) * per_unit
    assert n_in == _n_in(case)
    dev = torch.device("cuda", gpu)
    y = _loose_filter_outputs(gpu, torch, case, raw, per_unit)
    M = len(y)
    assert M == M_TOTAL
    W = L * ((M - 1) // L)
    # the loose notch over the whole stream in one call
    d_y = torch.from_numpy(y).to(dev)
    d_w = torch.zeros(M, dtype=torch.complex64, device=dev)
    torch.cuda.synchronize()
    nf = NotchFilter(n["pfa"], n["p_c_factor"], L, n["segments_est"], n["segments_reset"], n["segments_coeff"], device=gpu)
    assert nf.process_device(d_y.data_ptr(), M, d_w.data_ptr()) == W
    state = dict(nf.state(), thres=np.float32(nf.threshold))
    nf.close()
    w = d_w.cpu().numpy()[:W].copy()
    if "rs" in case:
        fs_in, fs_out = case["rs"]
        d_r = torch.zeros(int(W * fs_out / fs_in) + 8, dtype=torch.complex64, device=dev)
        n_r, _cons = direct_resample_device(gpu, d_w.data_ptr(), 0, W, fs_in, fs_out, 0, d_r.data_ptr(), d_r.numel())
        torch.cuda.synchronize()
        exp = d_r.cpu().numpy()[:n_r].copy()
    else:
        exp = w
    assert len(exp) == _plan(case, n_in), (name, len(exp), _plan(case, n_in))
    w_o, modes, orc, fig = walk_oracle(case, y)
    print(name, fig)
    check_coverage(name, fig)
    for a in (y, w, exp, w_o, modes):
        a.setflags(write=False)
    _EXPECTED[name] = dict(case=case, raw=raw, per_unit=per_unit, y=y, w=w, exp=exp, state=state, w_o=w_o, modes=modes, fig=fig, orc=orc)
    return _EXPECTED[name]


# ---- cut patterns: ascending totals of filter outputs at which the pushes end, the last one M_TOTAL

def _most(case):
    """filter outputs a push may add so that it completes at most CAPACITY ring samples (whole segments of them: up to L - 1 more than it adds)"""
    ratio = max(1.0, case["rs"][1] / case["rs"][0]) if "rs" in case else 1.0
    return int((CAPACITY - 8) / ratio) - _notch(case)["length"]


def _fill(ends, case, at=0):
    """`ends` (ascending filter-output totals above `at`) completed to M_TOTAL, steps larger than the ring allows split"""
    most, out = _most(case), []
    for e in list(ends) + [M_TOTAL]:
        while e - at > most:
            at += most
            out.append(at)
        if e > at:
            out.append(e)
            at = e
    return out


def _cuts_large(case):
    return _fill([], case)


def _cuts_segment_edges(case):
    """every push ends at M = 0, 1, 2 (mod L): one before, at, and one after the sample that completes a segment"""
    L = _notch(case)["length"]
    sizes = (1, 2, max(1, 300 // L), max(1, 1100 // L))   # segments per push, in rotation
    ends, seg, k = [], 0, 0
    while True:
        seg += sizes[k % 4]
        e = seg * L + k % 3
        if e >= M_TOTAL:
            break
        ends.append(e)
        k += 1
    assert {e % L for e in ends} >= {0, 1, 2 % L}
    return _fill(ends, case)


def _cuts_chunk_edges(case):
    """pushes that end with a segment boundary inside a chunk (M - 1 a multiple of L, not of 128), and one before, on and one after a chunk boundary"""
    L = _notch(case)["length"]
    ends, at, k = [], 0, 0
    strides = (1, 140, 700, 1500)
    kinds = set()
    while True:
        lo = at + strides[k % 4]
        if k % 2 == 0 and L % CHUNK != 0:
            s = -(-lo // L)
            while (s * L) % CHUNK == 0:
                s += 1
            e = s * L + 1                      # W' becomes s L: inside chunk floor(s L / 128)
            kinds.add("segment")
        else:
            d = (k // 2) % 3 - 1
            e = -(-lo // CHUNK) * CHUNK + 1 + d    # M - 1 = 128 c + d
            kinds.add(d)
        if e >= M_TOTAL:
            break
        if e > at:
            ends.append(e)
            at = e
        k += 1
    assert kinds >= {-1, 0, 1} and ("segment" in kinds or L % CHUNK == 0)
    return _fill(ends, case)


def _cuts_tiny(case):
    """one large push, a stretch of more than two segments that _blocks feeds in pushes of 1 - 3 input samples, then large pushes: (the stretch's
    first and last filter-output total, the totals after it)"""
    L = _notch(case)["length"]
    start = 1000 + CHUNK - 1000 % CHUNK - 7    # a few outputs before a chunk boundary
    stop = start + 2 * L + 9
    return start, stop, _fill([], case, at=stop)


def _cuts_random(case):
    L = _notch(case)["length"]
    rng = np.random.default_rng(SEED + 77 + L)
    ends, at = [], 0
    while at < M_TOTAL:
        kind = int(rng.integers(0, 4))
        at += 1 if kind == 0 else int(rng.integers(1, 2 * L + 2)) if kind == 1 else int(rng.integers(1, CHUNK + 2)) if kind == 2 else int(rng.integers(1, 3000))
        if at < M_TOTAL:
            ends.append(at)
    return _fill(ends, case)


CUTS = {"a large": _cuts_large, "b segment edges": _cuts_segment_edges, "c chunk edges": _cuts_chunk_edges, "d tiny": _cuts_tiny, "e random": _cuts_random}


def _blocks(case, pattern, n_units, per_unit):
    """block sizes in units of the raw array"""
    D = case.get("D", 1)

    def units_for(M):
        """the fewest units whose samples give M filter outputs"""
        for n_in in range((M - 1) * D + 1, M * D + 1):
            if n_in % per_unit == 0:
                return n_in // per_unit
        raise AssertionError((M, D, per_unit))

    ends = CUTS[pattern](case)
    if pattern != "d tiny":
        totals = [units_for(M) for M in ends]
    else:
        start, stop, rest = ends
        rng = np.random.default_rng(SEED + 5)
        totals = [units_for(start)]
        while totals[-1] < units_for(stop):
            totals.append(min(units_for(stop), totals[-1] + -(-int(rng.integers(1, 4)) // per_unit)))   # 1 - 3 input samples (a packed byte holds two)
        totals += [units_for(M) for M in rest]
    assert totals[-1] <= n_units and n_units - totals[-1] < D
    totals[-1] = n_units
    assert all(b > a for a, b in zip(totals, totals[1:])), pattern
    return [b - a for a, b in zip([0] + totals, totals)]


def _run(gpu, gsh, torch, name, pattern):
    """-> the last ring samples of the run; everything else is asserted here"""
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    e = _expected(gpu, torch, name)
    case, raw, per_unit, exp, state, modes = e["case"], e["raw"], e["per_unit"], e["exp"], e["state"], e["modes"]
    n_units = len(raw)
    blocks = _blocks(case, pattern, n_units, per_unit)
    assert sum(blocks) == n_units and min(blocks) >= 1
    ring = SampleStream(CAPACITY, WINDOW, device=gpu)
    assert ring.push(np.full(BASE, 3 - 4j, np.complex64)) == 0
    cond = SignalConditioner(ring, device=gpu, notch=case["notch"], **_chain_kw(case))
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
        pos, wraps, zero_pushes, flavours, j1 = 0, 0, 0, set(), 0
        for i, b in enumerate(blocks):
            j0, j1 = _plan(case, pos * per_unit), _plan(case, (pos + b) * per_unit)
            assert j1 - j0 <= CAPACITY, (name, pattern, i, b)
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
            assert (first, n_out) == (BASE + j0, j1 - j0), (name, pattern, i, first, n_out, j0, j1)
            assert cond.position() == (pos * per_unit, j1), (name, pattern, i)
            zero_pushes += n_out == 0
            if n_out:
                got = ring.read(first, n_out)
                assert np.array_equal(_bits(got), _bits(exp[j0:j1])), (name, pattern, i, j0, int(np.argmax(got != exp[j0:j1])))
                wraps += first // CAPACITY != (first + n_out - 1) // CAPACITY
        assert pos == n_units and j1 == len(exp)
        assert wraps >= 1 and flavours == {0, 1, 2}, (name, pattern, wraps)
        if pattern == "d tiny":
            assert zero_pushes >= max(1, _notch(case)["length"] // 2), (name, zero_pushes)   # pushes that complete nothing
        st = cond.notch_state()
        assert st["noise_pow_est"].view(np.uint32) == np.float32(state["noise_pow_est"]).view(np.uint32), (name, pattern, st, state)
        assert (st["n_segments"], st["filter_state"], st["n_segments_coeff"]) == (state["n_segments"], state["filter_state"], state["n_segments_coeff"]), (name, pattern, st, state)
        assert st["thres"].view(np.uint32) == state["thres"].view(np.uint32)
        lite = _notch(case)["segments_coeff"] > 0
        z0 = np.complex64(state["z0"]) if lite else np.complex64(0)
        assert np.array_equal(_bits([st["z0"]]), _bits([z0])), (name, pattern, st, state)
        assert (st["n_decided"], st["n_filtered"]) == (len(modes), int((modes == 1).sum())), (name, pattern, st, e["fig"])
        lo, hi = ring.range()
        lo = max(lo, BASE)
        tail = ring.read(lo, hi - lo)
        assert np.array_equal(_bits(tail), _bits(exp[lo - BASE:hi - BASE]))
        return tail
    finally:
        cond.close()
        assert gsh.gsh_host_unregister(C.c_void_p(pinned.ctypes.data)) == 0
        ring.close()


@pytest.mark.parametrize("name", list(CASES))
def test_ring_equals_the_loose_chain_whatever_the_cuts(gpu, gsh, name):
    import torch
    tails = [_run(gpu, gsh, torch, name, pattern) for pattern in CUTS]
    for t in tails[1:]:
        assert np.array_equal(_bits(tails[0]), _bits(t))
    e = _expected(gpu, torch, name)
    assert np.any(e["exp"] != 0) and len(e["modes"]) == (M_TOTAL - 1) // _notch(e["case"])["length"]


@pytest.mark.parametrize("name", ["1 gr_complex Notch L32", "3 ishort K33 D1 interpolating NotchLite L16"])
def test_ring_against_the_oracle(gpu, gsh, name):
    """the bars of tests/test_notch_filter_gpu.py: passed segments bit-identical, filtered segments within 1e-4 of the segment's amplitude, decisions
    identical up to a first differing segment, which must lie beyond 98 % of the segments.  The oracle is fed the device FIR's own outputs."""
    import torch
    import test_conditioner_gpu as plain
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    e = _expected(gpu, torch, name)
    case, raw, per_unit, w_o, modes = e["case"], e["raw"], e["per_unit"], e["w_o"], e["modes"]
    L = _notch(case)["length"]
    ring = SampleStream(CAPACITY, WINDOW, device=gpu)
    cond = SignalConditioner(ring, device=gpu, notch=case["notch"], **_chain_kw(case))
    try:
        got, pos = [], 0
        for b in _blocks(case, "e random", len(raw), per_unit):
            first, n_out = cond.push(raw[pos:pos + b], b * per_unit)
            pos += b
            if n_out:
                got.append(ring.read(first, n_out))
        got = np.concatenate(got)
    finally:
        cond.close()
        ring.close()
    # ring sample j is w[m(j)]
    m = np.array([plain._filter_index(case, j) for j in range(len(got))], np.int64)
    assert m[-1] < len(w_o) and (m[-1] == len(w_o) - 1 or "rs" in case)
    seg = m // L
    n_seg = len(modes)
    scale = np.maximum(np.abs(w_o.reshape(n_seg, L)).max(axis=1), 1e-6)
    err = np.zeros(n_seg)
    np.maximum.at(err, seg, np.abs(got - w_o[m]))
    err /= scale
    bad = np.nonzero(err > 1e-4)[0]
    first_bad = int(bad[0]) if len(bad) else n_seg
    assert first_bad >= 0.98 * n_seg, (name, first_bad, n_seg, err[bad[:4]] if len(bad) else None)
    ok = (seg < first_bad) & (modes[seg] != 1)
    assert ok.sum() > 1000 and np.array_equal(_bits(got[ok]), _bits(w_o[m[ok]]))     # passed segments: bit for bit
    assert ((seg < first_bad) & (modes[seg] == 1)).sum() > 1000


def test_refusals_move_nothing(gpu, gsh):
    """notch after the first push, notch with blanking on and the reverse, a push beyond the ring's capacity, a moved ring index: after each refusal
    the ring, the position and the state are as they were, and the stream continues bit for bit"""
    import torch
    from gnss_sdr_amd import GshError, SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "2 ibyte inverted xlating K33 D2 decimating Notch L100"
    e = _expected(gpu, torch, name)
    case, raw, exp, state, modes = e["case"], e["raw"], e["exp"], e["state"], e["modes"]
    plan = lambda n: _plan(case, n)
    ring = SampleStream(1201, WINDOW, device=gpu)
    cond = SignalConditioner(ring, device=gpu, notch=case["notch"], **_chain_kw(case))

    def unchanged(pos, done, extra=0):
        assert cond.position() == (pos, done) and ring.range() == (0, done + extra)
        return cond.notch_state()

    try:
        assert cond.push(raw[:1503]) == (0, plan(1503))
        done = plan(1503)
        assert done > 0
        held, st0 = ring.read(0, done), cond.notch_state()
        assert st0["n_decided"] == (752 - 1) // 100
        for attempt in (lambda: cond.set_notch(dict(length=7)), lambda: cond.set_notch(None), lambda: cond.set_blanking(dict(length=7)), lambda: cond.set_blanking(None)):
            with pytest.raises(GshError) as err:
                attempt()
            assert err.value.code == 4
        assert unchanged(1503, done) == st0
        assert plan(6503) - done > 1202
        with pytest.raises(GshError) as err:
            cond.push(raw[1503:6503])
        assert err.value.code == 1 and "capacity" in str(err.value)
        assert unchanged(1503, done) == st0 and np.array_equal(_bits(ring.read(0, done)), _bits(held))
        first, n_out = cond.push(raw[1503:2704])
        assert (first, n_out) == (done, plan(2704) - done) and n_out > 0
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        done += n_out
        st1 = cond.notch_state()
        assert ring.push(np.zeros(10, np.complex64)) == done
        with pytest.raises(GshError) as err:
            cond.push(raw[2704:3500])
        assert err.value.code == 4 and "someone else" in str(err.value)
        with pytest.raises(GshError) as err:
            cond.push_pinned_async(raw[2704:3500])
        assert err.value.code == 4
        assert unchanged(2704, done, 10) == st1
        cond.bind(ring)
        first, n_out = cond.push(raw[2704:3501])
        assert (first, n_out) == (done + 10, plan(3501) - done) and n_out > 0
        assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
        done += n_out
        pos = 3501
        while pos < len(raw):
            b = min(1500, len(raw) - pos)
            first, n_out = cond.push(raw[pos:pos + b])
            pos += b
            assert (first, n_out) == (done + 10, plan(pos) - done)
            assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
            done += n_out
        assert done == len(exp)
        st = cond.notch_state()
        assert (float(st["noise_pow_est"]), st["n_segments"], st["filter_state"]) == (state["noise_pow_est"], state["n_segments"], state["filter_state"])
        assert (st["n_decided"], st["n_filtered"]) == (len(modes), int((modes == 1).sum()))
    finally:
        cond.close()
        ring.close()
    # one mitigation stage per handle, either order; bad values are refused before anything is allocated and leave a handle that still works
    cond = SignalConditioner(None, device=gpu)
    try:
        cond.set_blanking(dict(length=8))
        with pytest.raises(GshError) as err:
            cond.set_notch(dict(length=8))
        assert err.value.code == 4 and "blanking" in str(err.value)
        assert cond.blanking_state()["n_decided"] == 0
        cond.set_blanking(None)
        cond.set_notch(dict(length=8))
        with pytest.raises(GshError) as err:
            cond.set_blanking(dict(length=8))
        assert err.value.code == 4 and "notch" in str(err.value)
        assert cond.notch_state()["n_decided"] == 0
        cond.set_notch(None)
        for bad in (dict(pfa=0.0), dict(length=1), dict(length=1025), dict(segments_est=-1), dict(segments_reset=-1), dict(segments_coeff=-1), dict(p_c_factor=float("nan"))):
            with pytest.raises(GshError) as err:
                cond.set_notch(bad)
            assert err.value.code == 1
        with pytest.raises(GshError) as err:
            cond.notch_state()
        assert err.value.code == 4
    finally:
        cond.close()
    with pytest.raises(GshError) as err:
        SignalConditioner(None, device=gpu, blanking=dict(length=8), notch=dict(length=8))
    assert err.value.code == 4


def test_time_push_leaves_everything_alone(gpu):
    import torch
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.sample_stream import SampleStream
    name = "3 ishort K33 D1 interpolating NotchLite L16"
    e = _expected(gpu, torch, name)
    case, raw, exp, state = e["case"], e["raw"], e["exp"], e["state"]
    plan = lambda n: _plan(case, n)
    ring = SampleStream(CAPACITY, WINDOW, device=gpu)
    cond = SignalConditioner(ring, device=gpu, notch=case["notch"], **_chain_kw(case))
    d_raw = torch.from_numpy(raw).to(torch.device("cuda", gpu))
    torch.cuda.synchronize()
    try:
        first, done = cond.push(raw[:2151])          # inside a filtered stretch: an open chunk with carried modes, a carry and a history
        held, st0 = ring.read(0, done), cond.notch_state()
        assert st0["n_decided"] == 2150 // 16 and st0["filter_state"]
        ms = cond.time_push(d_raw.data_ptr() + 4 * 2151, 3000, reps=3)
        assert ms > 0.0
        assert cond.position() == (2151, done) and ring.range() == (0, done)
        assert np.array_equal(_bits(ring.read(0, done)), _bits(held))
        assert cond.notch_state() == st0
        pos = 2151
        while pos < len(raw):
            b = min(3500, len(raw) - pos)
            first, n_out = cond.push(raw[pos:pos + b])
            pos += b
            assert (first, n_out) == (done, plan(pos) - done)
            assert np.array_equal(_bits(ring.read(first, n_out)), _bits(exp[done:done + n_out]))
            done += n_out
        st = cond.notch_state()
        assert (float(st["noise_pow_est"]), st["n_segments"], st["filter_state"], st["n_segments_coeff"]) == (state["noise_pow_est"], state["n_segments"],
                                                                                                            state["filter_state"], state["n_segments_coeff"])
    finally:
        cond.close()
        ring.close()


@pytest.mark.parametrize("name", ["3 ibyte inverted K33 D2 xlating decimating", "6 packed four-bit complex K33 D2"])
def test_a_handle_with_the_stage_turned_off_gives_the_plain_rings(gpu, gsh, name):
    """set_notch(...) then set_notch(NULL) before the first push: the rings of the plain conditioner (tests/test_conditioner_gpu.py's table)"""
    import torch
    import test_conditioner_gpu as plain
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.sample_stream import SampleStream
    case, raw, per_unit, exp = plain._expected(gpu, torch, name)
    ring = SampleStream(3001, WINDOW, device=gpu)
    cond = plain._conditioner(gpu, ring, case)
    try:
        cond.set_notch(dict(length=5, segments_est=2, segments_reset=3))
        cond.set_notch(None)
        with pytest.raises(GshError):
            cond.notch_state()
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
