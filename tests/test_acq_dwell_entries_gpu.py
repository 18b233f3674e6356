"""The dwell entries of the acquisition handle held to EACH OTHER (the oracle comparison is test_acquisition_gpu.py's job).

Every entry that hands a block to the device and runs a batch -- dwell, dwell_device, stage_input + dwell_resident (from host memory and
from a device tensor), dwell_cshort, dwell_ring, dwell_slots, dwell_step2 from host and from device memory, the two timing loops -- runs the
same kernels with the same launch geometry over the same numbers, so their results, grids and row records are equal bit for bit; two calls
of one entry are held to the same rule first (every field, grid value and row record repeats exactly at every shape below, so nothing
is held to a tolerance).  The samples are integers of at most 12 bits stored as complex64, so the cshort entry's int16
block holds exactly the same numbers.

Shapes: the smallest that reach each host path (on-chip plan, lag offset, placement offset, split plans by decimation in frequency and in
time, four-step kernels, zero-padded fallback, QuickSync folding)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from helpers import synth_gps_l1_stream

pytestmark = pytest.mark.gpu

PRNS = (1, 2, 3)
# fft_size, consumed_samples, bit_transition_flag, fold, fs
SHAPES = {
    "onchip_1000": (1000, 1000, False, 0, 1000000),
    "lag_offset_2000": (2000, 2000, True, 0, 1000000),
    "placement_2000": (2000, 1000, False, 0, 1000000),
    "split2_dif_32000": (32000, 32000, False, 0, 32000000),
    "split4_dit_64000": (64000, 64000, False, 0, 64000000),
    "fourstep_6625": (6625, 6625, False, 0, 6625000),
    "padded_4007": (4007, 4007, False, 0, 4007000),
    "fold4_1000": (1000, 4000, False, 4, 1000000),
}
STEP2_BINS = 3


def _step2_allowed(shape):
    return shape not in ("padded_4007", "fold4_1000")


@functools.lru_cache(maxsize=None)
def _block(consumed, fs):
    """(complex64 block of integer samples within 12 bits, the same numbers as int16 [n, 2], another block of the kind)"""
    x = synth_gps_l1_stream(consumed, fs, [PRNS[0], PRNS[2]], [480.0, -730.0], [100.2, 640.7], cn0_dbhz=50.0, seed_noise=consumed)
    x16 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 400.0), -2047, 2047).astype(np.int16)
    xf = (x16[:, 0].astype(np.float32) + 1j * x16[:, 1].astype(np.float32)).astype(np.complex64)
    for a in (x16, xf):
        a.setflags(write=False)
    other = np.ascontiguousarray(xf[::-1])
    other.setflags(write=False)
    return xf, x16, other


@functools.lru_cache(maxsize=None)
def _codes(fs):
    return tuple(oracle.ca_code_complex_sampled(p, fs) for p in PRNS)


def _bank(gpu, shape, use_cfar, keep_grid, step2=None, order=(0, 1, 2)):
    from gnss_sdr_amd.acquisition import PcpsAcquisitionBank
    n, consumed, bt, fold, fs = SHAPES[shape]
    step2 = _step2_allowed(shape) if step2 is None else step2
    acq = PcpsAcquisitionBank(device=gpu, fs_in=fs, fft_size=n, consumed_samples=consumed, bit_transition_flag=bt, fold=fold, doppler_max=1000,
                              doppler_step=500, samples_per_chip=int(np.ceil(fs / 1.023e6)), samples_per_code=float(fs // 1000), max_prn=3,
                              use_cfar=use_cfar, keep_grid=keep_grid, num_doppler_bins_step2=STEP2_BINS if step2 else 0, doppler_step2=125.0)
    assert acq.num_doppler_bins == 4
    for slot, k in enumerate(order):
        acq.set_local_code(slot, _codes(fs)[k])
    return acq


def _state(acq, n_slots=3):
    """what read_grid and read_row_peaks give for every slot"""
    out = []
    for p in range(n_slots):
        pk, ix = acq.read_row_peaks(p)
        out.append((acq.read_grid(p), pk, ix))
    return out


def _same_results(got, exp, tag):
    assert len(got) == len(exp), tag
    for p, (g, e) in enumerate(zip(got, exp)):
        for k in e:
            assert g[k] == e[k], f"{tag}: slot {p} field {k}: {g[k]!r} != {e[k]!r}"


def _same_state(got, exp, tag):
    for p, (g, e) in enumerate(zip(got, exp)):
        for what, a, b in zip(("grid", "row peaks", "row arg-max"), g, e):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{tag}: slot {p}: {what} differ"


@pytest.mark.parametrize("keep_grid", [True, False], ids=["grid", "nogrid"])
@pytest.mark.parametrize("use_cfar", [True, False], ids=["cfar", "ratio"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dwell_entries_agree(gpu, shape, use_cfar, keep_grid):
    import torch
    from gnss_sdr_amd.sample_stream import SampleStream
    n, consumed, bt, fold, fs = SHAPES[shape]
    x, x16, other = _block(consumed, fs)
    xt = torch.from_numpy(x.copy()).cuda(gpu)
    torch.cuda.synchronize()
    ring = SampleStream(4 * consumed, consumed, device=gpu)
    ring.push(other[:37])
    first = ring.push(x)
    assert first == 37
    acq = _bank(gpu, shape, use_cfar, keep_grid)
    state = (lambda: _state(acq)) if keep_grid else (lambda: None)
    same_state = _same_state if keep_grid else (lambda got, exp, tag: None)

    ref = acq.dwell(x, 3)
    ref_state = state()

    def resident(block):
        acq.stage_input(block)
        return acq.dwell_resident(3)

    entries = [("dwell again", lambda: acq.dwell(x, 3)),
               ("dwell_device", lambda: acq.dwell_device(xt.data_ptr(), 3)),
               ("stage_input + dwell_resident", lambda: resident(x)),
               ("stage_input(device) + dwell_resident", lambda: resident(xt)),
               ("dwell_cshort", lambda: acq.dwell_cshort(x16, 3)),
               ("dwell_ring", lambda: acq.dwell_ring(ring, first, 3))]
    for tag, call in entries:
        acq.stage_input(other)  # an entry that failed to hand its block over would search this one
        _same_results(call(), ref, tag)
        same_state(state(), ref_state, tag)

    # a batch of listed slots: the same batch geometry on a handle whose slots 0 and 1 hold those codes; the code table stays as it was
    two = _bank(gpu, shape, use_cfar, keep_grid, order=(2, 0))
    exp2 = two.dwell(x, 2)
    acq.stage_input(other)
    _same_results(acq.dwell_slots(x, [2, 0]), exp2, "dwell_slots [2, 0]")
    if keep_grid:
        _same_state(_state(acq, 2), _state(two, 2), "dwell_slots [2, 0]")
    two.close()
    _same_results(acq.dwell(x, 3), ref, "dwell after dwell_slots")
    same_state(state(), ref_state, "dwell after dwell_slots")
    acq.stage_input(other)
    _same_results(acq.dwell_slots(x, [0, 1, 2]), ref, "dwell_slots prefix")
    same_state(state(), ref_state, "dwell_slots prefix")

    if _step2_allowed(shape):
        order = [2, 0, 1]
        centers = [float(ref[i]["doppler_hz"]) for i in order]
        powers = [ref[i]["input_power"] for i in order]
        for accumulate in ((False, True) if keep_grid else (False,)):
            got = []
            for block in (x, xt):
                acq.dwell(x, 3)  # the grid that accumulate = 1 adds to
                acq.stage_input(other)
                got.append((acq.dwell_step2(block, order, centers, powers, accumulate=accumulate), state()))
            _same_results(got[1][0], got[0][0], f"dwell_step2 device against host, accumulate {accumulate}")
            same_state(got[1][1], got[0][1], f"dwell_step2 device against host, accumulate {accumulate}")

    if keep_grid:
        got = []
        for call in (lambda **kw: acq.dwell(x, 3, **kw), lambda **kw: acq.dwell_device(xt.data_ptr(), 3, **kw)):
            call()
            a = call(accumulate=True, dwell_count=1)
            b = call(accumulate=True, dwell_count=2)
            got.append((a + b, state()))
        _same_results(got[1][0], got[0][0], "accumulate over two calls, dwell_device against dwell")
        _same_state(got[1][1], got[0][1], "accumulate over two calls, dwell_device against dwell")
    elif n in (1000, 64000) and fold <= 1:
        # the pipelined loop: lane 0 still is the handle's own state afterwards, and a second call finds its lanes
        assert acq.time_dwells(x, 3, reps=4, pipelined=True) > 0.0
        _same_results(acq.dwell_resident(3), ref, "dwell_resident after the pipelined loop")
        assert acq.time_dwells(x, 3, reps=4, pipelined=True) > 0.0
        assert acq.time_dwells(x, 3, reps=4) > 0.0
        _same_results(acq.dwell_resident(3), ref, "dwell_resident after the timing loops")
    acq.close()
    ring.close()


def test_argument_errors_text_and_order(gpu):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd._lib import AcqResult
    x, _, _ = _block(1000, 1000000)
    res = (AcqResult * 3)()
    slots = (C.c_uint32 * 3)(0, 1, 2)
    xp = x.ctypes.data_as(C.POINTER(C.c_float))

    def fails(text, call, *args, **kw):
        with pytest.raises(GshError) as e:
            call(*args, **kw)
        assert text in str(e.value), str(e.value)

    def raw(name, *args):
        from gnss_sdr_amd._lib import check
        check(getattr(acq._lib, name)(acq._h, *args))

    acq = _bank(gpu, "onchip_1000", True, False, step2=False)
    fails("no input block resident", acq.dwell_resident, 3)
    fails("n_prn 0 outside 1..3", raw, "gsh_acq_dwell", xp, 0, 0, 1, res)
    fails("n_prn 0 outside 1..3", raw, "gsh_acq_dwell", xp, 0, 1, 1, res)    # the count before the accumulate rule
    fails("n_prn 4 outside 1..3", raw, "gsh_acq_dwell", None, 4, 0, 1, res)  # ... and before the block
    fails("n_prn 0 outside 1..3", raw, "gsh_acq_dwell_device", None, 0, 0, 1, res)
    fails("n_prn 0 outside 1..3", raw, "gsh_acq_dwell_cshort", None, 0, 0, 1, res)
    fails("n_prn 0 outside 1..3", raw, "gsh_acq_dwell_resident", 0, 0, 1, res)
    fails("accumulate != 0 needs the stored grid, but the handle was created with no_grid = 1", acq.dwell, x, 3, accumulate=True)
    fails("accumulate != 0 needs the stored grid", raw, "gsh_acq_dwell", None, 3, 1, 1, res)  # the accumulate rule before the block
    fails("accumulate != 0 needs the stored grid", acq.dwell_resident, 3, accumulate=True)
    fails("null input", raw, "gsh_acq_dwell", None, 3, 0, 1, res)
    fails("null input", raw, "gsh_acq_dwell_device", None, 3, 0, 1, res)
    fails("null input", raw, "gsh_acq_dwell_cshort", None, 3, 0, 1, res)
    fails("null argument", raw, "gsh_acq_dwell", xp, 3, 0, 1, None)
    fails("null argument", raw, "gsh_acq_stage_input", None)
    fails("null argument", raw, "gsh_acq_stage_input_device", None)
    fails("null argument", raw, "gsh_acq_dwell_slots", None, 3, slots, res)
    fails("make_two_steps off", acq.dwell_step2, x, [0], [0.0], [1.0])
    fails("make_two_steps off", acq.dwell_step2, x, [0, 0], [0.0, 0.0], [1.0, 1.0])  # before the slot list is looked at
    fails("prn slot 3 outside 0..2", acq.dwell_slots, x, [0, 3])
    fails("n 4 outside 1..3", acq.dwell_slots, x, [0, 1, 2, 0])
    twice = acq.dwell_slots(x, [1, 1])  # accepted here
    _same_results(twice[1:], twice[:1], "a slot listed twice in dwell_slots")
    acq.close()

    acq = _bank(gpu, "onchip_1000", True, True, order=(0, 1))  # slot 2 without a code
    fails("local code of prn slot 2 has not been set", acq.dwell, x, 3)
    fails("local code of prn slot 2 has not been set", acq.dwell_resident, 3)  # before "no input block resident"
    fails("local code of prn slot 2 has not been set", acq.dwell_slots, x, [1, 2])
    fails("local code of prn slot 2 has not been set", acq.dwell_step2, x, [2, 2], [0.0, 0.0], [1.0, 1.0])  # before "listed twice"
    fails("listed twice", acq.dwell_step2, x, [1, 0, 1], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    fails("is not finite", acq.dwell_step2, x, [1, 1], [0.0, float("nan")], [1.0, 1.0])  # the centre before "listed twice"
    fails("n 4 outside 1..3", acq.dwell_step2, x, [0, 1, 0, 1], [0.0] * 4, [1.0] * 4)
    fails("null argument", raw, "gsh_acq_dwell_step2", None, 3, slots, None, None, 0, 1, res)
    fails("null argument", raw, "gsh_acq_dwell_step2_device", None, 3, slots, None, None, 0, 1, res)
    assert len(acq.dwell(x, 2)) == 2
    acq.close()
