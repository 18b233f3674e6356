"""The batch entries of the correlator banks held to EACH OTHER (the oracle comparisons are test_tracking_gpu.py's, test_tracking_wide_taps_gpu.py's and
test_mcorr16_gpu.py's job).

Every way of handing one batch to a bank -- correlate; upload + launch + read; upload + time_launches + read; a stream in host memory, in borrowed
device memory, in a ring, or shifted by a sample base; the one-job facades -- stages the same table and runs the same kernels with the same launch
geometry over the same numbers, so the outputs are equal bit for bit.  A handle whose buffers have grown (and been passed by smaller batches again), and a
handle that has just refused a call, must answer what a fresh handle answers.  Every pair below repeats exactly; nothing is held to a tolerance.

Shapes: GPS C/A codes of 1023 chips, windows of 4096 to 4300 samples (two splits per job at these job counts, so the partial sums' buffer is
reached), streams of 5000 to 9000 samples; batches of 5 jobs (1, 3 and 5 taps, and a 3-tap job with its fused 1-tap partner: launch lists, the partner
table and fusion) and of 70 jobs (past the 64- and 32-job floors of the staging buffers)."""
import functools

import numpy as np
import pytest

import oracle
from helpers import synth_gps_l1_stream, tracking_params_for

pytestmark = pytest.mark.gpu

FS = 4e6
N_STREAM = 9000
N_SHORT = 5000
BASE = 1024  # samples the shifted stream is offset by
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = 1, 4, 5
WIDE_33 = [float(v) for v in np.linspace(-4.0, 4.0, 33)]
WIDE_17 = [float(v) for v in np.linspace(-2.0, 2.0, 17)]


@functools.lru_cache(maxsize=None)
def _x():
    """(complex64 stream of integer samples within 8 bits, the same numbers as int16 [n, 2])"""
    x = synth_gps_l1_stream(N_STREAM, FS, [1, 2, 3], [1000.0, -2000.0, 300.0], [5.0, 300.0, 800.0], seed_noise=4)
    x16 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 30.0), -127, 127).astype(np.int16)
    xf = (x16[:, 0].astype(np.float32) + 1j * x16[:, 1].astype(np.float32)).astype(np.complex64)
    for a in (x16, xf):
        a.setflags(write=False)
    return xf, x16


@functools.lru_cache(maxsize=None)
def _params():
    rng = np.random.default_rng(9)
    return tuple(tracking_params_for(FS, d, rng) for d in (1000.0, -2000.0, 300.0))


def _job(off, n, slot, shifts, **more):
    return dict(sample_offset=off, n_samples=n, code_slot=slot, shifts_chips=list(shifts), **_params()[slot], **more)


def _narrow_jobs(n_jobs=5, shift=0):
    """the 5-job batch: 1, 3 and 5 taps, then a 3-tap job and a 1-tap job over its window with its NCO values; longer batches repeat the pattern"""
    five = [_job(shift + 10, 4100, 0, [0.0]), _job(shift + 333, 4096, 1, [-0.5, 0.0, 0.5]), _job(shift + 601, 4299, 2, [-1.0, -0.5, 0.0, 0.5, 1.0]),
            _job(shift + 77, 4200, 0, [-0.25, 0.0, 0.25]), _job(shift + 77, 4200, 0, [0.0])]
    return [dict(five[i % 5], sample_offset=five[i % 5]["sample_offset"] + (i // 5) * 7) for i in range(n_jobs)]


def _wide_jobs(n_jobs=2, shift=0):
    two = [_job(shift + 21, 4100, 0, WIDE_33), _job(shift + 402, 4297, 1, WIDE_17)]
    return [dict(two[i % 2], sample_offset=two[i % 2]["sample_offset"] + (i // 2) * 5) for i in range(n_jobs)]


def _jobs16(n_jobs=3, shift=0):
    from gnss_sdr_amd.tracking16 import make_job16
    three = [(shift + 10, 4100, 0, [0.0]), (shift + 333, 4096, 1, [-0.5, 0.0, 0.5]), (shift + 601, 4299, 2, [-1.0, -0.5, 0.0, 0.5, 1.0])]
    out = []
    for i in range(n_jobs):
        off, n, slot, shifts = three[i % 3]
        p = _params()[slot]
        out.append(make_job16(off + (i // 3) * 7, n, slot, p["rem_carr_phase_rad"], p["phase_step_rad"], p["rem_code_phase_chips"], p["code_phase_step_chips"], shifts))
    return out


def _code16(prn):
    return np.stack([oracle.ca_code(prn), np.zeros(1023, np.float32)], -1).astype(np.int16)


def _bank(gpu, stream=None, slots=3):
    from gnss_sdr_amd.tracking import CorrelatorBank
    bank = CorrelatorBank(3, 1023, device=gpu)
    for c in range(slots):
        bank.set_code(c, oracle.ca_code(c + 1))
    if stream is not None:
        bank.set_stream_host(stream)
    return bank


def _bank16(gpu, stream=None, slots=3):
    from gnss_sdr_amd.tracking16 import CorrelatorBank16
    bank = CorrelatorBank16(3, 1023, device=gpu)
    for c in range(slots):
        bank.set_code(c, _code16(c + 1))
    if stream is not None:
        bank.set_stream_host(stream)
    return bank


def _ring(gpu, x):
    from gnss_sdr_amd.sample_stream import SampleStream
    ring = SampleStream(2 * N_STREAM, 4400, device=gpu)
    assert ring.push(x) == 0
    return ring


@functools.lru_cache(maxsize=None)
def _fresh(gpu, kind, n_jobs=0, n_stream=N_STREAM, shift=0):
    """what a fresh handle answers for a batch of the kind over the first n_stream samples: the yardstick of every comparison, computed once"""
    xf, x16 = _x()
    if kind == "bank16":
        bank = _bank16(gpu, x16[:n_stream])
        out = bank.correlate(_jobs16(n_jobs or 3, shift))
    else:
        bank = _bank(gpu, xf[:n_stream])
        out = bank.correlate(_narrow_jobs(n_jobs or 5, shift)) if kind == "narrow" else bank.correlate_wide(_wide_jobs(n_jobs or 2, shift))
    bank.close()
    assert np.any(out != 0)
    out.setflags(write=False)
    return out


def _same(got, exp, tag):
    assert got.shape == exp.shape and np.array_equal(got.view(np.uint32 if got.dtype == np.complex64 else np.int16), exp.view(np.uint32 if exp.dtype == np.complex64 else np.int16)), tag


def _raises(code, call, *args):
    from gnss_sdr_amd import GshError
    with pytest.raises(GshError) as e:
        call(*args)
    assert e.value.code == code, str(e.value)
    return str(e.value)


# ---- the narrow bank ----------------------------------------------------------------------------------------------------------------------------------
def test_narrow_entries_agree(gpu):
    import torch
    xf, _ = _x()
    exp = _fresh(gpu, "narrow")
    jobs = _narrow_jobs()
    bank = _bank(gpu, xf)
    _same(bank.correlate(jobs), exp, "correlate, twice")
    bank.upload_jobs(jobs)
    bank.launch()
    bank.synchronize()
    _same(bank.read_outputs(), exp, "upload + launch + synchronize + read_outputs")
    bank.upload_jobs(jobs)
    assert bank.time_launches(2) > 0
    _same(bank.read_outputs(), exp, "upload + time_launches + read_outputs")
    xd = torch.from_numpy(np.concatenate([xf, np.zeros(2, np.complex64)])).to(torch.device("cuda", gpu))
    bank.set_stream_device(xd.data_ptr(), len(xf), keepalive=xd)
    _same(bank.correlate(jobs), exp, "set_stream_device")
    ring = _ring(gpu, xf)
    bank.set_stream_ring(ring)
    _same(bank.correlate(jobs), exp, "ring-bound correlate")
    bank.upload_jobs(jobs)
    bank.launch()
    bank.synchronize()
    _same(bank.read_outputs(), exp, "ring-bound upload + launch")
    bank.set_stream_ring(None)
    bank.set_stream_host(np.concatenate([np.zeros(BASE, np.complex64), xf]))
    bank.set_sample_base(BASE)
    _same(bank.correlate(jobs), exp, "sample base over a stream offset by as much")
    bank.upload_jobs(jobs)
    assert bank.time_launches(2) > 0
    _same(bank.read_outputs(), exp, "sample base, upload + time_launches")
    bank.close()
    ring.close()


@pytest.mark.parametrize("form", ["rates_mode0", "rates_mode1", "six_arguments"])
def test_narrow_facade_equals_the_banks_row(gpu, form):
    from gnss_sdr_amd.tracking import HipMulticorrelatorRealCodes
    xf, _ = _x()
    n = 4100
    win = np.ascontiguousarray(xf[333:333 + n])
    p = _params()[1]
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    rates = dict(phase_rate_step_rad=float(np.float32(1e-9)), code_phase_rate_step_chips=float(np.float32(1e-10)))
    mode = {"rates_mode0": 0, "rates_mode1": 1, "six_arguments": 2}[form]
    if form == "six_arguments":
        rates["phase_rate_step_rad"] = 0.0
    bank = _bank(gpu, win)
    exp = bank.correlate([dict(_job(0, n, 1, shifts), high_dyn=mode, **rates)])
    bank.close()
    mc = HipMulticorrelatorRealCodes(gpu)
    out = np.zeros(3, np.complex64)
    mc.init(n + 100, 3)
    mc.set_local_code_and_taps(1023, oracle.ca_code(2), shifts)
    mc.set_input_output_vectors(out, win)
    mc.set_high_dynamics_resampler(mode != 0)
    for _ in range(2):
        if form == "six_arguments":
            mc.Carrier_wipeoff_multicorrelator_resampler(p["rem_carr_phase_rad"], p["phase_step_rad"], p["rem_code_phase_chips"], p["code_phase_step_chips"],
                                                         rates["code_phase_rate_step_chips"], n)
        else:
            mc.Carrier_wipeoff_multicorrelator_resampler(p["rem_carr_phase_rad"], p["phase_step_rad"], rates["phase_rate_step_rad"], p["rem_code_phase_chips"],
                                                         p["code_phase_step_chips"], rates["code_phase_rate_step_chips"], n)
        assert np.any(out != 0)
        _same(out, exp[0, :3], form)
    mc.close()


# ---- the wide bank ------------------------------------------------------------------------------------------------------------------------------------
def test_wide_entries_agree(gpu):
    xf, _ = _x()
    exp = _fresh(gpu, "wide")
    jobs = _wide_jobs()
    bank = _bank(gpu, xf)
    _same(bank.correlate_wide(jobs), exp, "correlate_wide, twice")
    assert bank.time_launches_wide(jobs, 2) > 0
    _same(bank.correlate_wide(jobs), exp, "correlate_wide after time_launches_wide")
    ring = _ring(gpu, xf)
    bank.set_stream_ring(ring)
    _same(bank.correlate_wide(jobs), exp, "ring-bound correlate_wide")
    bank.close()
    ring.close()


def test_wide_facade_equals_the_banks_row(gpu):
    from gnss_sdr_amd.tracking import HipMulticorrelatorRealCodes
    xf, _ = _x()
    n = 4100
    win = np.ascontiguousarray(xf[21:21 + n])
    p = _params()[0]
    bank = _bank(gpu, win)
    exp = bank.correlate_wide([_job(0, n, 0, WIDE_33)])
    bank.close()
    mc = HipMulticorrelatorRealCodes(gpu)
    out = np.zeros(33, np.complex64)
    mc.init(n, 33)
    mc.set_local_code_and_taps(1023, oracle.ca_code(1), np.array(WIDE_33, np.float32))
    mc.set_input_output_vectors(out, win)
    mc.set_high_dynamics_resampler(False)
    mc.Carrier_wipeoff_multicorrelator_resampler(p["rem_carr_phase_rad"], p["phase_step_rad"], 0.0, p["rem_code_phase_chips"], p["code_phase_step_chips"], 0.0, n)
    assert np.any(out != 0)
    _same(out, exp[0, :33], "33 correlators")
    mc.close()


# ---- the 16-bit bank ----------------------------------------------------------------------------------------------------------------------------------
def test_bank16_entries_agree(gpu):
    import torch
    from gnss_sdr_amd.tracking16 import HipMulticorrelator16sc
    _, x16 = _x()
    exp = _fresh(gpu, "bank16")
    jobs = _jobs16()
    bank = _bank16(gpu, x16)
    _same(bank.correlate(jobs), exp, "correlate, twice")
    bank.upload(jobs)
    bank.launch()
    _same(bank.read(), exp, "upload + launch + read")
    bank.upload(jobs)
    assert bank.time_launches(2) > 0
    _same(bank.read(), exp, "upload + time_launches + read")
    xd = torch.from_numpy(np.array(x16)).to(torch.device("cuda", gpu))
    bank.set_stream_device(xd.data_ptr(), len(x16), keepalive=xd)
    _same(bank.correlate(jobs), exp, "set_stream_device")
    bank.close()
    # the facade: job 1 of the batch as the one job of a call
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    p = _params()[1]
    mc = HipMulticorrelator16sc(gpu)
    out = np.zeros((3, 2), np.int16)
    mc.init(5000, 3)
    mc.set_local_code_and_taps(1023, _code16(2), shifts)
    mc.set_input_output_vectors(out, np.ascontiguousarray(x16[333:333 + 4096]))
    mc.Carrier_wipeoff_multicorrelator_resampler(p["rem_carr_phase_rad"], p["phase_step_rad"], p["rem_code_phase_chips"], p["code_phase_step_chips"], 4096)
    _same(out, exp[1, :3], "HipMulticorrelator16sc")
    mc.close()


# ---- growth -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["narrow", "wide", "bank16"])
def test_grown_buffers_answer_as_a_fresh_handle(gpu, kind):
    xf, x16 = _x()
    small = {"narrow": 5, "wide": 2, "bank16": 3}[kind]
    make = {"narrow": _narrow_jobs, "wide": _wide_jobs, "bank16": _jobs16}[kind]
    bank = _bank16(gpu, x16) if kind == "bank16" else _bank(gpu, xf)
    run = bank.correlate_wide if kind == "wide" else bank.correlate
    for n_jobs in (small, 70, small):
        _same(run(make(n_jobs)), _fresh(gpu, kind, n_jobs), f"{kind}: {n_jobs} jobs after the batches before")
    # the owned stream: short, longer (the batch now reaches past the short one's end), short again
    for n_stream, shift in ((N_SHORT, 0), (N_STREAM, 4000), (N_SHORT, 0)):
        bank.set_stream_host((x16 if kind == "bank16" else xf)[:n_stream])
        _same(run(make(small, shift)), _fresh(gpu, kind, small, n_stream, shift), f"{kind}: a stream of {n_stream} samples after the streams before")
    bank.close()


# ---- refusal, then use --------------------------------------------------------------------------------------------------------------------------------
def test_narrow_refusals_leave_the_handle_usable(gpu):
    xf, _ = _x()
    exp = _fresh(gpu, "narrow")
    jobs = _narrow_jobs()
    bank = _bank(gpu, slots=2)
    assert "no sample stream" in _raises(ERR_STATE, bank.correlate, jobs[:2])
    bank.upload_jobs(jobs[:2])
    _raises(ERR_STATE, bank.launch)
    bank.set_stream_host(xf)
    assert "code slot 2" in _raises(ERR_STATE, bank.correlate, jobs)  # an empty code slot
    bank.set_code(2, oracle.ca_code(3))
    _same(bank.correlate(jobs), exp, "after no stream and an empty slot")
    past = jobs[:4] + [dict(jobs[4], sample_offset=N_STREAM - 100)]
    assert "past the 9000-sample stream" in _raises(ERR_INVALID, bank.correlate, past)
    bank.upload_jobs(past)
    _raises(ERR_INVALID, bank.launch)
    _raises(ERR_INVALID, bank.time_launches, 2)
    _same(bank.correlate(jobs), exp, "after a window past the stream")
    assert "share high_dyn" in _raises(ERR_UNSUPPORTED, bank.correlate, jobs[:1] + [dict(jobs[1], high_dyn=1)])
    _raises(ERR_INVALID, bank.read_outputs, 1)  # a refused batch leaves none staged
    _same(bank.correlate(jobs), exp, "after mixed high_dyn")
    ring = _ring(gpu, xf)
    bank.set_stream_ring(ring)
    text = _raises(ERR_INVALID, bank.correlate, jobs[:4] + [dict(jobs[4], sample_offset=N_STREAM - 100)])
    assert "not resident" in text
    _same(bank.correlate(jobs), exp, "after a ring window that is not resident")
    bank.close()
    ring.close()


def test_wide_refusals_leave_the_handle_usable(gpu):
    xf, _ = _x()
    exp = _fresh(gpu, "wide")
    jobs = _wide_jobs()
    bank = _bank(gpu, slots=1)
    assert "no sample stream" in _raises(ERR_STATE, bank.correlate_wide, jobs[:1])
    bank.set_stream_host(xf)
    assert "code slot 1" in _raises(ERR_STATE, bank.correlate_wide, jobs)
    bank.set_code(1, oracle.ca_code(2))
    _same(bank.correlate_wide(jobs), exp, "after no stream and an empty slot")
    assert "past the 9000-sample stream" in _raises(ERR_INVALID, bank.correlate_wide, [jobs[0], dict(jobs[1], sample_offset=N_STREAM - 100)])
    _raises(ERR_INVALID, bank.time_launches_wide, [jobs[0], dict(jobs[1], sample_offset=N_STREAM - 100)], 2)
    _same(bank.correlate_wide(jobs), exp, "after a window past the stream")
    assert "shifts must ascend" in _raises(ERR_INVALID, bank.correlate_wide, [jobs[0], dict(jobs[1], shifts_chips=WIDE_17[::-1])])
    _same(bank.correlate_wide(jobs), exp, "after a descending shift")
    ring = _ring(gpu, xf)
    bank.set_stream_ring(ring)
    text = _raises(ERR_INVALID, bank.correlate_wide, [jobs[0], dict(jobs[1], sample_offset=N_STREAM - 100)])
    assert "job 1" in text and "not resident" in text
    _same(bank.correlate_wide(jobs), exp, "after a ring window that is not resident")
    bank.close()
    ring.close()


def test_bank16_refusals_leave_the_handle_usable(gpu):
    _, x16 = _x()
    exp = _fresh(gpu, "bank16")
    jobs = _jobs16()
    bank = _bank16(gpu, slots=2)
    _raises(ERR_INVALID, bank.correlate, jobs[:2])  # no stream attached
    bank.set_stream_host(x16)
    assert "code slot 2" in _raises(ERR_INVALID, bank.correlate, jobs)
    bank.set_code(2, _code16(3))
    _same(bank.correlate(jobs), exp, "after no stream and an empty slot")
    past = _jobs16()
    past[2].sample_offset = N_STREAM - 100
    assert "leaves the stream" in _raises(ERR_INVALID, bank.correlate, past)
    _same(bank.correlate(jobs), exp, "after a window past the stream")
    bank.close()


def test_bank16_stale_stream_is_refused_at_launch(gpu):
    """upload against the whole tensor, re-attach it declared shorter than a window's end: launch and time_launches refuse before anything is queued (the
    tensor keeps its full length throughout, so nothing here can read outside it)"""
    import torch
    _, x16 = _x()
    exp = _fresh(gpu, "bank16")
    jobs = _jobs16()
    xd = torch.from_numpy(np.array(x16)).to(torch.device("cuda", gpu))
    bank = _bank16(gpu)
    bank.set_stream_device(xd.data_ptr(), N_STREAM, keepalive=xd)
    bank.upload(jobs)
    bank.launch()
    _same(bank.read(), exp, "the whole tensor")
    bank.set_stream_device(xd.data_ptr(), 4500, keepalive=xd)  # job 2 ends at sample 4900
    assert "past the 4500-sample stream" in _raises(ERR_INVALID, bank.launch)
    assert "past the 4500-sample stream" in _raises(ERR_INVALID, bank.time_launches, 2)
    bank.set_stream_device(xd.data_ptr(), N_STREAM, keepalive=xd)
    bank.launch()
    _same(bank.read(), exp, "the whole tensor again")
    bank.close()
