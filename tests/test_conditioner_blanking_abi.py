"""CPU tests of the conditioner's pulse-blanking stage (gsh_cond_set_blanking, gsh_cond_plan_blanked, gsh_cond_blanking_state): declarations, the
host bookkeeping against a sample-by-sample walk, refusals that need no GPU, the timing difference to the block, and the property mapping."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["gsh_cond_blanking", "gsh_cond_set_blanking", "gsh_cond_plan_blanked", "gsh_cond_blanking_state"]


def test_header_declares_the_stage_and_the_abi_version_stays(gsh):
    from gnss_sdr_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\}\s*gsh_cond_blanking\s*;", code)
    assert re.search(r"\bstruct\s+gsh_cond_blanking_state\s*\{", code)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and getattr(gsh, name, None) is not None, name
    assert "#define GSH_ABI_VERSION 25" in src and gsh.gsh_abi_version() == 25
    assert [n for n, _t in _lib.CondBlanking._fields_] == ["pfa", "length", "n_segments_est", "n_segments_reset"]
    assert C.sizeof(_lib.CondBlanking) == 16
    assert [n for n, _t in _lib.CondBlankingState._fields_] == ["thres", "noise_power_estimation", "n_segments", "last_filtered", "n_decided", "n_blanked"]
    assert C.sizeof(_lib.CondBlankingState) == 32 and _lib.CondBlankingState.n_decided.offset == 16
    assert C.sizeof(_lib.CondConf) == 96                               # gsh_cond_conf keeps its layout
    assert "Not stages of this chain (they stay loose calls): Notch_Filter, Notch_Filter_Lite" in src


def _walk(n_filter_outputs, fs_in, fs_out):
    """direct_resampler_conditioner_cc.cc:52-59,83-110 walked sample by sample over n_filter_outputs inputs: how many outputs it produces
    (tests/test_conditioner_abi.py::_walk, restated)"""
    two_32 = 1 << 32
    if fs_in >= fs_out:
        step = int(np.floor(two_32 * fs_out / fs_in))
        phase, lphase, count = 0, 0, 0
        for _ in range(n_filter_outputs):
            if phase <= lphase:
                count += 1
            lphase = phase
            phase = (phase + step) % two_32
        return count
    step = int(np.floor(two_32 * fs_in / fs_out))
    phase, lphase, count, i = 0, 0, 0, 0
    while True:
        lphase = phase
        phase = (phase + step) % two_32
        if phase <= lphase:
            i += 1
        if i >= n_filter_outputs:
            return count
        count += 1


K = 7


@pytest.mark.parametrize("rates", [(0.0, 0.0), (25e6, 4e6), (4e6, 5e6)], ids=["none", "25to4", "4to5"])
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("L", [1, 5, 32])
def test_plan_is_the_walk_over_whole_segments(L, D, rates):
    """every total 0 .. 3 L D + K: the count is the resampler's walk over floor(M / L) L mitigated filter outputs, M = ceil(N / D)"""
    from gnss_sdr_amd.conditioner import outputs_after
    fs_in, fs_out = rates
    kw = dict(taps=np.ones(K, np.float32), decimation=D, sampling_freq_hz=1.0, fs_in=fs_in, fs_out=fs_out)
    walked = {}
    got, want = [], []
    for n in range(0, 3 * L * D + K + 1):
        m = (n + D - 1) // D
        mp = (m // L) * L
        if mp not in walked:
            walked[mp] = mp if fs_in == fs_out else _walk(mp, fs_in, fs_out)
        want.append(walked[mp])
        got.append(outputs_after(n, "gr_complex", blanking=dict(length=L), **kw))
    assert got == want
    assert got[-1] >= (3 * L if fs_in == fs_out else 1) and all(b >= a for a, b in zip(got, got[1:]))


def test_plan_with_null_blanking_is_the_plain_plan_and_bad_values_are_refused(gsh):
    from gnss_sdr_amd import _lib
    from gnss_sdr_amd.conditioner import _conf
    c, _keep = _conf("ibyte", False, np.ones(5, np.float32), 2, 0.0, 4e6, 25e6, 4e6)
    a, b = C.c_uint64(0), C.c_uint64(0)
    for n in (0, 1, 2, 77, 1000, 3_000_000_017):
        assert gsh.gsh_cond_plan(C.byref(c), n, C.byref(a)) == 0
        assert gsh.gsh_cond_plan_blanked(C.byref(c), None, n, C.byref(b)) == 0
        assert a.value == b.value
    good = dict(pfa=0.04, length=32, n_segments_est=10, n_segments_reset=20)
    for what, kw, text in [("pfa 0", dict(pfa=0.0), b"pfa"), ("pfa 1", dict(pfa=1.0), b"pfa"), ("negative pfa", dict(pfa=-0.5), b"pfa"),
                           ("length 0", dict(length=0), b"length"), ("length 4097", dict(length=4097), b"length"), ("negative length", dict(length=-3), b"length"),
                           ("negative est", dict(n_segments_est=-1), b"negative"), ("negative reset", dict(n_segments_reset=-1), b"negative")]:
        bl = _lib.CondBlanking(**dict(good, **kw))
        b.value = 5
        assert gsh.gsh_cond_plan_blanked(C.byref(c), C.byref(bl), 100, C.byref(b)) == 1, what
        assert text in gsh.gsh_last_error(), (what, gsh.gsh_last_error())
        assert b.value == 0
    bl = _lib.CondBlanking(**good)
    assert gsh.gsh_cond_plan_blanked(C.byref(c), C.byref(bl), 100, None) == 1
    assert gsh.gsh_cond_plan_blanked(None, C.byref(bl), 100, C.byref(b)) == 1
    assert gsh.gsh_cond_set_blanking(None, C.byref(bl)) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_cond_blanking_state(None, None) == 1


@pytest.mark.parametrize("L", [1, 5, 32])
def test_the_block_consumes_the_planned_segments_or_one_less(L):
    """PulseBlankingOracle (the block, statement by statement) offered the same stream in arbitrary partitions -- what it did not consume is offered
    again in front of the new items, as the scheduler does -- has consumed M' or M' - L items after every call: it leaves a segment that ends on
    the last offered item for the next call, the conditioner emits it.  Nothing else differs."""
    from gnss_sdr_amd.conditioner import outputs_after
    from oracle.pulse_blanking_oracle import PulseBlankingOracle
    rng = np.random.default_rng(100 + L)
    n = 40 * L + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    whole = PulseBlankingOracle(0.04, L, 5, 9)
    ref, ref_done = whole.general_work(x)
    for trial in range(4):
        orc = PulseBlankingOracle(0.04, L, 5, 9)
        out, consumed, offered, exact, behind = [], 0, 0, 0, 0
        while offered < n:
            offered = offered + int(rng.integers(1, 3 * L + 2))
            if rng.integers(0, 3) == 0:
                offered += -offered % L            # an offer that ends exactly on a segment
            offered = min(n, offered)
            y, done = orc.general_work(x[consumed:offered])
            out.append(y)
            consumed += done
            planned = outputs_after(offered, "gr_complex", blanking=dict(length=L, segments_est=5, segments_reset=9))
            assert planned == (offered // L) * L
            assert consumed in (planned, planned - L), (L, trial, offered, consumed, planned)
            assert (consumed == planned - L) == (offered % L == 0)
            exact += consumed == planned
            behind += consumed != planned
        assert behind > 0 and (exact > 0 or L == 1)   # (with L = 1 every offer ends on a segment)
        out = np.concatenate(out)
        assert np.array_equal(out[:ref_done].view(np.uint32), ref.view(np.uint32))     # the content does not depend on the partition


def test_property_names_of_the_blanking_filter_map_to_the_handle():
    from gnss_sdr_amd import SignalConditioner
    p, q = SignalConditioner.properties, SignalConditioner.properties_with_mitigation
    taps = [0.25, 0.5, 0.25]
    defaults = dict(pfa=0.04, length=32, segments_est=12500, segments_reset=5000000)
    assert q({"InputFilter": {"implementation": "Pulse_Blanking_Filter"}}) == dict(input_kind="gr_complex", inverted_spectrum=False, blanking=defaults)
    kw = q({"DataTypeAdapter": {"implementation": "Ibyte_To_Complex", "inverted_spectrum": "true"},
            "InputFilter": {"implementation": "Pulse_Blanking_Filter", "pfa": 0.01, "length": 64, "segments_est": 100, "segments_reset": 1000, "IF": 1.0},
            "Resampler": {"implementation": "Direct_Resampler", "sample_freq_in": 25e6, "sample_freq_out": 4e6}})
    # |IF| <= 1: no filter (pulse_blanking_filter.cc:73)
    assert kw == dict(input_kind="ibyte", inverted_spectrum=True, fs_in=25e6, fs_out=4e6, blanking=dict(pfa=0.01, length=64, segments_est=100, segments_reset=1000))
    assert "taps" not in q({"InputFilter": {"implementation": "Pulse_Blanking_Filter", "IF": -1.0, "taps": taps}})
    kw = q({"InputFilter": {"implementation": "Pulse_Blanking_Filter", "IF": -2.5e6, "taps": taps}})
    assert kw == dict(input_kind="gr_complex", inverted_spectrum=False, taps=taps, decimation=1, center_freq_hz=-2.5e6, sampling_freq_hz=4e6, blanking=defaults)
    kw = q({"InputFilter": {"implementation": "Pulse_Blanking_Filter", "if": 1e6, "sampling_frequency": 20e6, "taps": taps, "length": "16"}})
    assert (kw["center_freq_hz"], kw["sampling_freq_hz"], kw["decimation"], kw["blanking"]["length"]) == (1e6, 20e6, 1, 16)
    kw = q({"InputFilter": {"implementation": "Pulse_Blanking_Filter", "if": 1e6, "IF": 2e6, "taps": taps}})
    assert kw["center_freq_hz"] == 2e6                                  # IF wins over `if` (:52-53)
    for role in ({"InputFilter": {"implementation": "Pulse_Blanking_Filter", "IF": 2e6}},                       # |IF| > 1 without taps
                 {"InputFilter": {"implementation": "Pulse_Blanking_Filter", "item_type": "cshort"}},
                 {"InputFilter": {"implementation": "Notch_Filter"}}, {"InputFilter": {"implementation": "Notch_Filter_Lite"}},
                 {"InputFilter": {"implementation": "Pulse_Blanking_Filter"}, "Resampler": {"implementation": "Mmse_Resampler"}}):
        with pytest.raises(ValueError):
            q(role)
    # everything else is properties()
    role = {"DataTypeAdapter": {"implementation": "Ishort_To_Complex"}, "InputFilter": {"implementation": "Fir_Filter", "taps": taps}}
    assert q(role) == p(role) and q({}) == p({})
    with pytest.raises(ValueError):
        p({"InputFilter": {"implementation": "Pulse_Blanking_Filter"}})   # properties() itself still does not cover it
    with pytest.raises(ValueError):
        from gnss_sdr_amd.conditioner import outputs_after
        outputs_after(10, blanking=dict(lenght=3))
