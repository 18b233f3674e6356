"""CPU tests of the conditioner's notch stage (gsh_cond_set_notch, gsh_cond_plan_notched, gsh_cond_notch_state): declarations, the host bookkeeping
against its closed form (W' = L floor((M - 1) / L) notch outputs, then the resampler's count), refusals that need no GPU, and the property mapping."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["gsh_cond_notch", "gsh_cond_set_notch", "gsh_cond_plan_notched", "gsh_cond_notch_state"]


def test_header_declares_the_stage_and_the_abi_version_stays(gsh):
    from gnss_sdr_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\}\s*gsh_cond_notch\s*;", code)
    assert re.search(r"\bstruct\s+gsh_cond_notch_state\s*\{", code)
    for name in NAMES[1:]:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and getattr(gsh, name, None) is not None, name
    assert "#define GSH_ABI_VERSION 25" in src and gsh.gsh_abi_version() == 25
    assert [n for n, _t in _lib.CondNotch._fields_] == ["pfa", "p_c_factor", "length", "n_segments_est", "n_segments_reset", "n_segments_coeff"]
    assert C.sizeof(_lib.CondNotch) == 24
    assert [n for n, _t in _lib.CondNotchState._fields_] == ["thres", "noise_pow_est", "n_segments", "filter_state", "n_segments_coeff", "reserved", "z0", "n_decided",
                                                             "n_filtered"]
    assert C.sizeof(_lib.CondNotchState) == 48 and _lib.CondNotchState.z0.offset == 24 and _lib.CondNotchState.n_decided.offset == 32
    assert C.sizeof(_lib.CondConf) == 96                               # gsh_cond_conf keeps its layout
    assert "Not stages of this chain (they stay loose calls): Notch_Filter, Notch_Filter_Lite" in src
    assert src.index("gsh_cond_set_notch below") < src.index("Not stages of this chain")


def _resampled(m, fs_in, fs_out):
    """outputs of the direct resampler over m inputs: the j with m(j) < m (resampler.hip's integers)"""
    if m == 0 or fs_in == fs_out:
        return m
    two_32 = 1 << 32
    if fs_in >= fs_out:
        step = int(np.floor(two_32 * fs_out / fs_in))
        return ((m - 1) * step >> 32) + 1              # ceil(j 2^32 / step) <= m - 1
    step = int(np.floor(two_32 * fs_in / fs_out))
    return -((-m * two_32) // step) - 1                # floor((j + 1) step / 2^32) < m


CHAINS = {"no filter": dict(), "D1": dict(taps=np.ones(7, np.float32), decimation=1), "D2": dict(taps=np.ones(7, np.float32), decimation=2),
          "D5": dict(taps=np.ones(7, np.float32), decimation=5)}


@pytest.mark.parametrize("rates", [(0.0, 0.0), (25e6, 4e6), (4e6, 5e6)], ids=["none", "25to4", "4to5"])
@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("L", [2, 32, 100, 1024])
def test_plan_is_the_closed_form(L, chain, rates):
    """around every one of the first four segment boundaries (and from 0 on): W' = L floor((M - 1) / L), M = ceil(N / D), then the resampler's count"""
    from gnss_sdr_amd.conditioner import outputs_after
    fs_in, fs_out = rates
    kw = dict(CHAINS[chain], sampling_freq_hz=1.0, fs_in=fs_in, fs_out=fs_out)
    D = kw.get("decimation", 1)
    totals = set(range(0, 2 * D + 3))
    for s in range(1, 5):
        edge = s * L * D + 1            # the first total with M = s L + 1: segment s - 1 is complete
        totals.update(range(max(0, edge - 2 * D - 1), edge + 2 * D + 2))
    got, want, steps = [], [], 0
    for n in sorted(totals):
        m = (n + D - 1) // D
        w = 0 if m == 0 else L * ((m - 1) // L)
        want.append(_resampled(w, fs_in, fs_out))
        got.append(outputs_after(n, "gr_complex", notch=dict(length=L), **kw))
        steps += m >= 1 and (m - 1) % L == 0 and (m - 1) // L >= 1 and (n - 1 + D - 1) // D == m - 1   # this total completes a segment
    assert got == want
    assert steps >= 4 and got[-1] >= 1 and all(b >= a for a, b in zip(got, got[1:]))   # (with L = 2 the window behind the fourth boundary reaches the fifth)
    if fs_in == fs_out:
        assert sorted(set(got))[:5] == [0, L, 2 * L, 3 * L, 4 * L]


def test_resampled_counts_restate_a_walk_of_the_reference_accumulator():
    """_resampled against direct_resampler_conditioner_cc.cc:52-59,83-110 walked sample by sample (tests/test_conditioner_blanking_abi.py::_walk)"""
    from test_conditioner_blanking_abi import _walk
    for fs_in, fs_out in ((25e6, 4e6), (4e6, 5e6)):
        for m in (1, 2, 3, 31, 32, 33, 64, 100, 200, 1024):
            assert _resampled(m, fs_in, fs_out) == _walk(m, fs_in, fs_out), (fs_in, fs_out, m)


def test_plan_with_null_notch_is_the_plain_plan_and_bad_values_are_refused(gsh):
    from gnss_sdr_amd import _lib
    from gnss_sdr_amd.conditioner import _conf
    c, _keep = _conf("ibyte", False, np.ones(5, np.float32), 2, 0.0, 4e6, 25e6, 4e6)
    a, b = C.c_uint64(0), C.c_uint64(0)
    for n in (0, 1, 2, 77, 1000, 3_000_000_017):
        assert gsh.gsh_cond_plan(C.byref(c), n, C.byref(a)) == 0
        assert gsh.gsh_cond_plan_notched(C.byref(c), None, n, C.byref(b)) == 0
        assert a.value == b.value
    good = dict(pfa=0.001, p_c_factor=0.9, length=32, n_segments_est=10, n_segments_reset=20, n_segments_coeff=0)
    for what, kw, text in [("pfa 0", dict(pfa=0.0), b"pfa"), ("pfa 1", dict(pfa=1.0), b"pfa"), ("negative pfa", dict(pfa=-0.5), b"pfa"),
                           ("pfa nan", dict(pfa=float("nan")), b"pfa"),
                           ("length 1", dict(length=1), b"length"), ("length 0", dict(length=0), b"length"), ("length 1025", dict(length=1025), b"length"),
                           ("negative length", dict(length=-3), b"length"),
                           ("negative est", dict(n_segments_est=-1), b"negative"), ("negative reset", dict(n_segments_reset=-1), b"negative"),
                           ("negative coeff", dict(n_segments_coeff=-1), b"negative"),
                           ("p inf", dict(p_c_factor=float("inf")), b"p_c_factor"), ("p nan", dict(p_c_factor=float("nan")), b"p_c_factor")]:
        nt = _lib.CondNotch(**dict(good, **kw))
        b.value = 5
        assert gsh.gsh_cond_plan_notched(C.byref(c), C.byref(nt), 100, C.byref(b)) == 1, what
        assert text in gsh.gsh_last_error(), (what, gsh.gsh_last_error())
        assert b.value == 0
    nt = _lib.CondNotch(**good)
    for ok in (dict(length=2), dict(length=1024), dict(n_segments_coeff=7), dict(n_segments_est=0, n_segments_reset=0), dict(p_c_factor=-0.5)):
        assert gsh.gsh_cond_plan_notched(C.byref(c), C.byref(_lib.CondNotch(**dict(good, **ok))), 100, C.byref(b)) == 0, ok
    assert gsh.gsh_cond_plan_notched(C.byref(c), C.byref(nt), 100, None) == 1
    assert gsh.gsh_cond_plan_notched(None, C.byref(nt), 100, C.byref(b)) == 1
    assert gsh.gsh_cond_set_notch(None, C.byref(nt)) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_cond_notch_state(None, None) == 1


def test_property_names_of_the_notch_filters_map_to_the_handle():
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.conditioner import outputs_after
    p, q, r = SignalConditioner.properties, SignalConditioner.properties_with_mitigation, SignalConditioner.properties_with_notch
    defaults = dict(pfa=0.001, p_c_factor=0.9, length=32, segments_est=12500, segments_reset=5000000, segments_coeff=0)
    assert r({"InputFilter": {"implementation": "Notch_Filter"}}) == dict(input_kind="gr_complex", inverted_spectrum=False, notch=defaults)
    kw = r({"DataTypeAdapter": {"implementation": "Ibyte_To_Complex", "inverted_spectrum": "true"},
            "InputFilter": {"implementation": "Notch_Filter", "pfa": 0.01, "p_c_factor": 0.8, "length": "64", "segments_est": 100, "segments_reset": 1000},
            "Resampler": {"implementation": "Direct_Resampler", "sample_freq_in": 25e6, "sample_freq_out": 4e6}})
    assert kw == dict(input_kind="ibyte", inverted_spectrum=True, fs_in=25e6, fs_out=4e6,
                      notch=dict(pfa=0.01, p_c_factor=0.8, length=64, segments_est=100, segments_reset=1000, segments_coeff=0))
    # Notch_Filter_Lite: n_segments_coeff = max(1, int((samp_freq / coeff_rate) / length)) in float32 (notch_filter_lite.cc:48-61)
    lite = lambda **f: r({"InputFilter": dict(implementation="Notch_Filter_Lite", **f)})["notch"]
    assert lite() == dict(defaults, segments_coeff=1)                                # (4e6 / 4e5) / 32 = 0.3125 -> 0 -> 1
    assert lite(length=2)["segments_coeff"] == int(np.float32(np.float32(4e6) / np.float32(np.float32(4e6) * np.float32(0.1))) / np.float32(2))
    assert lite(length=2)["segments_coeff"] in (4, 5)                                # 10 / 2 up to the float32 rounding of 0.1
    assert lite(coeff_rate=1000.0, length=16)["segments_coeff"] == 250
    assert lite(coeff_rate=1000.0, length=16, sampling_frequency=20e6)["segments_coeff"] == 1250
    assert lite(coeff_rate=3.0, length=7, sampling_frequency=1e6)["segments_coeff"] == int(np.float32(np.float32(1e6) / np.float32(3.0)) / np.float32(7))
    assert lite(coeff_rate=1e9)["segments_coeff"] == 1
    for role in ({"InputFilter": {"implementation": "Notch_Filter", "item_type": "cshort"}},
                 {"InputFilter": {"implementation": "Notch_Filter_Lite", "item_type": "cbyte"}},
                 {"InputFilter": {"implementation": "Notch_Filter_Lite", "coeff_rate": 0.0}},
                 {"InputFilter": {"implementation": "Notch_Filter"}, "Resampler": {"implementation": "Mmse_Resampler"}},
                 {"InputFilter": {"implementation": "Some_Other_Filter"}}):
        with pytest.raises(ValueError):
            r(role)
    # everything else is properties_with_mitigation()
    taps = [0.25, 0.5, 0.25]
    for role in ({}, {"DataTypeAdapter": {"implementation": "Ishort_To_Complex"}, "InputFilter": {"implementation": "Fir_Filter", "taps": taps}},
                 {"InputFilter": {"implementation": "Pulse_Blanking_Filter", "length": 16}}):
        assert r(role) == q(role)
    # the two older mappings still do not cover the notch roles
    for f in (p, q):
        for impl in ("Notch_Filter", "Notch_Filter_Lite"):
            with pytest.raises(ValueError):
                f({"InputFilter": {"implementation": impl}})
    with pytest.raises(ValueError):
        outputs_after(10, notch=dict(lenght=3))
    with pytest.raises(ValueError):
        outputs_after(10, notch=dict(length=3), blanking=dict(length=3))
    assert outputs_after(100, notch=None) == 100 and outputs_after(100, notch=dict(length=10)) == 90 and outputs_after(101, notch=dict(length=10)) == 100
