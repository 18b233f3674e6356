"""CPU tests of the signal conditioner's boundary (gsh_cond_*, gnss_sdr_amd.conditioner): declarations, refusals that need no GPU, the mapping of
the reference's property names, and the host bookkeeping against a brute-force walk of the reference's phase accumulator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["gsh_cond_create", "gsh_cond_destroy", "gsh_cond_plan", "gsh_cond_bind", "gsh_cond_push", "gsh_cond_push_device",
                "gsh_cond_push_pinned_async", "gsh_cond_position", "gsh_cond_time_push"]


def test_header_declares_the_conditioner_and_the_abi_version_stays(gsh):
    from gnss_sdr_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and getattr(gsh, name, None) is not None, name
    assert re.search(r"\}\s*gsh_cond_conf\s*;", code)
    for field in ("input", "item_type", "inverted_spectrum", "n_taps", "taps", "decimation", "center_freq_hz", "sampling_freq_hz", "fs_in", "fs_out", "packed"):
        assert field in dict(_lib.CondConf._fields_), field
    assert C.sizeof(_lib.CondConf) == 96 and _lib.CondConf.packed.offset == 64 and _lib.CondConf.taps.offset == 16
    assert "#define GSH_ABI_VERSION 25" in src and gsh.gsh_abi_version() == 25


def test_null_handles_and_invalid_confs_are_refused_with_a_message(gsh):
    from gnss_sdr_amd import _lib
    from gnss_sdr_amd.conditioner import _conf
    from gnss_sdr_amd.sample_stream import PackedFormat
    n = C.c_uint64(0)
    assert gsh.gsh_cond_push(None, None, 0, None, None) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_cond_push_device(None, None, 0, None, None, None) == 1
    assert gsh.gsh_cond_push_pinned_async(None, None, 0, None, None) == 1
    assert gsh.gsh_cond_bind(None, None) == 1
    assert gsh.gsh_cond_position(None, C.byref(n), C.byref(n)) == 1
    assert gsh.gsh_cond_time_push(None, None, 1, 1, None) == 1
    gsh.gsh_cond_destroy(None)
    h = C.c_void_p()
    assert gsh.gsh_cond_create(0, None, C.byref(h)) == 1 and not h
    taps = np.ones(5, np.float32)
    nsr = PackedFormat.from_signal_source("Nsr_File_Signal_Source")
    bad = [
        ("real input without a filter", dict(input_kind="short"), b"real input without a filter"),
        ("a real packed family without a filter", dict(input_kind=nsr), b"real input without a filter"),
        ("inverted_spectrum on real input", dict(input_kind="byte", taps=taps, inverted_spectrum=True), b"inverted_spectrum"),
        ("decimation 0 .. 64", dict(taps=taps, decimation=65), b"decimation"),
        ("negative decimation", dict(taps=taps, decimation=-1), b"decimation"),
        ("decimation without a filter", dict(decimation=2), b"decimation"),
        ("too many taps", dict(taps=np.ones(1025, np.float32)), b"n_taps"),
        ("sampling frequency", dict(taps=taps, sampling_freq_hz=0.0), b"sampling frequency"),
        ("one rate missing", dict(fs_in=4e6), b"sample rates"),
        ("a negative rate", dict(fs_in=4e6, fs_out=-1.0), b"sample rates"),
        ("a ratio below 2^-32", dict(fs_in=1e12, fs_out=1.0), b"too extreme"),
        ("a bad packed format", dict(input_kind=PackedFormat(99), taps=taps), b""),
    ]
    for what, kw, text in bad:
        args = dict(input_kind="gr_complex", inverted_spectrum=False, taps=None, decimation=1, center_freq_hz=0.0, sampling_freq_hz=4e6, fs_in=0.0, fs_out=0.0)
        args.update(kw)
        c, _keep = _conf(**args)
        assert gsh.gsh_cond_create(0, C.byref(c), C.byref(h)) == 1 and not h, what   # GSH_ERR_INVALID before any device is touched
        assert text in gsh.gsh_last_error() and gsh.gsh_last_error() != b"", (what, gsh.gsh_last_error())
        assert gsh.gsh_cond_plan(C.byref(c), 100, C.byref(n)) == 1, what
    c = _lib.CondConf(input=7)
    assert gsh.gsh_cond_create(0, C.byref(c), C.byref(h)) == 1 and b"input" in gsh.gsh_last_error()
    c = _lib.CondConf(input=0, item_type=9)
    assert gsh.gsh_cond_create(0, C.byref(c), C.byref(h)) == 1 and b"item type" in gsh.gsh_last_error()
    c = _lib.CondConf(input=0, n_taps=3, decimation=1, sampling_freq_hz=1.0)   # taps announced, none given
    assert gsh.gsh_cond_create(0, C.byref(c), C.byref(h)) == 1 and b"taps" in gsh.gsh_last_error()


def test_property_names_of_the_reference_map_to_the_handle():
    from gnss_sdr_amd import SignalConditioner
    from gnss_sdr_amd.conditioner import SignalConditioner as same
    assert SignalConditioner is same
    taps = [0.25, 0.5, 0.25]
    p = SignalConditioner.properties
    assert p({}) == dict(input_kind="gr_complex", inverted_spectrum=False)
    assert p({"DataTypeAdapter": {"implementation": "Pass_Through", "item_type": "cshort"}}) == dict(input_kind="cshort", inverted_spectrum=False)
    kw = p({"DataTypeAdapter": {"implementation": "Ibyte_To_Complex", "inverted_spectrum": "true"},
            "InputFilter": {"implementation": "Freq_Xlating_Fir_Filter", "input_item_type": "gr_complex", "output_item_type": "gr_complex", "taps": taps,
                            "decimation_factor": 2, "IF": 1.2e6, "sampling_frequency": 8e6},
            "Resampler": {"implementation": "Direct_Resampler", "sample_freq_in": 4e6, "sample_freq_out": 2.5e6}})
    assert kw == dict(input_kind="ibyte", inverted_spectrum=True, taps=taps, decimation=2, center_freq_hz=1.2e6, sampling_freq_hz=8e6, fs_in=4e6, fs_out=2.5e6)
    kw = p({"DataTypeAdapter": {"implementation": "Ishort_To_Complex"}, "InputFilter": {"implementation": "Fir_Filter", "taps": taps, "decimation_factor": 4, "IF": 1e6}})
    # fir_filter_ccf: no translation, no decimation, whatever the role says; sampling_frequency defaults to 4 Msps (freq_xlating_fir_filter.cc:46)
    assert kw == dict(input_kind="ishort", inverted_spectrum=False, taps=taps, decimation=1, center_freq_hz=0.0, sampling_freq_hz=4e6)
    kw = p({"InputFilter": {"implementation": "Freq_Xlating_Fir_Filter", "input_item_type": "short", "taps": taps, "IF": 2e6},
            "Resampler": {"implementation": "Direct_Resampler", "sample_freq_out": 2e6}})
    assert kw["input_kind"] == "short" and (kw["fs_in"], kw["fs_out"]) == (4e6, 2e6)   # sample_freq_in defaults to 4 Msps (direct_resampler_conditioner.cc:52)
    for role in ({"InputFilter": {"implementation": "Pulse_Blanking_Filter"}}, {"InputFilter": {"implementation": "Notch_Filter"}},
                 {"InputFilter": {"implementation": "Notch_Filter_Lite"}}, {"DataTypeAdapter": {"implementation": "Byte_To_Short"}},
                 {"Resampler": {"implementation": "Mmse_Resampler"}}, {"InputFilter": {"implementation": "Fir_Filter"}},   # no taps
                 {"InputFilter": {"implementation": "Freq_Xlating_Fir_Filter", "taps": taps, "output_item_type": "cshort"}},
                 {"DataTypeAdapter": {"implementation": "Ibyte_To_Complex"}, "InputFilter": {"implementation": "Fir_Filter", "taps": taps, "input_item_type": "byte"}},
                 {"Resampler": {"implementation": "Direct_Resampler", "sample_freq_in": 4e6}}):
        with pytest.raises(ValueError):
            p(role)


def _walk(n_filter_outputs, fs_in, fs_out):
    """direct_resampler_conditioner_cc.cc:52-59,83-110 walked sample by sample over n_filter_outputs inputs: how many outputs it produces.
    (decimation: a sample is copied whenever the 32-bit accumulator wraps, sample 0 always; interpolation: the input advances on a wrap and
    the output that caused the wrap already reads the next sample)"""
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


@pytest.mark.parametrize("fs_in,fs_out", [(4e6, 2.5e6), (25e6, 4e6), (4e6, 4.092e6), (2e6, 6.5e6), (3e6, 3e6), (0.0, 0.0), (7e6, 1e6)])
@pytest.mark.parametrize("D", [1, 2, 8])
def test_host_bookkeeping_equals_a_walk_of_the_reference_accumulator(fs_in, fs_out, D):
    """every cut position of a short stream: the count after N inputs is the walk's count over the ceil(N / D) filter outputs those inputs complete, so
    any sequence of pushes that ends at N has produced exactly that many ring samples"""
    from gnss_sdr_amd.conditioner import outputs_after
    taps = [1.0, 2.0, 3.0] if D > 1 else None
    got = [outputs_after(n, "gr_complex", taps=taps, decimation=D, sampling_freq_hz=1.0, fs_in=fs_in, fs_out=fs_out) for n in range(0, 241)]
    want = []
    for n in range(0, 241):
        m = (n + D - 1) // D
        want.append(m if fs_in == fs_out else _walk(m, fs_in, fs_out))
    assert got == want
    assert all(b >= a for a, b in zip(got, got[1:]))
    # and far into a stream, against the closed forms of resampler.hip's header
    if fs_in > 0.0 and fs_in != fs_out:
        two_32 = 1 << 32
        n = 3_000_000_017
        m = (n + D - 1) // D
        c = outputs_after(n, "gr_complex", taps=taps, decimation=D, sampling_freq_hz=1.0, fs_in=fs_in, fs_out=fs_out)
        if fs_in > fs_out:
            step = int(np.floor(two_32 * fs_out / fs_in))
            index = lambda j: -((-j * two_32) // step)
        else:
            step = int(np.floor(two_32 * fs_in / fs_out))
            index = lambda j: ((j + 1) * step) >> 32
        assert index(c - 1) < m <= index(c)
