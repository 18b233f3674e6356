"""CPU tests of the signal generator's boundary (gsh_gen_*, gnss_sdr_amd.signal_generator): declarations, every refusal that needs no GPU, and the
noise's Philox4x32-10 word stage -- the text the kernel runs (csrc/signal_generator.h), called on the host through gsh_gen_philox_words -- against a
numpy restatement of the published round function (tests/siggen_reference.py) and the known answers of the Random123 distribution."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import siggen_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["gsh_gen_create", "gsh_gen_destroy", "gsh_gen_set_satellite", "gsh_gen_check_satellite", "gsh_gen_set_noise", "gsh_gen_seek",
                "gsh_gen_position", "gsh_gen_generate_device", "gsh_gen_push", "gsh_gen_time_generate", "gsh_gen_philox_words"]


def test_header_declares_the_generator_and_the_abi_version_stays(gsh):
    from gnss_sdr_amd import _lib
    src = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and getattr(gsh, name, None) is not None, name
    assert re.search(r"#define\s+GSH_GEN_MAX_SATS\s+32\b", code) and re.search(r"#define\s+GSH_GEN_MAX_SIGNS\s+1024\b", code)
    assert re.search(r"typedef\s+struct\s+gsh_gen\s+gsh_gen_t\s*;", code)
    # the group cites its reference block as the other groups do
    assert "signal_generator_c.h" in src and "sg.cc:362-383" in src and "sg.cc:540-546" in src
    # declared signatures: the argument counts of the prototypes and of the ctypes table agree
    for name in ENTRY_POINTS:
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert len([a for a in proto.split(",") if a.strip() and a.strip() != "void"]) == len(_lib.SYMBOLS[name][1]), name
    assert "#define GSH_ABI_VERSION 25" in src and gsh.gsh_abi_version() == 25      # entry points were added, nothing changed


def test_null_handles_are_refused(gsh):
    n = C.c_uint64(0)
    ms = C.c_float(0)
    one = (C.c_int8 * 1)(1)
    tab = (C.c_float * 2)(1.0, 0.0)
    assert gsh.gsh_gen_set_satellite(None, 0, tab, None, 1, 0, one, 1, None, 0, 0.0, 0.0, 0.0) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_gen_set_noise(None, 1, 5) == 1
    assert gsh.gsh_gen_seek(None, 0) == 1
    assert gsh.gsh_gen_position(None, C.byref(n)) == 1
    assert gsh.gsh_gen_generate_device(None, 1, None) == 1
    assert gsh.gsh_gen_push(None, None, 1, None) == 1
    assert gsh.gsh_gen_time_generate(None, 1, 1, C.byref(ms)) == 1 and b"null" in gsh.gsh_last_error()
    gsh.gsh_gen_destroy(None)
    assert gsh.gsh_gen_create(0, 4e6, 1, None) == 1


def test_create_refuses_before_any_device_is_touched(gsh):
    h = C.c_void_p()
    for n_sats in (0, -1, 33):
        assert gsh.gsh_gen_create(0, 4e6, n_sats, C.byref(h)) == 1 and not h and b"n_sats" in gsh.gsh_last_error(), n_sats
    for fs in (0.0, -4e6, float("nan"), float("inf")):
        assert gsh.gsh_gen_create(0, fs, 1, C.byref(h)) == 1 and not h and b"sample rate" in gsh.gsh_last_error(), fs


def test_every_bad_satellite_is_refused_with_a_message(gsh):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.signal_generator import Satellite, check_satellite
    tab = np.ones(8, np.complex64)
    ok = dict(table_a=tab, table_b=tab, delay_samples=3, signs_a=np.array([1, -1], np.int8), signs_b=np.ones(5, np.int8), doppler_hz=100.0,
              start_phase_rad=0.5, carrier_offset_hz=0.0)
    check_satellite(4e6, Satellite(**ok))
    check_satellite(4e6, Satellite(**dict(ok, table_b=None, signs_b=np.zeros(0, np.int8))))    # without B its signs are not read
    check_satellite(4e6, Satellite(**dict(ok, delay_samples=7, signs_a=np.ones(1024, np.int8))))
    nan_tab = tab.copy()
    nan_tab[5] = complex(0.0, float("nan"))
    bad = [
        ("delay_samples == period", dict(delay_samples=8), "delay_samples"),
        ("a Doppler that is not finite", dict(doppler_hz=float("nan")), "Doppler"),
        ("an infinite Doppler", dict(doppler_hz=float("inf")), "Doppler"),
        ("a start phase that is not finite", dict(start_phase_rad=float("inf")), "start phase"),
        ("a carrier offset that is not finite", dict(carrier_offset_hz=float("nan")), "carrier offset"),
        ("a table value that is not finite", dict(table_a=nan_tab), "table A"),
        ("a table B value that is not finite", dict(table_b=nan_tab), "table B"),
        ("a sign byte 0", dict(signs_a=np.array([1, 0, -1], np.int8)), "sign sequence A"),
        ("a sign byte 2", dict(signs_b=np.array([2], np.int8)), "sign sequence B"),
        ("an empty sign sequence", dict(signs_a=np.zeros(0, np.int8)), "sign sequence A"),
        ("a sign sequence of 1025", dict(signs_a=np.ones(1025, np.int8)), "sign sequence A"),
        ("an empty sign sequence B with a table B", dict(signs_b=np.zeros(0, np.int8)), "sign sequence B"),
    ]
    for what, kw, text in bad:
        with pytest.raises(GshError) as e:
            check_satellite(4e6, Satellite(**dict(ok, **kw)))
        assert e.value.code == 1 and text in str(e.value) and str(e.value), (what, str(e.value))
    one = (C.c_int8 * 1)(1)
    raw = (C.c_float * 2)(1.0, 0.0)
    assert gsh.gsh_gen_check_satellite(4e6, raw, None, 0, 0, one, 1, None, 0, 0.0, 0.0, 0.0) == 1 and b"period 0 below 1" in gsh.gsh_last_error()
    assert gsh.gsh_gen_check_satellite(4e6, raw, None, 1, 1, one, 1, None, 0, 0.0, 0.0, 0.0) == 1 and b"delay_samples" in gsh.gsh_last_error()
    assert gsh.gsh_gen_check_satellite(4e6, None, None, 1, 0, one, 1, None, 0, 0.0, 0.0, 0.0) == 1 and b"null table A" in gsh.gsh_last_error()
    assert gsh.gsh_gen_check_satellite(4e6, raw, None, 1, 0, None, 1, None, 0, 0.0, 0.0, 0.0) == 1 and b"null sign" in gsh.gsh_last_error()
    assert gsh.gsh_gen_check_satellite(4e6, raw, None, 1, 0, one, 1, None, 0, 0.0, 0.0, 0.0) == 0
    with pytest.raises(GshError) as e:
        check_satellite(float("nan"), Satellite(**ok))
    assert e.value.code == 1 and "sample rate" in str(e.value)


def test_python_face_is_exported():
    import gnss_sdr_amd
    from gnss_sdr_amd import signal_generator as SG
    assert gnss_sdr_amd.SignalGenerator is SG.SignalGenerator
    for name in ("Satellite", "gps_l1_ca_satellite", "galileo_e5a_satellite", "cn0_scale", "check_satellite", "philox_words"):
        assert hasattr(SG, name), name


# Random123's kat_vectors for philox4x32-10: (counter, key) -> words
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_numpy_restatement_gives_the_published_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = R.philox4x32_10(*[np.array([c], np.uint64) for c in ctr], *key)
        assert tuple(int(w[0]) for w in got) == want, (ctr, key)


def test_philox_word_stage_of_the_shared_header_equals_the_published_round_function():
    from gnss_sdr_amd.signal_generator import philox_words
    assert tuple(int(w) for w in philox_words(0, 0)) == KNOWN_ANSWERS[0][2]        # counter 0, key 0: the first known answer
    rng = np.random.default_rng(20131)
    counters = [0, 1, 2 ** 32 - 1, 2 ** 32, int(rng.integers(0, 2 ** 63)) * 2 + 1, 2 ** 40 + 1]
    seeds = [0, 1, 0xFFFFFFFF, 2 ** 32, int(rng.integers(0, 2 ** 63)) * 2 + 1]
    for seed in seeds:
        for n in counters:
            want = R.philox4x32_10(np.array([n & 0xFFFFFFFF], np.uint64), np.array([n >> 32], np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64),
                                   seed & 0xFFFFFFFF, seed >> 32)
            assert [int(w) for w in philox_words(seed, n)] == [int(w[0]) for w in want], (seed, n)
    # and the vectorised word stage the GPU tests use
    w = R.noise_words(seeds[4], 2 ** 32 - 3, 6)
    for i in range(6):
        assert [int(x[i]) for x in w] == [int(x) for x in philox_words(seeds[4], 2 ** 32 - 3 + i)]
