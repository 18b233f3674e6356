"""CPU tests of the antenna-array entry points (gsh_beam_*, include/gnss_sdr_hip.h): the header's constants, the 16-byte format structure and the
refusals that need no GPU.  No kernel runs here."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSH_ERR_INVALID = 1


def _header():
    return open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()


def test_header_constants_match_the_python_face():
    from gnss_sdr_amd import _lib
    src = _header()
    defs = dict(re.findall(r"#define\s+(GSH_ARRAY_[A-Z_]+)\s+(\d+)", src))
    assert defs == {"GSH_ARRAY_MAX_ANTENNAS": "8", "GSH_ARRAY_MAX_BEAMS": "8", "GSH_ARRAY_PLANAR": "0", "GSH_ARRAY_INTERLEAVED": "1"}
    assert (_lib.GSH_ARRAY_MAX_ANTENNAS, _lib.GSH_ARRAY_MAX_BEAMS, _lib.GSH_ARRAY_PLANAR, _lib.GSH_ARRAY_INTERLEAVED) == (8, 8, 0, 1)
    assert re.search(r"#define\s+GSH_ABI_VERSION\s+25\b", src)      # entry points were added, nothing changed


def test_array_format_is_sixteen_bytes():
    from gnss_sdr_amd._lib import ArrayFormat
    assert C.sizeof(ArrayFormat) == 16
    assert [(n, getattr(ArrayFormat, n).offset) for n, _ in ArrayFormat._fields_] == [("n_antennas", 0), ("item_type", 4), ("layout", 8), ("first_is_q", 12)]
    from gnss_sdr_amd.array import ArrayFormat as Fmt
    s = Fmt(3, "ishort", "interleaved", first_is_q=True).struct()
    assert (s.n_antennas, s.item_type, s.layout, s.first_is_q) == (3, 1, 1, 1)
    assert Fmt(3, "ishort", "interleaved").n_buffers == 1 and Fmt(3, "ibyte").n_buffers == 3 and Fmt(2, "gr_complex").item_bytes == 8


def test_every_beam_symbol_is_exported(gsh):
    from gnss_sdr_amd import _lib
    names = [n for n in _lib.SYMBOLS if n.startswith("gsh_beam_")]
    assert sorted(names) == sorted(["gsh_beam_create", "gsh_beam_destroy", "gsh_beam_set_weights", "gsh_beam_get_weights", "gsh_beam_process_device",
                                    "gsh_beam_push", "gsh_beam_push_device", "gsh_beam_covariance", "gsh_beam_covariance_device", "gsh_beam_time_process"])
    for n in names:
        assert getattr(gsh, n, None) is not None, n


def _refused(gsh, rc, *words):
    assert rc == GSH_ERR_INVALID
    text = gsh.gsh_last_error().decode()
    assert text and all(w in text for w in words), text


def test_refusals_that_need_no_gpu(gsh):
    from gnss_sdr_amd._lib import ArrayFormat
    h = C.c_void_p()
    good = ArrayFormat(4, 0, 0, 0)
    _refused(gsh, gsh.gsh_beam_create(0, None, 1, C.byref(h)), "null")
    _refused(gsh, gsh.gsh_beam_create(0, C.byref(good), 1, None), "null")
    for A in (0, 9, -1):
        f = ArrayFormat(A, 0, 0, 0)
        _refused(gsh, gsh.gsh_beam_create(0, C.byref(f), 1, C.byref(h)), "antennas")
    for B in (0, 9, -3):
        _refused(gsh, gsh.gsh_beam_create(0, C.byref(good), B, C.byref(h)), "beams")
    for item in (3, -1):
        f = ArrayFormat(4, item, 0, 0)
        _refused(gsh, gsh.gsh_beam_create(0, C.byref(f), 1, C.byref(h)), "item type")
    for layout in (2, -1):
        f = ArrayFormat(4, 0, layout, 0)
        _refused(gsh, gsh.gsh_beam_create(0, C.byref(f), 1, C.byref(h)), "layout")
    assert not h.value
    # a null handle
    w = (C.c_float * 2)(1.0, 0.0)
    r = (C.c_double * 2)()
    ms = C.c_float(0.0)
    one = (C.c_void_p * 1)(None)
    first = (C.c_uint64 * 1)()
    _refused(gsh, gsh.gsh_beam_set_weights(None, w), "null")
    _refused(gsh, gsh.gsh_beam_get_weights(None, w), "null")
    _refused(gsh, gsh.gsh_beam_process_device(None, one, 1, 0, one, None), "null")
    _refused(gsh, gsh.gsh_beam_push(None, one, one, 1, 0, first), "null")
    _refused(gsh, gsh.gsh_beam_push_device(None, one, one, 1, 0, None, first), "null")
    _refused(gsh, gsh.gsh_beam_covariance(None, one, 1, 0, r), "null")
    _refused(gsh, gsh.gsh_beam_covariance_device(None, one, 1, 0, r), "null")
    _refused(gsh, gsh.gsh_beam_time_process(None, 1024, 1, C.byref(ms)), "null")
    gsh.gsh_beam_destroy(None)    # a no-op


def test_python_face_has_no_cpu_fallback(gsh):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.array import ArrayFormat, Beamformer
    if gsh.gsh_device_count() > 0:
        Beamformer(ArrayFormat(4), 2).close()
    else:
        with pytest.raises(GshError) as e:
            Beamformer(ArrayFormat(4), 2)
        assert e.value.code == 2  # GSH_ERR_NO_DEVICE
    with pytest.raises(GshError) as e:
        Beamformer(ArrayFormat(9), 2)
    assert e.value.code == 1
