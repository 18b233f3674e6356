"""CPU tests of the beamformer's adaptive mode at the C boundary (gsh_adaptive_beam_set, gsh_adaptive_beam_state): the header's declarations, the structures'
sizes, and the refusals that need no GPU.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np

import aw_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSH_ERR_INVALID = 1


def _header():
    src = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_functions_and_the_structures():
    src = _header()
    assert re.search(r"int\s+gsh_adaptive_beam_set\s*\(\s*gsh_beam_t\s*\*\s*\w+\s*,\s*const\s+gsh_beam_adapt\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"int\s+gsh_adaptive_beam_state\s*\(\s*gsh_beam_t\s*\*\s*\w+\s*,\s*struct\s+gsh_beam_adapt_state\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"typedef\s+struct\s+gsh_beam_adapt\s*\{[^}]*forgetting[^}]*loading_rel[^}]*loading_abs[^}]*"
                     r"constraint_iq\s*\[GSH_ARRAY_MAX_BEAMS\]\s*\[GSH_ARRAY_MAX_ANTENNAS\]\s*\[2\][^}]*\}\s*gsh_beam_adapt\s*;", src)
    assert re.search(r"struct\s+gsh_beam_adapt_state\s*\{[^}]*blocks[^}]*failures[^}]*delta[^}]*r_acc_iq[^}]*w_iq[^}]*\}\s*;", src)
    assert re.search(r"#define\s+GSH_ABI_VERSION\s+25\b", src)      # entry points were added, nothing changed


def test_symbols_and_structure_sizes(gsh):
    from gnss_sdr_amd import _lib
    for name in ("gsh_adaptive_beam_set", "gsh_adaptive_beam_state"):
        assert name in _lib.SYMBOLS and getattr(gsh, name, None) is not None, name
    assert _lib.missing_symbols() == []
    assert gsh.gsh_abi_version() == 25
    host = aw_host.lib()
    assert C.sizeof(_lib.BeamAdapt) == host.gsh_test_beam_adapt_bytes() == 3 * 8 + 8 * 8 * 2 * 8
    assert C.sizeof(_lib.BeamAdaptState) == host.gsh_test_beam_adapt_state_bytes() == 3 * 8 + 8 * 8 * 2 * 8 + 8 * 8 * 2 * 4
    assert _lib.BeamAdapt.constraint_iq.offset == 24 and _lib.BeamAdaptState.r_acc_iq.offset == 24 and _lib.BeamAdaptState.w_iq.offset == 24 + 1024


def _conf(forgetting=0.5, loading_rel=1e-6, loading_abs=0.0, c=None):
    from gnss_sdr_amd import _lib
    conf = _lib.BeamAdapt(forgetting, loading_rel, loading_abs)
    full = np.zeros((8, 8), np.complex128)
    full[:, 0] = 1.0
    if c is not None:
        full[:] = c
    C.memmove(conf.constraint_iq, full.ctypes.data, full.nbytes)
    return conf


def test_null_handle_is_refused_without_a_gpu(gsh):
    from gnss_sdr_amd import _lib
    good = _conf()
    assert gsh.gsh_adaptive_beam_set(None, C.byref(good)) == GSH_ERR_INVALID
    assert b"null" in gsh.gsh_last_error()
    assert gsh.gsh_adaptive_beam_set(None, None) == GSH_ERR_INVALID
    assert b"null" in gsh.gsh_last_error()
    st = _lib.BeamAdaptState()
    assert gsh.gsh_adaptive_beam_state(None, C.byref(st)) == GSH_ERR_INVALID
    assert b"null" in gsh.gsh_last_error()


def _bad_numbers():
    nan, inf = float("nan"), float("inf")
    notfinite = np.zeros((8, 8), np.complex128)
    notfinite[:, 0] = 1.0
    notfinite[1, 2] = complex(0.0, nan)
    return [
        (_conf(forgetting=-0.01), "forgetting"), (_conf(forgetting=1.01), "forgetting"), (_conf(forgetting=nan), "finite"), (_conf(forgetting=-inf), "finite"),
        (_conf(loading_rel=-1e-9), "negative loading"), (_conf(loading_abs=-1.0), "negative loading"), (_conf(loading_rel=nan), "finite"),
        (_conf(loading_abs=inf), "finite"), (_conf(c=notfinite), "finite"),
    ]


def test_invalid_numbers_are_refused_without_a_gpu(gsh):
    """what the numbers alone show is refused before the handle is looked at: the refusal names the number, with no handle and no device at all
    (an all-zero constraint vector is one of a beam the handle forms: tests/test_beam_adaptive_gpu.py, where a handle can be created)"""
    for conf, word in _bad_numbers():
        assert gsh.gsh_adaptive_beam_set(None, C.byref(conf)) == GSH_ERR_INVALID, word
        assert word.encode() in gsh.gsh_last_error() and b"null" not in gsh.gsh_last_error(), (word, gsh.gsh_last_error())
