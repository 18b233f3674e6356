"""The Kalman loop's two entry points (gsh_trk_set_kalman, gsh_trk_kf_state) as the header declares them, and the two code objects behind them."""
import ctypes as C
import os
import re

import pytest

import gnss_sdr_amd
from gnss_sdr_amd import _lib
from kernel_metadata import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_two_functions_and_the_conf():
    h = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    assert re.search(r"int gsh_trk_set_kalman\(gsh_trk_t\* t, const gsh_trk_kf_conf\* kf\);", h)
    assert re.search(r"int gsh_trk_kf_state\(gsh_trk_t\* t, int channel, double x\[4\], double P\[16\], double R\[2\]\);", h)
    assert "} gsh_trk_kf_conf;" in h
    assert "#define GSH_ABI_VERSION 25" in h
    assert "gsh_trk_set_kalman" in _lib.SYMBOLS and "gsh_trk_kf_state" in _lib.SYMBOLS


def test_conf_is_ten_doubles_with_kf_confs_defaults():
    from gnss_sdr_amd.tracking_loop import kf_conf
    assert C.sizeof(_lib.TrkKfConf) == 80
    k = kf_conf()
    assert [getattr(k, n) for n, _ in _lib.TrkKfConf._fields_] == [0.2, 0.3, 0.15, 0.25, 0.6, 0.01, 0.5, 0.7, 5.0, 1.0]
    assert kf_conf(carrier_freq_sd_hz=1.5).carrier_freq_sd_hz == 1.5


def test_null_handle_is_refused_without_a_gpu():
    from gnss_sdr_amd.tracking_loop import kf_conf
    lib = _lib.load()
    k = kf_conf()
    assert lib.gsh_trk_set_kalman(None, C.byref(k)) == 1  # GSH_ERR_INVALID
    assert b"null" in lib.gsh_last_error()
    assert lib.gsh_trk_kf_state(None, 0, None, None, None) == 1


def test_exactly_two_kalman_flavours_of_the_loop_kernel():
    lib = gnss_sdr_amd._lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("library not built")
    loop = [n for n in kernels(lib) if "trk_loop_kernel" in n]
    # trk_loop_kernel<NT, HD, LIVE, COOP, KF>: the Kalman flavours are <3 | 5, false, false, false, true>
    kf = sorted(n for n in loop if re.search(r"trk_loop_kernelILi\dELb[01]ELb[01]ELb[01]ELb1EE", n))
    assert len(kf) == 2 and all("ELb0ELb0ELb0ELb1EE" in n for n in kf) and "ILi3E" in kf[0] and "ILi5E" in kf[1], kf
    assert len(loop) == 12
