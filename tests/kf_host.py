"""Host build of gnss-sdr_amd/csrc/kalman_step.h (tests/host/kalman_step_host.cc) for the tests: g++ -O2 -ffp-contract=off, as tests/test_exact_division.py builds
exact_division.h.  The device compiles the same text with contraction off as well, so a step replayed here from the same inputs is the device's, bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KF_DEFAULT_SD = (0.2, 0.3, 0.15, 0.25, 0.6, 0.01, 0.5, 0.7, 5.0, 1.0)  # Kf_Conf, kf_conf.cc:39-48, in gsh_trk_kf_conf's order


class KfState(C.Structure):
    """gsh::KfState"""
    _fields_ = [("x", C.c_double * 4), ("P", C.c_double * 16), ("Q", C.c_double * 16), ("R", C.c_double * 2), ("Ti", C.c_double), ("beta", C.c_double),
                ("code_error_kf_chips", C.c_double), ("pad_", C.c_double)]

    def arrays(self):
        return np.array(self.x[:]), np.array(self.P[:]).reshape(4, 4), np.array(self.Q[:]).reshape(4, 4), np.array(self.R[:])


@functools.lru_cache(maxsize=1)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="kalman_step_host_"), "libkalman_step_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "gnss-sdr_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "kalman_step_host.cc"), "-o", out], check=True)
    so = C.CDLL(out)
    sp = C.POINTER(KfState)
    so.gsh_test_kf_state_bytes.restype = C.c_int
    so.gsh_test_kf_init.argtypes = [sp, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
    so.gsh_test_kf_init.restype = None
    so.gsh_test_kf_run.argtypes = [sp, C.c_double, C.c_double]
    so.gsh_test_kf_run.restype = C.c_double
    so.gsh_test_kf_narrow.argtypes = [sp, C.c_int, C.c_double, C.c_float, C.c_double]
    so.gsh_test_kf_narrow.restype = None
    so.gsh_test_kf_cn0.argtypes = [sp, C.c_float, C.c_double]
    so.gsh_test_kf_cn0.restype = None
    so.gsh_test_kf_exp10.argtypes = [C.c_double]
    so.gsh_test_kf_exp10.restype = C.c_double
    assert so.gsh_test_kf_state_bytes() == C.sizeof(KfState)
    return so


class HostKalman:
    """One channel's filter on the host build of the header."""

    def __init__(self, Ti, acq_doppler_hz, sd=KF_DEFAULT_SD, code_chip_rate=1.023e6, signal_carrier_freq=1575.42e6, acq_code_phase_chips=0.0):
        self._lib = lib()
        self.s = KfState()
        self._lib.gsh_test_kf_init(C.byref(self.s), (C.c_double * 10)(*sd), code_chip_rate, signal_carrier_freq, Ti, acq_code_phase_chips, acq_doppler_hz)

    def run(self, code_disc_chips, carr_disc_hz):
        return self._lib.gsh_test_kf_run(C.byref(self.s), float(code_disc_chips), float(carr_disc_hz))

    def narrow(self, extend, Ti_new, spc, cn0_dbhz):
        self._lib.gsh_test_kf_narrow(C.byref(self.s), int(extend), float(Ti_new), float(spc), float(cn0_dbhz))

    def cn0(self, spc, cn0_dbhz):
        self._lib.gsh_test_kf_cn0(C.byref(self.s), float(spc), float(cn0_dbhz))

    def set_R(self, R):
        self.s.R[0], self.s.R[1] = float(R[0]), float(R[1])

    @property
    def x(self):
        return np.array(self.s.x[:])

    @property
    def P(self):
        return np.array(self.s.P[:]).reshape(4, 4)

    @property
    def R(self):
        return np.array(self.s.R[:])
