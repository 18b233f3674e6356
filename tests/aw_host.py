"""Host build of gnss-sdr_amd/csrc/array_weights.h (tests/host/array_weights_host.cc) for the tests: g++ -O2 -ffp-contract=off, as tests/kf_host.py builds
kalman_step.h.  The device compiles the same text with contraction off as well, so a call replayed here from the same block covariance is the device's,
bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AW_MAX = 8
AW_PAIRS = AW_MAX * (AW_MAX + 1) // 2


class AwState(C.Structure):
    """gsh::AwState"""
    _fields_ = [("r_acc", C.c_double * (2 * AW_PAIRS)), ("delta", C.c_double), ("blocks", C.c_uint64), ("failures", C.c_uint64), ("solved", C.c_uint64),
                ("w", C.c_float * 2 * AW_MAX * AW_MAX)]


class AwConf(C.Structure):
    """gsh::AwConf"""
    _fields_ = [("forgetting", C.c_double), ("loading_rel", C.c_double), ("loading_abs", C.c_double), ("c", C.c_double * 2 * AW_MAX * AW_MAX),
                ("fixed_w", C.c_float * 2 * AW_MAX * AW_MAX)]


@functools.lru_cache(maxsize=1)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="array_weights_host_"), "libarray_weights_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "gnss-sdr_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "array_weights_host.cc"), "-o", out], check=True)
    so = C.CDLL(out)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    for name in ("gsh_test_aw_state_bytes", "gsh_test_aw_conf_bytes", "gsh_test_beam_adapt_bytes", "gsh_test_beam_adapt_state_bytes"):
        getattr(so, name).restype = C.c_int
    so.gsh_test_aw_accumulate.argtypes = [C.c_int, C.c_double, dp, dp]
    so.gsh_test_aw_accumulate.restype = None
    so.gsh_test_aw_weights.argtypes = [C.c_int, dp, C.c_double, C.c_double, dp, dp, dp, fp]
    so.gsh_test_aw_weights.restype = C.c_int
    so.gsh_test_aw_step.argtypes = [C.c_int, C.c_int, C.POINTER(AwConf), dp, C.c_int, C.POINTER(AwState)]
    so.gsh_test_aw_step.restype = C.c_int
    assert so.gsh_test_aw_state_bytes() == C.sizeof(AwState) and so.gsh_test_aw_conf_bytes() == C.sizeof(AwConf)
    return so


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def upper(R) -> np.ndarray:
    """complex [A, A] -> the upper triangle row by row as float64 (re, im) pairs, the layout of gsh::AwState::r_acc"""
    R = np.asarray(R, np.complex128)
    A = R.shape[0]
    flat = np.array([R[i, j] for i in range(A) for j in range(i, A)], np.complex128)
    return np.ascontiguousarray(flat.view(np.float64))


def full(up, A: int) -> np.ndarray:
    """the inverse of upper(): complex128 [A, A], the lower triangle the conjugate of the upper (as gsh_beam_covariance returns R)"""
    z = np.asarray(up, np.float64)[:A * (A + 1)].view(np.complex128)
    R = np.zeros((A, A), np.complex128)
    p = 0
    for i in range(A):
        for j in range(i, A):
            R[i, j] = z[p]
            if j != i:
                R[j, i] = np.conj(z[p])
            p += 1
    return R


def accumulate(A: int, lam: float, block_upper: np.ndarray, acc_upper: np.ndarray) -> np.ndarray:
    acc = np.array(acc_upper, np.float64)
    lib().gsh_test_aw_accumulate(A, float(lam), _dp(np.ascontiguousarray(block_upper, np.float64)), _dp(acc))
    return acc


def weights(R, c, loading_rel=0.0, loading_abs=0.0, w_in=None):
    """One beam from the covariance R (complex [A, A]; its upper triangle is used) -> (ok, delta, v complex128 [A], w complex64 [A]);
    w starts as w_in and is written only when the solve succeeds."""
    A = np.asarray(R).shape[0]
    acc = upper(R)
    cc = np.ascontiguousarray(np.asarray(c, np.complex128).reshape(A))
    v = np.zeros(A, np.complex128)
    w = np.array(np.zeros(A) if w_in is None else w_in, np.complex64)
    delta = C.c_double(0.0)
    ok = lib().gsh_test_aw_weights(A, _dp(acc), float(loading_rel), float(loading_abs), _dp(cc.view(np.float64)), C.byref(delta), _dp(v.view(np.float64)),
                                   w.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)))
    return bool(ok), float(delta.value), v, w


class HostAdaptive:
    """The state of an adaptive beamformer handle replayed on the host build of the header: step(R_block) is one adaptive call."""

    def __init__(self, A: int, n_beams: int, constraints, fixed_w, forgetting=0.0, loading_rel=0.0, loading_abs=0.0):
        self._lib = lib()
        self.A, self.n_beams = A, n_beams
        self.conf = AwConf(float(forgetting), float(loading_rel), float(loading_abs))
        c = np.zeros((AW_MAX, AW_MAX), np.complex128)
        c[:n_beams, :A] = np.asarray(constraints, np.complex128)   # one vector for every beam, or one per beam
        C.memmove(self.conf.c, c.ctypes.data, c.nbytes)
        self.set_fixed(fixed_w)
        self.s = AwState()
        self.reset = True
        w0 = np.zeros((AW_MAX, AW_MAX), np.complex64)   # until the first call the caller's weights are in force
        w0[:n_beams, :A] = np.asarray(fixed_w, np.complex64).reshape(n_beams, A)
        C.memmove(self.s.w, w0.ctypes.data, w0.nbytes)

    def set_fixed(self, fixed_w):
        w = np.ones((AW_MAX, AW_MAX), np.complex64)
        w[:self.n_beams, :self.A] = np.asarray(fixed_w, np.complex64).reshape(self.n_beams, self.A)
        C.memmove(self.conf.fixed_w, w.ctypes.data, w.nbytes)

    def step(self, R_block) -> bool:
        ok = self._lib.gsh_test_aw_step(self.A, self.n_beams, C.byref(self.conf), _dp(upper(R_block)), int(self.reset), C.byref(self.s))
        self.reset = False
        return bool(ok)

    def state(self) -> dict:
        """as array.Beamformer.adaptive_state()"""
        A = self.A
        w = np.frombuffer(self.s.w, np.float32).copy().view(np.complex64).reshape(AW_MAX, AW_MAX)[:self.n_beams, :A].copy()
        return dict(blocks=int(self.s.blocks), failures=int(self.s.failures), delta=float(self.s.delta),
                    r_acc=full(np.frombuffer(self.s.r_acc, np.float64).copy(), A), weights=w)


def same_state(a: dict, b: dict) -> bool:
    """bit equality of two adaptive states"""
    return (a["blocks"], a["failures"]) == (b["blocks"], b["failures"]) and np.float64(a["delta"]).tobytes() == np.float64(b["delta"]).tobytes() \
        and a["r_acc"].tobytes() == b["r_acc"].tobytes() and a["weights"].tobytes() == b["weights"].tobytes()
