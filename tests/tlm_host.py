"""Host build of gnss-sdr_amd/csrc/viterbi_acs.h (tests/host/viterbi_acs_host.cc) for the tests: g++ -O2 -ffp-contract=off, as tests/kf_host.py builds
kalman_step.h.  The device compiles the same text with contraction off as well."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from gnss_sdr_amd._lib import TlmPageJob, TlmPageResult
from gnss_sdr_amd.telemetry import FRAME, job_table, unpack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=1)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="viterbi_acs_host_"), "libviterbi_acs_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "gnss-sdr_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "viterbi_acs_host.cc"), "-o", out], check=True)
    so = C.CDLL(out)
    so.gsh_test_tlm_run_jobs.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_uint64, C.POINTER(TlmPageJob), C.c_int, C.POINTER(TlmPageResult),
                                         C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    so.gsh_test_tlm_crc_bytes.argtypes = [C.c_char_p, C.c_int]
    so.gsh_test_tlm_crc_bytes.restype = C.c_uint32
    jb, rb = C.c_int(), C.c_int()
    assert so.gsh_test_tlm_sizes(C.byref(jb), C.byref(rb)) == 64
    assert (jb.value, rb.value) == (C.sizeof(TlmPageJob), C.sizeof(TlmPageResult))
    return so


class HostTelemetryDecoder:
    """the interface of gnss_sdr_amd.telemetry.TelemetryDecoder on the host build of the header"""

    def __init__(self, n_channels, metric="full"):
        self.n_channels, self.mode = n_channels, {"full": 0, "reference": 1}[metric]
        self.metrics = np.full(64 * n_channels, -1e7, np.float32)
        self.chain = np.zeros(n_channels, np.uint32)

    def channel_reset(self, channel):
        self.metrics[64 * channel:64 * channel + 64] = -1e7
        self.chain[channel] = 0

    def decode_pages(self, symbols, jobs):
        x = np.ascontiguousarray(symbols, np.float32)
        res = (TlmPageResult * max(1, len(jobs)))()
        rc = lib().gsh_test_tlm_run_jobs(self.mode, self.n_channels, x.ctypes.data_as(C.POINTER(C.c_float)), len(x), job_table(jobs), len(jobs), res,
                                         self.metrics.ctypes.data_as(C.POINTER(C.c_float)), self.chain.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0, f"job {rc - 1} fails a range check"
        out = []
        for j, r in zip(jobs, res):
            words = np.array(r.bits[:], np.uint32)
            out.append(dict(bits=unpack_bits(words, FRAME[j["frame_type"]]["info_bits"]), words=words, crc_register=int(r.crc_register), crc_ok=int(r.crc_ok)))
        return out
