"""The telemetry entry points (gsh_tlm_*) as the header declares them, their ctypes bindings, and the range errors, which are returned on the host
alone: no device is touched before every job of a table has passed."""
import ctypes as C
import os
import re

import pytest

from gnss_sdr_amd import _lib
from gnss_sdr_amd.telemetry import job_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gsh_tlm_create", "gsh_tlm_destroy", "gsh_tlm_channel_reset", "gsh_tlm_check_jobs", "gsh_tlm_preamble_scan", "gsh_tlm_decode_pages",
                "gsh_tlm_decode_pages_device", "gsh_tlm_time_decode_pages"]


def test_header_declares_the_entry_points_and_structs():
    h = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    assert "#define GSH_ABI_VERSION 25" in h
    assert re.search(r"int gsh_tlm_create\(int device, int n_channels, int metric_mode, gsh_tlm_t\*\* out\);", h)
    assert re.search(r"void gsh_tlm_destroy\(gsh_tlm_t\* h\);", h)
    assert re.search(r"int gsh_tlm_channel_reset\(gsh_tlm_t\* h, int channel\);", h)
    assert re.search(r"int gsh_tlm_preamble_scan\(gsh_tlm_t\* h, int frame_type, const float\* symbols, uint64_t n, int8_t\* corr_out\);", h)
    assert re.search(r"int gsh_tlm_decode_pages\(gsh_tlm_t\* h, const float\* symbols, uint64_t n_symbols, const gsh_tlm_page_job\* jobs, int n_jobs, "
                     r"gsh_tlm_page_result\* results\);", h)
    assert re.search(r"int gsh_tlm_decode_pages_device\(gsh_tlm_t\* h, const void\* device_symbols, uint64_t n_symbols,", h)
    assert "} gsh_tlm_page_job;" in h and "} gsh_tlm_page_result;" in h
    assert "#define GSH_TLM_METRIC_FULL 0" in h and "#define GSH_TLM_METRIC_REFERENCE 1" in h
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS, name
    section = h[h.index("Galileo telemetry pages"):]   # the entry points cite the reference lines they replace
    for cite in ("viterbi_decoder.cc:47-120", ":352-361", ":371-377", ":962-972", ":364-560", ":1040-1046", "galileo_inav_message.cc:146-177"):
        assert cite in section, cite


def test_struct_layouts():
    assert C.sizeof(_lib.TlmPageJob) == 32 and _lib.TlmPageJob.symbol_offset.offset == 8 and _lib.TlmPageJob.flags.offset == 16
    assert C.sizeof(_lib.TlmPageResult) == 72 and _lib.TlmPageResult.crc_register.offset == 64 and _lib.TlmPageResult.crc_ok.offset == 68
    assert (_lib.GSH_TLM_JOB_INVERT, _lib.GSH_TLM_JOB_CRC_CONTINUE, _lib.GSH_TLM_JOB_INAV_AUTO) == (1, 2, 4)


def test_library_exports_the_entry_points(gsh):
    assert gsh.gsh_abi_version() == 25
    for name in ENTRY_POINTS:
        assert getattr(gsh, name, None) is not None, name


GOOD = dict(channel=1, frame_type=2, symbol_offset=12, crc_bits=214, crc_check=1)
BAD = {
    "window leaves the buffer": dict(GOOD, symbol_offset=13),
    "offset beyond the buffer": dict(GOOD, symbol_offset=1 << 40),
    "unknown frame type 0": dict(GOOD, frame_type=0),
    "unknown frame type 4": dict(GOOD, frame_type=4),
    "channel = n_channels": dict(GOOD, channel=2),
    "negative channel": dict(GOOD, channel=-1),
    "crc_bits + 24 beyond the page": dict(GOOD, crc_bits=215),
    "crc_bits beyond the page": dict(GOOD, crc_bits=239, crc_check=0),
    "negative crc_bits": dict(GOOD, crc_bits=-1),
    "unknown flag": dict(GOOD, flags=8),
    "I/NAV flag on F/NAV": dict(GOOD, flags=4),
}


def test_range_errors_are_returned_without_a_device(gsh):
    n_symbols = 12 + 488
    assert gsh.gsh_tlm_check_jobs(2, n_symbols, job_table([GOOD]), 1) == 0
    assert gsh.gsh_tlm_check_jobs(2, n_symbols, job_table([dict(GOOD, crc_bits=238, crc_check=0)]), 1) == 0  # the whole page, nothing compared
    assert gsh.gsh_tlm_check_jobs(2, 250, job_table([dict(channel=0, frame_type=1, symbol_offset=10, flags=4)]), 1) == 0
    for why, job in BAD.items():
        assert gsh.gsh_tlm_check_jobs(2, n_symbols, job_table([GOOD, job]), 2) == 1, why  # GSH_ERR_INVALID
        assert b"job 1" in gsh.gsh_last_error(), why
    h = C.c_void_p()
    assert gsh.gsh_tlm_create(0, 0, 0, C.byref(h)) == 1 and not h
    assert gsh.gsh_tlm_create(0, 1, 2, C.byref(h)) == 1 and b"metric" in gsh.gsh_last_error()
    assert gsh.gsh_tlm_create(0, 1, 0, None) == 1
    res = (_lib.TlmPageResult * 1)()
    assert gsh.gsh_tlm_decode_pages(None, None, 0, job_table([GOOD]), 1, res) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_tlm_decode_pages_device(None, None, 0, job_table([GOOD]), 1, res) == 1
    assert gsh.gsh_tlm_preamble_scan(None, 1, None, 0, None) == 1
    assert gsh.gsh_tlm_channel_reset(None, 0) == 1
    gsh.gsh_tlm_destroy(None)


@pytest.mark.gpu
def test_range_errors_of_a_live_handle_launch_nothing(gsh, gpu):
    import numpy as np
    h = C.c_void_p()
    assert gsh.gsh_tlm_create(gpu, 2, 0, C.byref(h)) == 0
    try:
        x = np.ones(500, np.float32)
        res = (_lib.TlmPageResult * 2)()
        for why, job in BAD.items():
            assert gsh.gsh_tlm_decode_pages(h, _lib.fptr(x), len(x), job_table([GOOD, job]), 2, res) == 1, why
        assert gsh.gsh_tlm_channel_reset(h, 2) == 1 and gsh.gsh_tlm_preamble_scan(h, 0, _lib.fptr(x), len(x), None) == 1
        assert all(w == 0 for w in res[0].bits)  # nothing was written
    finally:
        gsh.gsh_tlm_destroy(h)
