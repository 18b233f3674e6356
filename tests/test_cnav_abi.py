"""The GPS CNAV entry points (gsh_cnav_*) as the header declares them, their ctypes bindings, and the range errors, which are returned on the host
alone: no device is touched before every job of a table has passed."""
import ctypes as C
import os
import re

from gnss_sdr_amd import _lib
from gnss_sdr_amd.telemetry import CnavDecoder, cnav_job_table, cnav_result_capacity, symbols_from_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gsh_cnav_create", "gsh_cnav_destroy", "gsh_cnav_channel_reset", "gsh_cnav_check_jobs", "gsh_cnav_push_u8", "gsh_cnav_push_f32",
                "gsh_cnav_push_f32_device", "gsh_cnav_time_push", "gsh_cnav_channel_get_state", "gsh_cnav_channel_set_state"]


def test_header_declares_the_entry_points_and_structs():
    h = open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    assert "#define GSH_ABI_VERSION 25" in h
    assert re.search(r"int gsh_cnav_create\(int device, int n_channels, int quantiser_mode, float soft_scale, gsh_cnav_t\*\* out\);", h)
    assert re.search(r"void gsh_cnav_destroy\(gsh_cnav_t\* h\);", h)
    assert re.search(r"int gsh_cnav_channel_reset\(gsh_cnav_t\* h, int channel\);", h)
    assert re.search(r"int gsh_cnav_check_jobs\(int n_channels, uint64_t n_symbols, uint32_t n_results, const gsh_cnav_job\* jobs, int n_jobs\);", h)
    assert re.search(r"int gsh_cnav_push_u8\(gsh_cnav_t\* h, const uint8_t\* symbols, uint64_t n_symbols, const gsh_cnav_job\* jobs, int n_jobs, "
                     r"gsh_cnav_message\* results,", h)
    assert re.search(r"int gsh_cnav_push_f32\(gsh_cnav_t\* h, const float\* symbols, uint64_t n_symbols,", h)
    assert re.search(r"int gsh_cnav_push_f32_device\(gsh_cnav_t\* h, const void\* device_symbols, uint64_t n_symbols,", h)
    assert re.search(r"int gsh_cnav_time_push\(gsh_cnav_t\* h, const uint8_t\* symbols, uint64_t n_symbols, const gsh_cnav_job\* jobs, int n_jobs, int reps, "
                     r"float\* avg_ms\);", h)
    assert re.search(r"int gsh_cnav_channel_get_state\(gsh_cnav_t\* h, int channel, gsh_cnav_channel_state\* state\);", h)
    assert re.search(r"int gsh_cnav_channel_set_state\(gsh_cnav_t\* h, int channel, const gsh_cnav_channel_state\* state\);", h)
    for name in ("gsh_cnav_job", "gsh_cnav_message", "gsh_cnav_part_state", "gsh_cnav_channel_state"):
        assert "} %s;" % name in h, name
    assert "#define GSH_CNAV_QUANTISER_HARD 0" in h and "#define GSH_CNAV_QUANTISER_SOFT 1" in h
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS, name
    section = h[h.index("GPS CNAV messages"):]   # the entry points cite the reference lines they replace
    for cite in ("cnav_msg.c:374-390", "cnav_msg.c:415-439", "cnav_msg.c:344", "cnav_msg.h:67-99", "gps_l2c_telemetry_decoder_gs.cc:178",
                 "gps_l5_telemetry_decoder_gs.cc:213", "gps_l5_telemetry_decoder_gs.cc:227-234"):
        assert cite in section, cite


def test_struct_layouts():
    assert C.sizeof(_lib.CnavJob) == 32 and _lib.CnavJob.symbol_offset.offset == 8 and _lib.CnavJob.result_offset.offset == 24
    assert C.sizeof(_lib.CnavMessage) == 60 and _lib.CnavMessage.symbol_index.offset == 40 and _lib.CnavMessage.prn.offset == 52
    assert _lib.CnavMessage.invert_or.offset == 57
    assert C.sizeof(_lib.CnavPartState) == 1240 and _lib.CnavPartState.old_metrics.offset == 512 and _lib.CnavPartState.symbols.offset == 1024
    assert _lib.CnavPartState.decoded.offset == 1152 and _lib.CnavPartState.decisions_index.offset == 1216
    assert C.sizeof(_lib.CnavChannelState) == 2480
    assert (_lib.GSH_CNAV_FLAG_PREAMBLE_SEEN, _lib.GSH_CNAV_FLAG_INVERT, _lib.GSH_CNAV_FLAG_MESSAGE_LOCK, _lib.GSH_CNAV_FLAG_CRC_OK,
            _lib.GSH_CNAV_FLAG_INIT) == (1, 2, 4, 8, 16)


def test_library_exports_the_entry_points(gsh):
    assert gsh.gsh_abi_version() == 25
    for name in ENTRY_POINTS:
        assert getattr(gsh, name, None) is not None, name


GOOD = [dict(channel=0, symbol_offset=0, n_symbols=1200, result_offset=0, result_capacity=3),
        dict(channel=1, symbol_offset=1200, n_symbols=599, result_offset=3, result_capacity=2)]
BAD = {
    "channel = n_channels": dict(GOOD[1], channel=2),
    "negative channel": dict(GOOD[1], channel=-1),
    "duplicate channel": dict(GOOD[1], channel=0),
    "span past the array": dict(GOOD[1], n_symbols=600, result_capacity=2, result_offset=3),
    "offset past the array": dict(GOOD[1], symbol_offset=1 << 40),
    "more than 2^31 symbols": dict(GOOD[1], symbol_offset=0, n_symbols=(1 << 31) + 1, result_capacity=1 << 23),
    "capacity below n / 600 + 1": dict(GOOD[1], symbol_offset=1199, n_symbols=600, result_capacity=1),
    "capacity n / 600 + 1 where two messages fit": dict(GOOD[1], result_capacity=1),             # 577..599 symbols can deliver two
    "capacity n / 600 + 1 where four messages fit": dict(GOOD[1], symbol_offset=0, n_symbols=1793, result_offset=0, result_capacity=3),
    "capacity zero": dict(GOOD[1], result_capacity=0),
    "result slice past the array": dict(GOOD[1], result_offset=4),
    "result slice beyond uint32": dict(GOOD[1], result_offset=0xFFFFFFFF),
    "overlapping result slices": dict(GOOD[1], result_offset=2),
}


def test_range_errors_are_returned_without_a_device(gsh):
    n_symbols, n_results = 1799, 5
    assert gsh.gsh_cnav_check_jobs(2, n_symbols, n_results, cnav_job_table(GOOD), 2) == 0
    assert gsh.gsh_cnav_check_jobs(2, n_symbols, n_results, cnav_job_table(GOOD[::-1]), 2) == 0
    assert gsh.gsh_cnav_check_jobs(2, n_symbols, n_results, cnav_job_table([dict(GOOD[1], n_symbols=0, symbol_offset=1799)]), 1) == 0  # an empty job
    for n, need in ((0, 1), (1, 1), (576, 1), (577, 2), (1152, 2), (1153, 3), (1793, 4), (6000, 11), (1 << 31, 3728271)):
        assert cnav_result_capacity(n) == need and need >= n // 600 + 1
        job = dict(channel=0, symbol_offset=0, n_symbols=n, result_offset=0, result_capacity=need)
        assert gsh.gsh_cnav_check_jobs(1, 1 << 31, 1 << 22, cnav_job_table([job]), 1) == 0, n
        assert gsh.gsh_cnav_check_jobs(1, 1 << 31, 1 << 22, cnav_job_table([dict(job, result_capacity=need - 1)]), 1) == 1, n
    for why, job in BAD.items():
        assert gsh.gsh_cnav_check_jobs(2, n_symbols, n_results, cnav_job_table([GOOD[0], job]), 2) == 1, why  # GSH_ERR_INVALID
        assert b"job 1" in gsh.gsh_last_error(), why
    assert gsh.gsh_cnav_check_jobs(0, n_symbols, n_results, cnav_job_table(GOOD), 2) == 1
    h = C.c_void_p()
    assert gsh.gsh_cnav_create(0, 0, 0, 1.0, C.byref(h)) == 1 and not h
    assert gsh.gsh_cnav_create(0, 1, 2, 1.0, C.byref(h)) == 1 and b"quantiser" in gsh.gsh_last_error()
    assert gsh.gsh_cnav_create(0, 1, 1, 0.0, C.byref(h)) == 1 and b"scale" in gsh.gsh_last_error()
    assert gsh.gsh_cnav_create(0, 1, 1, float("nan"), C.byref(h)) == 1
    assert gsh.gsh_cnav_create(0, 1, 0, 1.0, None) == 1
    assert "#define GSH_CNAV_RESULT_CAPACITY(n) ((n) == 0 ? 1u : ((n) + 575u) / 576u)" in open(os.path.join(ROOT, "include", "gnss_sdr_hip.h")).read()
    res, counts = (_lib.CnavMessage * 5)(), (C.c_int32 * 2)()
    assert gsh.gsh_cnav_push_u8(None, None, 0, cnav_job_table(GOOD), 2, res, 4, counts) == 1 and b"null" in gsh.gsh_last_error()
    assert gsh.gsh_cnav_push_f32(None, None, 0, cnav_job_table(GOOD), 2, res, 4, counts) == 1
    assert gsh.gsh_cnav_push_f32_device(None, None, 0, cnav_job_table(GOOD), 2, res, 4, counts) == 1
    assert gsh.gsh_cnav_channel_reset(None, 0) == 1 and gsh.gsh_cnav_channel_get_state(None, 0, None) == 1
    assert gsh.gsh_cnav_channel_set_state(None, 0, None) == 1 and gsh.gsh_cnav_time_push(None, None, 0, None, 0, 1, None) == 1
    gsh.gsh_cnav_destroy(None)


def test_symbols_from_records_takes_either_component():
    class Rec:
        def __init__(self, flags, i, q, counter):
            self.symbol_flags, self.p_data_accu, self.sample_counter = flags, (i, q), counter
    recs = [Rec(1, 1.5, -2.5, 10), Rec(0, 9.0, 9.0, 20), Rec(3, -3.5, 4.5, 30)]
    sym, counters = symbols_from_records(recs)
    assert sym.tolist() == [1.5, -3.5] and counters.tolist() == [10, 30]   # as before: Prompt_I
    assert symbols_from_records(recs, 0)[0].tolist() == [1.5, -3.5]
    sym_q, counters_q = symbols_from_records(recs, component=1)              # GPS L5 reads Prompt_Q
    assert sym_q.tolist() == [-2.5, 4.5] and counters_q.tolist() == [10, 30]


def test_a_decoder_refused_at_construction_can_still_be_closed(gsh):
    for kwargs in (dict(signal="L1"), dict(quantiser="soft"), dict(quantiser=("hard", 1.0))):
        dec = CnavDecoder.__new__(CnavDecoder)
        try:
            dec.__init__(1, **kwargs)
        except ValueError:
            pass
        else:
            raise AssertionError(kwargs)
        dec.close()   # what __del__ calls: there is no handle, and that is no error
