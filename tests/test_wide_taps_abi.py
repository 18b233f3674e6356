"""The wide correlator bank's additions to the C ABI: header, ctypes binding and library agree (no GPU)."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnss_sdr_hip.h")
WIDE_SYMBOLS = ("gsh_bank_correlate_wide", "gsh_bank_time_launches_wide")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_binding_and_library_agree_on_the_wide_symbols(gsh):
    from gnss_sdr_amd import _lib
    text = _header()
    for name in WIDE_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in the header"
        assert name in _lib.SYMBOLS, f"{name} has no prototype in _lib.py"
        assert getattr(gsh, name, None) is not None, f"{name} is not exported by the library"
    assert not [n for n in _lib.missing_symbols() if n in WIDE_SYMBOLS]
    # the argument lists: (bank, jobs, n_jobs, out) and (bank, jobs, n_jobs, reps, avg_ms)
    assert len(_lib.SYMBOLS["gsh_bank_correlate_wide"][1]) == 4 and len(_lib.SYMBOLS["gsh_bank_time_launches_wide"][1]) == 5
    assert _lib.SYMBOLS["gsh_bank_correlate_wide"][1][1]._type_ is _lib.CorrJobWide


def test_wide_job_record_has_the_size_the_header_states():
    from gnss_sdr_amd import _lib
    text = _header()
    m = re.search(r"\}\s*gsh_corr_job_wide;\s*/\*\s*(\d+) bytes", text)
    assert m, "the header states the size of gsh_corr_job_wide beside its definition"
    assert C.sizeof(_lib.CorrJobWide) == int(m.group(1)) == 296
    body = re.search(r"typedef struct gsh_corr_job_wide\s*\{(.*?)\}\s*gsh_corr_job_wide;", text, re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", body)
    assert fields == [f[0] for f in _lib.CorrJobWide._fields_]
    assert _lib.CorrJobWide.shifts_chips.offset == 40 and _lib.CorrJobWide.shifts_chips.size == 4 * 64


def test_wide_tap_limit_and_abi_version(gsh):
    from gnss_sdr_amd import _lib
    text = _header()
    assert re.search(r"#define\s+GSH_MAX_WIDE_TAPS\s+64\b", text)
    assert _lib.GSH_MAX_WIDE_TAPS == 64 and _lib.GSH_MAX_TAPS == 8
    assert re.search(r"#define\s+GSH_ABI_VERSION\s+25\b", text)
    assert gsh.gsh_abi_version() == 25
