"""Signals with secondary codes beyond GPS L1 C/A and Galileo E1 (tests/secondary_code_cases.py) through the CPU oracle loop, asserted from the truth
built into the signal: state sequence, the period of the hand-over to state 3 / 4, symbol cadence, decoded bits, no loss of lock.  The device loop is
held to the same oracle runs in tests/test_secondary_code_loop_gpu.py."""
import os

import numpy as np
import pytest

import oracle
import secondary_code_cases as cases


def test_secondary_code_constants_match_the_reference_headers():
    d = "/root/reference/src/core/system_parameters/"
    if not os.path.exists(d + "GPS_L5.h"):
        pytest.skip("reference tree not present")
    l5 = open(d + "GPS_L5.h").read()
    assert f'GPS_L5I_NH_CODE_STR[11] = "{cases.GPS_L5I_NH_CODE}"' in l5 and f'GPS_L5Q_NH_CODE_STR[21] = "{cases.GPS_L5Q_NH_CODE}"' in l5
    assert f'BEIDOU_B1I_SECONDARY_CODE_STR[21] = "{cases.GPS_L5Q_NH_CODE}"' in open(d + "Beidou_B1I.h").read()
    assert f'GALILEO_E5A_I_SECONDARY_CODE[] = "{cases.GALILEO_E5A_I_SECONDARY_CODE}"' in open(d + "Galileo_E5a.h").read()


def test_the_100_symbol_pattern_can_only_match_at_lag_0():
    code = cases.E5A_Q_LIKE_SECONDARY_CODE
    assert len(code) == 100 and set(code) == {"0", "1"}
    # acquire_secondary (trk.cc:1118-1160) wants |sum of sign agreements| == 100: any cyclic shift of the pattern must disagree with it (or its inverse) somewhere
    assert cases.worst_off_peak_circular_autocorrelation(code) < 100
    for nh in (cases.GPS_L5I_NH_CODE, cases.GPS_L5Q_NH_CODE, cases.GALILEO_E5A_I_SECONDARY_CODE):
        assert cases.worst_off_peak_circular_autocorrelation(nh) < len(nh)


def test_secondary_code_signal_carries_what_it_says():
    """the builder's own truth, read back without a loop: wiping the carrier and the code off a noise-free signal leaves secondary chip x bit per code period"""
    sec, dsec, spb, first = cases.GPS_L5Q_NH_CODE, cases.GPS_L5I_NH_CODE, 10, 7
    p, d = oracle.ca_code(7).astype(np.float64), oracle.ca_code(19).astype(np.float64)
    bits = "1101000101"
    x, n = cases.pilot_data_with_secondary_codes(60, 4e6, p, d, 0.0, bits, sec, dsec, spb, first=first, cn0_dbhz=120.0)
    idx = np.floor(np.arange(n) * (1.023e6 / 4e6)).astype(np.int64)
    for k in range(60):
        w = x[k * n:(k + 1) * n].real
        pilot, data = np.sign(np.dot(w, p[idx])), np.sign(np.dot(w, d[idx]))
        assert pilot == (1.0 if sec[(k - first) % 20] == "0" else -1.0), k
        bit = 1.0 if bits[((k - first) // spb) % len(bits)] == "1" else -1.0
        assert data == bit * (1.0 if dsec[(k - first) % 10] == "0" else -1.0), k


@pytest.mark.parametrize("name", list(cases.SECONDARY_CODE_CASES))
def test_oracle_secondary_code_structures(name):
    """The signal structures beyond L1 C/A and E1 (GPS L5 / QZSS L5 pilot, Galileo E5a pilot, BeiDou B1I, GPS L5I) at the smallest shape that runs their
    paths: E/P/L (+ data tap), a secondary code with several symbols per bit, a data secondary code, extended integration over a secondary code.
    Everything asserted follows from the builder's truth: secondary period 0 sits at code period `first`, so the first window that holds the whole
    code from its first chip ends at period first + len - 1 and the loop leaves state 2 at first + len; bit j spans periods first + j x symbols_per_bit.
    Polarity: a pilot channel's four-quadrant PLL puts the wiped pilot on +I, so the wiped data prompt is the bit itself.  A data-only channel's Costas
    loop settles either way round and the search tells which (symbol_flags bit 1) -- with the reference's conventions (the search reads a '0' chip as a
    NEGATIVE prompt, trk.cc:1118-1160, the wipe multiplies a '0' chip by +1, trk.cc:1493-1512) the wiped symbol is +bit when the flag is SET."""
    pilot, sec, dsec, spb, ext, first = cases.SECONDARY_CODE_CASES[name]
    x, code, dcode, bits, rec = cases.secondary_case_oracle(name)
    assert len(rec) == cases.SECONDARY_CASE_PERIODS and not any(r.flags & 2 for r in rec)       # no loss of lock
    states = [r.state for r in rec]
    h = first + len(sec)
    assert states[:h] == [2] * h and h % len(sec) == first % len(sec)
    cycle = [3] * (ext - 1) + [4]
    assert states[h:] == (cycle * (len(rec) // ext + 1))[:len(rec) - h]
    out = [i for i, r in enumerate(rec) if r.symbol_flags & 1]
    assert out == list(range(h + spb - 1, len(rec), spb)) and len(out) >= 15
    flag = rec[-1].symbol_flags & 2
    # (the search sets the polarity flag in the period that completes it: the last one in state 2)
    assert all((r.symbol_flags & 2) == flag for r in rec[h - 1:]) and not any(r.symbol_flags & 2 for r in rec[:h - 1])
    polarity = 1.0 if (pilot or flag) else -1.0
    got = "".join("1" if polarity * rec[i].p_data_accu[0] > 0 else "0" for i in out)
    exp = "".join(bits[((i - first) // spb) % len(bits)] for i in out)
    assert got == exp
    if pilot:
        assert flag   # (this stream's Costas loop settled with the '0' chips positive: no half-cycle turn at the switch to the four-quadrant discriminator)
    if ext > 1:
        assert all(rec[k].carr_error_filt_hz == 0.0 for k in range(h, len(rec)) if states[k] == 3)
    assert abs(np.mean([r.carrier_doppler_hz for r in rec[-100:] if r.state != 3]) - cases.SECONDARY_CASE_DOPPLER_HZ) < 1.0


