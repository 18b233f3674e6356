"""Scenario builder for signals with secondary codes on the pilot and on the data component (GPS L5 / QZSS L5, Galileo E5a, BeiDou B1I, GPS L5I),
beside the GPS L1 C/A and Galileo E1 builders of tests/symbol_sync_cases.py, and the six small structures the CPU oracle tests
(tests/test_secondary_code_oracle.py), the pinned reference tests (tests/test_oracle_loop_pinned_l5.py) and the device tests
(tests/test_secondary_code_loop_gpu.py) share.

Constants come from the ICDs, not from the reference tree; tests/test_secondary_code_oracle.py checks them against the reference's headers when
those are present."""
import numpy as np

import oracle
from helpers import GPS_CA_CHIP_RATE, GPS_L1_FREQ_HZ, TWO_PI, cn0_to_amplitude

# Neuman-Hofman codes: NH10 on GPS L5I (IS-GPS-705, 3.2.1.2), NH20 on GPS L5Q and on BeiDou B1I / B3I D1 (BDS-SIS-ICD-B1I, 4.2.1);
# Galileo E5a-I secondary code CS20_1 = 0x842E9 (Galileo OS SIS ICD, table 21)
GPS_L5I_NH_CODE = "0000110101"
GPS_L5Q_NH_CODE = "00000100110101001110"
GALILEO_E5A_I_SECONDARY_CODE = "10000100001011101001"


def _sign_of(chars):
    """'0' -> +1, '1' -> -1: how save_correlation_results wipes a secondary chip off a correlator output (trk.cc:1493-1512)"""
    return np.array([1.0 if ch == "0" else -1.0 for ch in chars])


def worst_off_peak_circular_autocorrelation(code: str) -> int:
    s = _sign_of(code)
    return int(max(abs(np.dot(s, np.roll(s, k))) for k in range(1, len(s))))


def _seeded_100_symbol_code() -> str:
    """A fixed 100-symbol pattern standing in for a per-PRN Galileo E5a-Q secondary code (CS100_x): the search in state 2 wants all 100
    signs to agree, so all that matters is that no cyclic shift of the pattern equals it or its inverse (off-peak autocorrelation below 100)."""
    return "".join(np.random.default_rng(100).choice(["0", "1"], 100))


E5A_Q_LIKE_SECONDARY_CODE = _seeded_100_symbol_code()


def pilot_data_with_secondary_codes(n_periods, fs, pilot_code, data_code, doppler_hz, bits, secondary, data_secondary, symbols_per_bit, first=0,
                                    chip_rate=GPS_CA_CHIP_RATE, carrier_hz=GPS_L1_FREQ_HZ, cn0_dbhz=47.0, seed=17, onto=None):
    """pilot_code x secondary[k % len] / sqrt(2)  +  data_code x data_secondary[k % len] x bit[k // symbols_per_bit] / sqrt(2), or (pilot_code None) the
    data component alone at full amplitude; k = code period - first, so the secondary codes' period 0 and bit 0 sit at code period `first`.  The code
    starts at sample 0.  Secondary chips '0' -> +1 as the loop's wipe reads them, bits '1' -> +1; an empty secondary / data_secondary -> no such code
    on that component; the code periods before `first` carry what the cyclic extension gives them (k < 0).  onto: a stream of the same length
    (complex128, unit-variance noise per component already in it) to add the signal to instead of fresh noise.  -> (stream, samples per period)"""
    code_len = len(data_code)
    n = int(round(fs * code_len / chip_rate))
    total = (n_periods + 3) * n
    if onto is None:
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(total) + 1j * rng.standard_normal(total)
    else:
        x = onto
        assert len(x) == total
    t = np.arange(total, dtype=np.float64)
    chips = t * (chip_rate * (1.0 + doppler_hz / carrier_hz) / fs)
    idx = np.floor(chips).astype(np.int64) % code_len
    k = np.floor(chips / code_len).astype(np.int64) - first
    bit = np.array([1.0 if b == "1" else -1.0 for b in bits])[(k // symbols_per_bit) % len(bits)]
    sig = np.asarray(data_code, np.float64)[idx] * bit
    if data_secondary:
        sig *= _sign_of(data_secondary)[k % len(data_secondary)]
    if pilot_code is not None:
        pil = np.asarray(pilot_code, np.float64)[idx]
        if secondary:
            pil = pil * _sign_of(secondary)[k % len(secondary)]
        sig = (sig + pil) / np.sqrt(2.0)
    x += cn0_to_amplitude(cn0_dbhz, fs) * sig * np.exp(1j * TWO_PI * doppler_hz / fs * t)
    return (x.astype(np.complex64) if onto is None else x), n


# ---- the structures beyond GPS L1 C/A and Galileo E1 at the smallest shape that runs their paths of the loop: C/A PRN 7 as "pilot", PRN 19 as "data"
# name: (pilot?, secondary, data secondary, symbols per bit, extend_correlation_symbols, first)
SECONDARY_CODE_CASES = {
    "l5_pilot": (True, GPS_L5Q_NH_CODE, GPS_L5I_NH_CODE, 10, 1, 0),
    "l5_pilot_ext10": (True, GPS_L5Q_NH_CODE, GPS_L5I_NH_CODE, 10, 10, 7),
    "l5_pilot_ext5": (True, GPS_L5Q_NH_CODE, GPS_L5I_NH_CODE, 10, 5, 13),
    "e5a_pilot": (True, E5A_Q_LIKE_SECONDARY_CODE, GALILEO_E5A_I_SECONDARY_CODE, 20, 1, 31),
    "b1i_data": (False, GPS_L5Q_NH_CODE, GPS_L5Q_NH_CODE, 20, 1, 4),
    "l5i_data": (False, GPS_L5I_NH_CODE, "", 10, 1, 2),
}
SECONDARY_CASE_PERIODS = 500
SECONDARY_CASE_DOPPLER_HZ, SECONDARY_CASE_HANDOVER_HZ = 940.0, 935.0


def secondary_case_bits(name: str) -> str:
    return "".join(np.random.default_rng(sorted(SECONDARY_CODE_CASES).index(name) + 50).choice(["0", "1"], 64))


def secondary_case_kw(name: str, fs=4e6, vector_length=4000, **over) -> dict:
    """trk_conf keywords of a case (oracle.trk_conf and gnss_sdr_amd.tracking_loop.trk_conf take the same)"""
    pilot, _, _, _, extend, _ = SECONDARY_CODE_CASES[name]
    kw = dict(fs_in=fs, vector_length=vector_length, track_pilot=int(pilot), pll_bw_hz=25.0, dll_bw_hz=2.0, pull_in_time_s=0, enable_lock_detectors=1,
              pll_bw_narrow_hz=10.0, dll_bw_narrow_hz=1.0, early_late_space_narrow_chips=0.2, extend_correlation_symbols=extend)
    kw.update(over)
    return kw


def secondary_case_sync(name: str, set_symbol_sync, conf) -> None:
    _, sec, dsec, spb, _, _ = SECONDARY_CODE_CASES[name]
    set_symbol_sync(conf, spb, sec, has_secondary=True, data_secondary_code=dsec)


def secondary_case_signal(name: str, n_periods=SECONDARY_CASE_PERIODS, first=None, seed=17, cn0_dbhz=47.0):
    """-> (x, n, bits, tracked code, data code or None) at fs = 4 Msps"""
    pilot, sec, dsec, spb, _, first0 = SECONDARY_CODE_CASES[name]
    p, d = oracle.ca_code(7), oracle.ca_code(19)
    bits = secondary_case_bits(name)
    # a data-only signal carries on its one component the secondary code the loop synchronises to (GPS L5I: NH10, which the block's configuration
    # does not list again as "data secondary code": trk.cc:254-262)
    x, n = pilot_data_with_secondary_codes(n_periods, 4e6, p if pilot else None, d, SECONDARY_CASE_DOPPLER_HZ, bits, sec, dsec if pilot else sec, spb,
                                           first=first0 if first is None else first, cn0_dbhz=cn0_dbhz, seed=seed)
    return (x, n, bits, p, d) if pilot else (x, n, bits, d, None)


_ORACLE_RUNS = {}


def secondary_case_oracle(name: str):
    """-> (x, code, data code, bits, oracle records) of a case, computed once per session and shared by the CPU and the GPU tests (read-only)"""
    if name not in _ORACLE_RUNS:
        x, n, bits, code, dcode = secondary_case_signal(name)
        conf = oracle.trk_conf(**secondary_case_kw(name))
        secondary_case_sync(name, oracle.set_symbol_sync, conf)
        rec = oracle.trk_run(conf, code, x, 0, 0, SECONDARY_CASE_HANDOVER_HZ, SECONDARY_CASE_PERIODS, data_code=dcode, pull_in_over=True)
        _ORACLE_RUNS[name] = (x, code, dcode, bits, rec)
    return _ORACLE_RUNS[name]
