"""PIN of the loop oracle to the reference's GPS_L5_DLL_PLL_Tracking block (CPU), with track_pilot and without: the E/P/L (+ data tap) flavour, NH20 / NH10
secondary codes and ten symbols per bit.  Same driver, comparison and bars as tests/test_oracle_loop_pinned.py, whose helpers it uses."""
import numpy as np
import pytest

from oracle import ref_trk
from test_oracle_loop_pinned import _check_trajectory, _run_both

pytestmark = pytest.mark.skipif(not ref_trk.available(), reason="oracle/_ref/libgnsssdr_ref_trk.so not built (needs /root/reference at build time)")


# ---- GPS L5: E/P/L (+ the data tap), NH20 / NH10 secondary codes, ten symbols per bit --------------------------------------------------------------------------
def _gps_l5_block_and_oracle(track_pilot):
    """the reference's GPS_L5_DLL_PLL_Tracking block and the oracle loop over the same L5 stream, through the pull-in second, the secondary-code search, the switch
    to state 4 and at least five telemetry symbols"""
    from helpers import golden_e1_l5_codes
    from secondary_code_cases import GPS_L5I_NH_CODE, GPS_L5Q_NH_CODE, pilot_data_with_secondary_codes
    fs, prn, fd, first = 12000000, 6, 1500.0, 3
    g = golden_e1_l5_codes()
    l5q, l5i = g["l5q"][prn - 1], g["l5i"][prn - 1]
    rng = np.random.default_rng(9)
    bits = "".join(rng.choice(["0", "1"], 128))
    n_periods = 1000 + 2 * 20 + 80
    if track_pilot:
        x, n = pilot_data_with_secondary_codes(n_periods + 10, fs, l5q, l5i, fd, bits, GPS_L5Q_NH_CODE, GPS_L5I_NH_CODE, 10, first=first,
                                               chip_rate=10.23e6, carrier_hz=1176.45e6, cn0_dbhz=47.0)
    else:
        x, n = pilot_data_with_secondary_codes(n_periods + 10, fs, None, l5i, fd, bits, "", GPS_L5I_NH_CODE, 10, first=first,
                                               chip_rate=10.23e6, carrier_hz=1176.45e6, cn0_dbhz=47.0)
    p = {"GNSS-SDR.internal_fs_sps": fs, "Tracking.pll_bw_hz": 25.0, "Tracking.dll_bw_hz": 2.0, "Tracking.early_late_space_chips": 0.5,
         "Tracking.track_pilot": "true" if track_pilot else "false", "Tracking.pull_in_time_s": 0}
    t = ref_trk.RefTrackingChannel("GPS_L5_DLL_PLL_Tracking", p)
    acq_stamp, acq_doppler = n, fd - 8.0            # the code starts at sample 0 of the stream
    t.set_acquisition("G", "L5", prn, 0.0, acq_doppler, acq_stamp)
    t.work(x[:2 * n])
    t.start_tracking()
    c, outs, rec, start = _run_both(t, x, n, acq_stamp, acq_doppler, n_periods)
    # the block's own replicas (gps_l5i_code_gen_float / gps_l5q_code_gen_float) are what the signal was built from
    code, data_code = t.codes()
    assert np.array_equal(code, l5q if track_pilot else l5i) and (not track_pilot or np.array_equal(data_code, l5i))
    if c["interchange_iq"]:
        # trk.cc:2170-2179, 2222-2231: the data-only L5I block publishes its symbol with I and Q interchanged -- a matter of the output item, not of the loop:
        # the oracle's record holds d_P_data_accu as it is
        outs = [dict(o, prompt_i=o["prompt_q"], prompt_q=o["prompt_i"]) for o in outs]
    return c, outs, rec, start, n, acq_doppler, fs, first


@pytest.mark.parametrize("track_pilot", [True, False])
def test_gps_l5_secondary_codes_lock_and_data_symbols(track_pilot):
    """GPS L5 with track_pilot (E/P/L on L5Q, NH20 search and wipe, the data prompt on L5I wiped by NH10, ten symbols per bit) and without (E/P/L on L5I,
    NH10 search and wipe on the accumulators, the bit summed from the unwiped prompts, trk.cc:1553-1581): block and oracle period by period with this file's
    bars, through the switch to state 4 and at least five symbols."""
    c, outs, rec, start, n, acq_doppler, fs, first = _gps_l5_block_and_oracle(track_pilot)
    sec_len = 20 if track_pilot else 10
    assert (c["track_pilot"], c["secondary"], c["symbols_per_bit"], c["secondary_code_length"], c["data_secondary_code_length"], c["n_correlator_taps"]) == \
        (int(track_pilot), 1, 10, sec_len, 10 if track_pilot else 0, 3)
    assert c["interchange_iq"] == (0 if track_pilot else 1)
    _check_trajectory(outs, rec, c, start, acq_doppler, float(fs), 2 * n)
    states = [r.state for r in rec]
    assert states[0] == 2 and 4 in states
    first4 = states.index(4)
    assert all(s == 4 for s in states[first4:]) and 1000 <= first4 <= 1000 + 2 * sec_len + 2
    # the search succeeded in the period that completed the secondary code: record k is code period (start / n rounded) + k of the stream
    assert (int(round(start / n)) + first4 - first) % sec_len == 0
    produced = [k for k, o in enumerate(outs) if o["produced"]]
    assert len(produced) >= 5 and produced[0] == first4 + 9 and all(b - a == 10 for a, b in zip(produced, produced[1:]))
