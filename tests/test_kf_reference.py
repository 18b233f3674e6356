"""tests/kf_reference.py -- kf_tracking as a Python model -- on synthetic GPS L1 C/A streams: it pulls in, holds lock and hands out the navigation symbols.
The bars are the project's for a tracking loop (tests/test_tracking_loop_gpu.py): mean Doppler error of the last 80 periods below 1.5 Hz, prompt above 0.9
of the nominal amplitude."""
import numpy as np

import oracle
from gnss_sdr_amd.tracking_loop import set_symbol_sync, trk_conf
from helpers import cn0_to_amplitude, synth_gps_l1_stream
from kf_reference import KfTrackingModel
from symbol_sync_cases import GPS_CA_PREAMBLE_SYMBOLS, gps_l1_with_nav_bits

KF_KW = dict(fs_in=4e6, vector_length=4000, early_late_space_chips=0.25, spc=0.25)  # Kf_Conf's spacing (kf_conf.cc:49)


def test_state_2_pulls_in_and_holds_lock():
    fs, n, epochs = 4e6, 4000, 400
    prns, dops, cphs = [3, 9, 17, 22], [1200.0, -2750.0, 4100.0, 35.0], [417.3, 12.9, 800.4, 333.3]
    x = synth_gps_l1_stream(epochs * n + 3 * n, fs, prns, dops, cphs, cn0_dbhz=47.0, seed_noise=31)
    amp = cn0_to_amplitude(47.0, fs) * n
    for prn, fd, cph in zip(prns, dops, cphs):
        f_code = 1.023e6 * (1 + fd / 1575.42e6)
        start = int(round((1023.0 - cph) / f_code * fs + 0.15 * fs / 1.023e6))  # 0.15 chip late
        rec = KfTrackingModel(trk_conf(**KF_KW), oracle.ca_code(prn), x, start, 0, fd - 12.0).run(epochs)
        assert len(rec) == epochs
        tail = rec[-80:]
        print(prn, np.mean([r.carrier_doppler_hz for r in tail]) - fd, np.mean([np.hypot(r.corr[2], r.corr[3]) for r in tail]) / amp)
        assert abs(np.mean([r.carrier_doppler_hz for r in tail]) - fd) < 1.5, prn
        assert np.mean([np.hypot(r.corr[2], r.corr[3]) for r in tail]) > 0.9 * amp, prn
        assert all(r.state == 0 and r.carr_error_filt_hz == r.carrier_doppler_hz for r in rec)


def gps_symbol_case(extend=20):
    """1 s of pull-in, alternating bits, the preamble, more bits (the scenario of tests/test_symbol_sync.py)"""
    bits = "01" * 27 + "10001011" + "0110100111000101"
    fs = 4e6  # (not a whole number of samples per chip: at 2.046 Msps early and late select the same chips as the prompt once the spacing narrows)
    x, n = gps_l1_with_nav_bits(1600, fs, 7, -1750.0, bits, first_bit_period=0)
    conf = trk_conf(fs_in=fs, vector_length=n, early_late_space_chips=0.25, spc=0.25, pull_in_time_s=0, enable_lock_detectors=1, early_late_space_narrow_chips=0.2)
    set_symbol_sync(conf, 20, GPS_CA_PREAMBLE_SYMBOLS, has_secondary=False)
    conf.extend_correlation_symbols = extend
    return x, n, bits, conf


def test_symbol_sync_extended_integration_and_symbols():
    x, n, bits, conf = gps_symbol_case()
    rec = KfTrackingModel(conf, oracle.ca_code(7), x, 0, 0, -1742.0).run(1600)
    assert len(rec) == 1600 and not any(r.flags & 2 for r in rec)
    states = [r.state for r in rec]
    first3 = states.index(3)
    assert first3 == (54 + 8) * 20 and set(states[:first3]) == {2}
    assert states[first3:first3 + 40] == ([3] * 19 + [4]) * 2
    closes = [i for i in range(first3, len(rec)) if states[i] == 4]
    flip = -1.0 if (rec[-1].symbol_flags & 2) else 1.0
    got = "".join("1" if flip * rec[i].p_data_accu[0] > 0 else "0" for i in closes)
    m = len(bits) - 62
    assert all(rec[i].symbol_flags & 1 for i in closes)
    assert got[:m] == bits[62:] and m >= 15
    assert abs(np.mean([rec[i].carrier_doppler_hz for i in closes[3:]]) + 1750.0) < 1.5
    amp20 = 20 * cn0_to_amplitude(47.0, 4e6) * n
    assert np.mean([abs(rec[i].p_data_accu[0]) for i in closes[3:]]) > 0.9 * amp20


def test_loss_of_lock_when_the_signal_ends():
    fs, n = 4e6, 4000
    x = synth_gps_l1_stream(1500 * n, fs, [5], [800.0], [0.0], cn0_dbhz=47.0, seed_noise=9).copy()
    half = 600 * n
    noise = np.random.default_rng(77)
    x[half:] = (noise.standard_normal(len(x) - half) + 1j * noise.standard_normal(len(x) - half)).astype(np.complex64)
    conf = trk_conf(**KF_KW, pull_in_time_s=0, enable_lock_detectors=1, cn0_min=36, max_code_lock_fail=50, cn0_smoother_alpha=0.05)
    rec = KfTrackingModel(conf, oracle.ca_code(5), x, 0, 0, 795.0).run(1400)
    assert rec[-1].flags & 2 and 600 < len(rec) < 1400 and rec[-1].prn_length_samples == 0
    assert not any(r.flags & 2 for r in rec[:-1])
