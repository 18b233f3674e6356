"""GPU tests of the Kalman-filter tracking loop (gsh_trk_set_kalman: kf_tracking closed on the device).

Two checkers.  (a) REPLAY, exact: the device's own discriminator outputs (the records' code_error_chips / carr_phase_error_hz) and C/N0 go through the host
build of csrc/kalman_step.h -- the text the kernel compiles, contraction off on both sides, no library call in it -- and x, P and R must come out bit for
bit.  (b) CLOSED LOOP against tests/kf_reference.py (kf_tracking as a Python model on the oracle's correlator), with the comparison rule of
tests/test_tracking_loop_gpu.py::_compare restated: until the first chip-edge flip the project's tight bars (identical windows, Doppler 0.05 Hz, correlators
2e-4 of the prompt, discriminators 1e-4); from the first flip on, bars MEASURED on the checker itself: the model is run twice on the test's own streams, plain and
with every correlator output perturbed by 1e-5 relative (the size of the documented GPU-vs-oracle difference), and the largest difference per quantity over
all channels and periods, times 2, is the bar (never below the tight bar).  The Kalman code state feeds the discriminator straight back into the code phase,
so these differ from the DLL/PLL loop's loose bars.  Measured on the development machine (model against perturbed model, largest difference / bar = 2 x):
    E/P/L GPS L1 C/A, 4 Msps, 4 channels x 350 periods: correlators 0.0540 / 0.108 of the prompt scale, code discriminator 0.0244 / 0.0488 chip, carrier
        discriminator 0.0075 / 0.0150 Hz, Doppler 0.0656 / 0.131 Hz, code frequency 4.3e-5 chip/s (the tight 2e-3 stays); first flips at periods 7 .. 37
    Galileo E1 VE/E/P/L/VL + pilot, 32 Msps, 40 periods: correlators 0.121 / 0.242, code discriminator 0.0819 / 0.164 chip, carrier discriminator
        0.0102 / 0.0204 Hz, Doppler 0.0929 / 0.186 Hz; first flip at period 4
    GPS L1 C/A, 4 Msps, symbol sync, extend 20, 1600 periods: correlators 0.0400 / 0.0801, code discriminator 0.0331 / 0.0663 chip, carrier discriminator
        0.0055 / 0.0110 Hz, Doppler 0.0460 / 0.0919 Hz
(every test prints its own figures).  Fixed whatever the bars: every period is compared under one of the two sets, compared == len(records), window offsets
never exceed one sample."""
import ctypes as C

import numpy as np
import pytest

import kf_host
import oracle
from helpers import add_code_signal, cn0_to_amplitude, golden_e1_l5_codes, synth_gps_l1_stream
from kf_reference import KfTrackingModel
from symbol_sync_cases import GPS_CA_PREAMBLE_SYMBOLS, gps_l1_with_nav_bits

pytestmark = pytest.mark.gpu

GSH_ERR_INVALID, GSH_ERR_STATE = 1, 4
TIGHT = dict(corr=2e-4, doppler=0.05, code_freq=2e-3, code_disc=1e-4, carr_disc=1e-4)


def _kf_loop(gpu, conf, n_channels, max_len, kf=None):
    from gnss_sdr_amd.tracking_loop import TrackingLoop, kf_conf
    loop = TrackingLoop(conf, n_channels, max_len, device=gpu)
    loop.set_kalman(kf if kf is not None else kf_conf())
    return loop


def _bytes(r):
    return C.string_at(C.addressof(r), C.sizeof(r))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _prompt_index(n_taps):
    return n_taps - 1 if n_taps == 3 else 4


def _pair_differences(rec_a, rec_b, n_taps):
    """largest difference per quantity between two runs of the model (the measurement behind the post-flip bars)"""
    pi = _prompt_index(n_taps)
    d = dict(corr=0.0, doppler=0.0, code_freq=0.0, code_disc=0.0, carr_disc=0.0, offset=0, first_flip=None)
    for e, (a, b) in enumerate(zip(rec_a, rec_b)):
        pa, pb = np.array(list(a.corr)[:2 * n_taps]), np.array(list(b.corr)[:2 * n_taps])
        scale = max(np.hypot(pb[pi], pb[pi + 1]), 50.0)
        dev = float(np.max(np.abs(pa - pb))) / scale
        if dev > TIGHT["corr"] and d["first_flip"] is None:
            d["first_flip"] = e
        d["corr"] = max(d["corr"], dev)
        d["doppler"] = max(d["doppler"], abs(a.carrier_doppler_hz - b.carrier_doppler_hz))
        d["code_freq"] = max(d["code_freq"], abs(a.code_freq_chips - b.code_freq_chips))
        d["code_disc"] = max(d["code_disc"], abs(a.code_error_chips - b.code_error_chips))
        d["carr_disc"] = max(d["carr_disc"], abs(a.carr_phase_error_hz - b.carr_phase_error_hz))
        d["offset"] = max(d["offset"], abs(int(a.sample_counter) - int(b.sample_counter)))
    return d


def _loose_bars(pairs, n_taps, tag):
    """2 x the largest model-vs-perturbed-model difference over all (plain, perturbed) record lists, never below the tight bars"""
    worst = dict(corr=0.0, doppler=0.0, code_freq=0.0, code_disc=0.0, carr_disc=0.0)
    flips = []
    for a, b in pairs:
        d = _pair_differences(a, b, n_taps)
        assert d["offset"] <= 1, (tag, d)
        flips.append(d["first_flip"])
        for k in worst:
            worst[k] = max(worst[k], d[k])
    bars = {k: max(TIGHT[k], 2.0 * v) for k, v in worst.items()}
    print(f"{tag}: model vs perturbed model, largest differences {worst}, first flips {flips}; post-flip bars {bars}")
    return bars


def _compare(rec_gpu, rec_ref, n_taps, tag, loose):
    """tests/test_tracking_loop_gpu.py::_compare restated for the Kalman loop: tight bars until the first chip-edge flip (or one-sample window offset), the measured
    bars `loose` from then on; every period under one of the two sets"""
    assert len(rec_gpu) == len(rec_ref), (tag, len(rec_gpu), len(rec_ref))
    pi = _prompt_index(n_taps)
    flips, compared, worst_after = 0, 0, dict(corr=0.0, doppler=0.0, code_disc=0.0)
    for e, (g, o) in enumerate(zip(rec_gpu, rec_ref)):
        assert abs(int(g.sample_counter) - int(o.sample_counter)) <= 1, (tag, e, g.sample_counter, o.sample_counter)
        assert g.state == o.state and g.symbol_flags == o.symbol_flags, (tag, e, g.state, o.state, g.symbol_flags, o.symbol_flags)
        pg, po = np.array(list(g.corr)[:2 * n_taps]), np.array(list(o.corr)[:2 * n_taps])
        scale = max(np.hypot(po[pi], po[pi + 1]), 50.0)
        dev = float(np.max(np.abs(pg - po))) / scale
        if flips == 0 and g.sample_counter != o.sample_counter:
            # before any flip a window may only move where the float64 block length sat on an integer boundary
            prev = rec_ref[e - 1]
            assert min(prev.rem_code_phase_samples, 1.0 - prev.rem_code_phase_samples) < 1e-6, (tag, e, g.sample_counter, o.sample_counter)
            flips += 1
        if dev > TIGHT["corr"]:
            flips += 1
        bars = loose if flips > 0 else TIGHT
        assert g.flags == o.flags, (tag, e)
        assert dev <= bars["corr"], (tag, e, dev, bars["corr"], flips)
        assert abs(g.carrier_doppler_hz - o.carrier_doppler_hz) <= bars["doppler"], (tag, e, g.carrier_doppler_hz, o.carrier_doppler_hz, flips)
        assert abs(g.code_freq_chips - o.code_freq_chips) <= bars["code_freq"], (tag, e, g.code_freq_chips, o.code_freq_chips, flips)
        assert abs(g.code_error_chips - o.code_error_chips) <= bars["code_disc"], (tag, e, g.code_error_chips, o.code_error_chips, flips)
        assert abs(g.carr_phase_error_hz - o.carr_phase_error_hz) <= bars["carr_disc"], (tag, e, g.carr_phase_error_hz, o.carr_phase_error_hz, flips)
        if flips == 0:
            near_int = min(o.rem_code_phase_samples, 1.0 - o.rem_code_phase_samples)
            assert g.prn_length_samples == o.prn_length_samples or near_int < 1e-6, (tag, e)
            assert abs(g.code_error_filt_chips - o.code_error_filt_chips) <= 1e-4 and abs(g.carr_freq_error_hz - o.carr_freq_error_hz) <= 0.05, (tag, e)
        else:
            worst_after["corr"] = max(worst_after["corr"], dev)
            worst_after["doppler"] = max(worst_after["doppler"], abs(g.carrier_doppler_hz - o.carrier_doppler_hz))
            worst_after["code_disc"] = max(worst_after["code_disc"], abs(g.code_error_chips - o.code_error_chips))
        compared += 1
    assert compared == len(rec_ref), (tag, compared)
    print(f"{tag}: {compared} periods compared, first flip events {flips}, largest post-flip differences {worst_after}")
    return flips


# ---- scenarios -------------------------------------------------------------------------------------------------------------------------------------------
PRNS, DOPS, CPHS = [3, 9, 17, 22], [1200.0, -2750.0, 4100.0, 35.0], [417.3, 12.9, 800.4, 333.3]


def _gps_state2_case(epochs):
    from gnss_sdr_amd.tracking_loop import trk_conf
    fs, n = 4e6, 4000
    conf = trk_conf(fs_in=fs, vector_length=n, early_late_space_chips=0.25, spc=0.25)  # Kf_Conf's spacing
    x = synth_gps_l1_stream(epochs * n + 3 * n, fs, PRNS, DOPS, CPHS, cn0_dbhz=47.0, seed_noise=31)
    starts = [int(round((1023.0 - cph) / (1.023e6 * (1 + fd / 1575.42e6)) * fs + 0.15 * fs / 1.023e6)) for fd, cph in zip(DOPS, CPHS)]  # 0.15 chip late
    return conf, x, starts, fs, n


def _gps_symbol_case():
    from gnss_sdr_amd.tracking_loop import set_symbol_sync, trk_conf
    bits = "01" * 27 + "10001011" + "0110100111000101"
    fs = 4e6  # (not a whole number of samples per chip: at 2.046 Msps early and late select the same chips as the prompt once the spacing narrows)
    x, n = gps_l1_with_nav_bits(1600, fs, 7, -1750.0, bits, first_bit_period=0)
    conf = trk_conf(fs_in=fs, vector_length=n, early_late_space_chips=0.25, spc=0.25, pull_in_time_s=0, enable_lock_detectors=1, early_late_space_narrow_chips=0.2)
    set_symbol_sync(conf, 20, GPS_CA_PREAMBLE_SYMBOLS, has_secondary=False)
    conf.extend_correlation_symbols = 20
    return conf, x, n, bits


# ---- 4. replay, exact ---------------------------------------------------------------------------------------------------------------------------------------
def _replay(loop_steps, loop_whole, n_channels, epochs, acq_dopplers, conf):
    """run(1) x epochs with kf_state() after every call on loop_steps, run(epochs) on loop_whole: the records must be the same bytes (a later call continues
    where the last one stopped), and every period's x, P, R must be what the host build of kalman_step.h makes of the device's own discriminators and C/N0"""
    code_period = conf.code_length_chips / conf.code_chip_rate
    host = [kf_host.HostKalman(code_period, fd, kf_host.KF_DEFAULT_SD, conf.code_chip_rate, conf.signal_carrier_freq) for fd in acq_dopplers]
    whole, done = loop_whole.run(epochs)
    assert done[:n_channels] == [epochs] * n_channels
    seen = {2: 0, 3: 0, 4: 0, 0: 0}
    switches = 0
    for e in range(epochs):
        rec, done = loop_steps.run(1)
        for ch in range(n_channels):
            assert done[ch] == 1
            r = rec[ch][0]
            assert _bytes(r) == _bytes(whole[ch][e]), (ch, e)
            x, P, R = loop_steps.kf_state(ch)
            h = host[ch]
            seen[r.state] += 1
            if r.state != 3:
                if r.state == 4:
                    h.cn0(conf.early_late_space_narrow_chips, r.cn0_db_hz)                 # update_kf_cn0 with the device's own C/N0 of this period
                    assert np.array_equal(_bits(h.R), _bits(R)), (ch, e, h.R, R)           # (kf_exp10 is part of the shared text: R too is bit for bit)
                    h.set_R(R)
                e_kf = h.run(r.code_error_chips, r.carr_phase_error_hz)
                assert _bits([e_kf])[0] == _bits([r.code_error_filt_chips])[0], (ch, e)
                assert r.carrier_doppler_hz == x[2] == r.carr_error_filt_hz and r.carr_freq_error_hz == x[3]
            if r.state == 2 and e + 1 < epochs and whole[ch][e + 1].state == 3:
                # the switch into the extended integration: Q is replaced by the propagated sum, Ti stretched, R rebuilt (with the wide spacing)
                h.narrow(conf.extend_correlation_symbols, float(np.float32(conf.extend_correlation_symbols) * np.float32(code_period)), conf.spc, r.cn0_db_hz)
                switches += 1
                assert np.array_equal(_bits(h.R), _bits(R)), (ch, e, h.R, R)
            assert np.array_equal(_bits(h.x), _bits(x)), (ch, e, r.state, h.x, x)
            assert np.array_equal(_bits(h.P), _bits(P)), (ch, e, r.state, h.P - P)
            assert x[0] == 0.0
    return seen, switches


def test_replay_state_2_is_bit_exact(gpu):
    epochs = 300
    conf, x, starts, fs, n = _gps_state2_case(epochs)
    loops = []
    for _ in range(2):
        loop = _kf_loop(gpu, conf, 4, 1023)
        loop.set_stream_host(x)
        for ch, prn in enumerate(PRNS):
            loop.start(ch, oracle.ca_code(prn), starts[ch], 0, DOPS[ch] - 12.0)
        loops.append(loop)
    seen, _ = _replay(loops[0], loops[1], 4, epochs, [fd - 12.0 for fd in DOPS], conf)
    assert seen[0] == 4 * epochs
    for loop in loops:
        loop.close()


def test_replay_through_the_switch_into_extended_integration_and_state_4_is_bit_exact(gpu):
    conf, x, n, bits = _gps_symbol_case()
    epochs = 1500
    loops = []
    for _ in range(2):
        loop = _kf_loop(gpu, conf, 1, 1023)
        loop.set_stream_host(x)
        loop.start(0, oracle.ca_code(7), 0, 0, -1742.0)
        loops.append(loop)
    seen, switches = _replay(loops[0], loops[1], 1, epochs, [-1742.0], conf)
    print("periods per state", seen)
    assert switches == 1 and seen[2] == 1240 and seen[4] >= 12 and seen[3] == 19 * seen[4], seen
    for loop in loops:
        loop.close()


# ---- 5. closed loop against the model ------------------------------------------------------------------------------------------------------------------------
def test_gps_l1_epl_closed_loop_matches_the_model(gpu):
    epochs, more = 300, 50
    conf, x, starts, fs, n = _gps_state2_case(epochs + more)
    loop = _kf_loop(gpu, conf, 5, 1023)  # channel 4 is never started
    loop.set_stream_host(x)
    for ch, prn in enumerate(PRNS):
        loop.start(ch, oracle.ca_code(prn), starts[ch], 0, DOPS[ch] - 12.0)
    rec, done = loop.run(epochs)
    rec2, done2 = loop.run(more)  # the continuation call
    assert done[4] == 0 and done2[4] == 0
    plain = [KfTrackingModel(conf, oracle.ca_code(prn), x, starts[ch], 0, DOPS[ch] - 12.0).run(epochs + more) for ch, prn in enumerate(PRNS)]
    pert = [KfTrackingModel(conf, oracle.ca_code(prn), x, starts[ch], 0, DOPS[ch] - 12.0, perturb=1e-5, perturb_seed=100 + ch).run(epochs + more) for ch, prn in enumerate(PRNS)]
    loose = _loose_bars(list(zip(plain, pert)), 3, "E/P/L")
    for ch in range(4):
        assert done[ch] == epochs and done2[ch] == more
        _compare(rec[ch] + rec2[ch], plain[ch], 3, f"E/P/L ch{ch}", loose)
    loop.close()


def test_galileo_e1_veml_pilot_closed_loop_matches_the_model(gpu):
    """the set-up of tests/test_tracking_loop_gpu.py::test_galileo_e1_veml_pilot_and_data under the Kalman loop"""
    from gnss_sdr_amd.tracking_loop import trk_conf
    fs, n, epochs = 32e6, 128000, 40
    g = golden_e1_l5_codes()
    rng = np.random.default_rng(41)
    n_stream = (epochs + 2) * n
    x = (rng.standard_normal(n_stream) + 1j * rng.standard_normal(n_stream)).astype(np.complex64)
    amp = cn0_to_amplitude(45.0, fs)
    fd, ph = -1830.0, 3000.0
    rate = 1.023e6 * (1 + fd / 1575.42e6) / fs * 2.0
    add_code_signal(x, (g["e1b"][7] - g["e1c"][7]) / np.sqrt(2.0), fs, rate, ph, fd, amp)
    conf = trk_conf(fs_in=fs, vector_length=n, code_length_chips=4092, code_samples_per_chip=2, veml=1, track_pilot=1, cloop=0,
                    early_late_space_chips=0.15, very_early_late_space_chips=0.5)
    loop = _kf_loop(gpu, conf, 1, 8184)
    loop.set_stream_host(x)
    start = int(round((8184.0 - ph) / rate))
    loop.start(0, g["e1c"][7], start, 0, fd - 5.0, data_code=g["e1b"][7])
    rec, done = loop.run(epochs)
    plain = KfTrackingModel(conf, g["e1c"][7], x, start, 0, fd - 5.0, data_code=g["e1b"][7]).run(epochs)
    pert = KfTrackingModel(conf, g["e1c"][7], x, start, 0, fd - 5.0, data_code=g["e1b"][7], perturb=1e-5, perturb_seed=7).run(epochs)
    loose = _loose_bars([(plain, pert)], 5, "E1 VEML pilot")
    assert done[0] == len(plain) == epochs
    _compare(rec[0], plain, 5, "E1 VEML pilot", loose)
    for rg, ro in zip(rec[0], plain):
        assert abs(rg.prompt_data[0] - ro.prompt_data[0]) <= max(loose["corr"], 2e-4) * max(50.0, abs(complex(*ro.prompt_data)))
    tail = rec[0][-10:]
    expect = amp * n / np.sqrt(2.0)
    assert np.mean([np.hypot(r.corr[4], r.corr[5]) for r in tail]) > 0.85 * expect
    assert np.mean([np.hypot(*r.prompt_data) for r in tail]) > 0.85 * expect
    loop.close()


def test_gps_l1_symbol_sync_extended_integration_matches_the_model(gpu):
    conf, x, n, bits = _gps_symbol_case()
    epochs = 1600
    loop = _kf_loop(gpu, conf, 1, 1023)
    loop.set_stream_host(x)
    loop.start(0, oracle.ca_code(7), 0, 0, -1742.0)
    rec, _ = loop.run(1250)
    rec2, _ = loop.run(350)  # the second launch starts in the middle of a coherent integration
    rec = rec[0] + rec2[0]
    plain = KfTrackingModel(conf, oracle.ca_code(7), x, 0, 0, -1742.0).run(epochs)
    pert = KfTrackingModel(conf, oracle.ca_code(7), x, 0, 0, -1742.0, perturb=1e-5, perturb_seed=3).run(epochs)
    assert [r.state for r in plain] == [r.state for r in pert]
    loose = _loose_bars([(plain, pert)], 3, "symbol sync")
    _compare(rec, plain, 3, "symbol sync", loose)
    closes = [i for i, r in enumerate(rec) if r.state == 4]
    assert len(closes) >= 17 and all(rec[i].symbol_flags & 1 for i in closes)  # telemetry symbols leave once per bit
    flip = -1.0 if (rec[-1].symbol_flags & 2) else 1.0
    got = "".join("1" if flip * rec[i].p_data_accu[0] > 0 else "0" for i in closes)
    m = len(bits) - 62
    assert got[:m] == bits[62:]
    g = np.array([rec[i].p_data_accu[0] for i in closes])
    o = np.array([plain[i].p_data_accu[0] for i in closes])
    assert np.array_equal(np.sign(g), np.sign(o)) and np.max(np.abs(g - o)) <= loose["corr"] * np.mean(np.abs(o))  # (20 prompts, each within the bar)
    loop.close()


# ---- 6. lock properties on the device's own records ----------------------------------------------------------------------------------------------------------
def test_device_loop_pulls_in_and_holds_lock(gpu):
    """the bars of tests/test_kf_reference.py on the device records: Doppler within 1.5 Hz over the last 80 of 400 periods, prompt above 0.9 of the nominal amplitude"""
    epochs = 400
    conf, x, starts, fs, n = _gps_state2_case(epochs)
    loop = _kf_loop(gpu, conf, 4, 1023)
    loop.set_stream_host(x)
    for ch, prn in enumerate(PRNS):
        loop.start(ch, oracle.ca_code(prn), starts[ch], 0, DOPS[ch] - 12.0)
    rec, done = loop.run(epochs)
    amp = cn0_to_amplitude(47.0, fs) * n
    for ch, fd in enumerate(DOPS):
        assert done[ch] == epochs
        tail = rec[ch][-80:]
        err = np.mean([r.carrier_doppler_hz for r in tail]) - fd
        level = np.mean([np.hypot(r.corr[2], r.corr[3]) for r in tail]) / amp
        print(f"ch{ch}: Doppler error {err:+.4f} Hz, prompt {level:.4f} of nominal")
        assert abs(err) < 1.5 and level > 0.9
        x4, P, R = loop.kf_state(ch)
        assert x4[0] == 0.0 and np.all(np.linalg.eigvalsh((P + P.T) / 2) > 0.0)
        assert np.array_equal(R, [0.2 ** 2, 0.3 ** 2])  # state 2: R stays init_kf's
    loop.close()


def test_loss_of_lock_when_the_signal_ends(gpu):
    from gnss_sdr_amd.tracking_loop import trk_conf
    fs, n = 4e6, 4000
    x = synth_gps_l1_stream(1500 * n, fs, [5], [800.0], [0.0], cn0_dbhz=47.0, seed_noise=9).copy()
    half = 600 * n
    noise = np.random.default_rng(77)
    x[half:] = (noise.standard_normal(len(x) - half) + 1j * noise.standard_normal(len(x) - half)).astype(np.complex64)
    conf = trk_conf(fs_in=fs, vector_length=n, early_late_space_chips=0.25, spc=0.25, pull_in_time_s=0, enable_lock_detectors=1, cn0_min=36, max_code_lock_fail=50,
                    cn0_smoother_alpha=0.05)
    loop = _kf_loop(gpu, conf, 1, 1023)
    loop.set_stream_host(x)
    loop.start(0, oracle.ca_code(5), 0, 0, 795.0)
    rec, done = loop.run(1400)
    model = KfTrackingModel(conf, oracle.ca_code(5), x, 0, 0, 795.0).run(1400)
    print("loss of lock at period", done[0], "model", len(model))
    assert 600 < done[0] < 1400 and rec[0][-1].flags & 2 and rec[0][-1].prn_length_samples == 0
    assert not any(r.flags & 2 for r in rec[0][:-1])
    assert abs(done[0] - len(model)) <= 12
    rec2, done2 = loop.run(2)  # the channel has stopped
    assert done2[0] == 0
    loop.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back_to_dll_pll(gpu):
    from gnss_sdr_amd import GshError
    from gnss_sdr_amd.tracking_loop import TrackingLoop, kf_conf, set_symbol_sync, trk_conf

    def refused(fn, code):
        with pytest.raises(GshError) as ei:
            fn()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert len(str(ei.value)) > 25  # (a gsh_last_error() text comes with the code)

    for kw in (dict(high_dyn=1), dict(enable_doppler_correction=1)):
        loop = TrackingLoop(trk_conf(**kw), 1, 1023, device=gpu)
        refused(lambda: loop.set_kalman(kf_conf()), GSH_ERR_INVALID)
        loop.close()
    c = trk_conf()
    set_symbol_sync(c, 20, GPS_CA_PREAMBLE_SYMBOLS)  # symbol sync without the lock detectors
    loop = TrackingLoop(c, 1, 1023, device=gpu)
    refused(lambda: loop.set_kalman(kf_conf()), GSH_ERR_INVALID)
    loop.close()
    loop = TrackingLoop(trk_conf(), 2, 1023, device=gpu)
    loop.set_split(2)
    refused(lambda: loop.set_kalman(kf_conf()), GSH_ERR_INVALID)
    loop.set_split(1)
    for bad in (dict(code_disc_sd_chips=-0.1), dict(carrier_freq_sd_hz=float("nan")), dict(init_carrier_phase_sd_rad=float("inf"))):
        refused(lambda: loop.set_kalman(kf_conf(**bad)), GSH_ERR_INVALID)
    loop.set_kalman(kf_conf())
    refused(lambda: loop.set_split(2), GSH_ERR_INVALID)
    refused(lambda: loop.set_split(0), GSH_ERR_INVALID)
    loop.set_split(1)
    refused(loop.live_begin, GSH_ERR_INVALID)
    # ... while a channel is active: GSH_ERR_STATE, either way
    epochs = 60
    conf, x, starts, fs, n = _gps_state2_case(epochs)
    a = TrackingLoop(conf, 1, 1023, device=gpu)
    a.set_stream_host(x)
    a.set_kalman(kf_conf())
    a.start(0, oracle.ca_code(PRNS[0]), starts[0], 0, DOPS[0] - 12.0)
    refused(lambda: a.set_kalman(None), GSH_ERR_STATE)
    refused(lambda: a.set_kalman(kf_conf()), GSH_ERR_STATE)
    rec_kf, _ = a.run(epochs)
    a._lib.gsh_trk_stop(a._h, 0)
    # switched back, the handle is a DLL/PLL handle again: the same records as one that never was anything else, byte for byte
    a.set_kalman(None)
    a.start(0, oracle.ca_code(PRNS[0]), starts[0], 0, DOPS[0] - 12.0)
    rec_back, _ = a.run(epochs)
    b = TrackingLoop(conf, 1, 1023, device=gpu)
    b.set_stream_host(x)
    b.start(0, oracle.ca_code(PRNS[0]), starts[0], 0, DOPS[0] - 12.0)
    rec_plain, _ = b.run(epochs)
    assert [_bytes(r) for r in rec_back[0]] == [_bytes(r) for r in rec_plain[0]]
    assert [_bytes(r) for r in rec_kf[0]] != [_bytes(r) for r in rec_plain[0]]
    refused(lambda: b.kf_state(0), GSH_ERR_STATE)
    for t in (loop, a, b):
        t.close()


# ---- 8. gsh_trk_time_run saves and restores the filters ---------------------------------------------------------------------------------------------------------
def test_time_run_at_config_2_leaves_the_kalman_state_unchanged(gpu):
    """BASELINE config 2: 32 channels, 25 Msps, 25 000-sample E/P/L windows.  Prints the microseconds per period of the Kalman flavour beside the DLL/PLL flavour's."""
    from gnss_sdr_amd.tracking_loop import TrackingLoop, kf_conf, trk_conf
    fs, n, epochs = 25e6, 25000, 100
    prns = list(range(1, 9))
    dops = [-3000.0 + 800.0 * i for i in range(8)]
    x = synth_gps_l1_stream((epochs + 13) * n, fs, prns, dops, [0.0] * 8, cn0_dbhz=45.0, seed_noise=2)
    conf = trk_conf(fs_in=fs, vector_length=n, early_late_space_chips=0.25, spc=0.25, enable_lock_detectors=1, pull_in_time_s=0)
    us = {}
    for name in ("dll_pll", "kalman"):
        loop = TrackingLoop(conf, 32, 1023, device=gpu)
        if name == "kalman":
            loop.set_kalman(kf_conf())
        loop.set_stream_host(x)
        for ch in range(32):
            loop.start(ch, oracle.ca_code(prns[ch % 8]), 0, 0, dops[ch % 8] - 5.0)
        loop.run(10, want_records=False)
        before = [loop.kf_state(ch) for ch in range(32)] if name == "kalman" else None
        ms = loop.time_run(epochs, reps=5)
        assert ms > 0.0
        us[name] = ms * 1e3 / epochs
        if name == "kalman":
            after = [loop.kf_state(ch) for ch in range(32)]
            for b, a in zip(before, after):
                assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(b, a))
            assert any(np.any(b[1] != np.diag([0.25, 0.49, 25.0, 1.0])) for b in before)  # (the filters have moved off init_kf's P)
        loop.close()
    print(f"config 2 (32 channels, 25 Msps): DLL/PLL {us['dll_pll']:.2f} us per period, Kalman {us['kalman']:.2f} us per period")
