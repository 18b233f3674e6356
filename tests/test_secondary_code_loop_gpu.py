"""GPU tests of the device-closed loop (gsh_trk_*) on the signal structures beyond GPS L1 C/A and Galileo E1: E/P/L plus the data tap, secondary codes on the
pilot and on the data component, several symbols per bit, extended integration over a secondary code (tests/secondary_code_cases.py: SECONDARY_CODE_CASES).
The checker is the CPU oracle loop (oracle.trk_run), which tests/test_secondary_code_oracle.py holds to the truth built into the signals and
tests/test_oracle_loop_pinned_l5.py to the reference's own GPS L5 block; under the Kalman loop it is tests/kf_reference.KfTrackingModel.

Every tolerance is the one of the existing test it is named after; state sequences, symbol flags and symbol signs carry none.

Coverage (test -> flavour of trk_loop_kernel):

    path of the loop                              launched                          live          coop           HD           KF
    CF_TRACK_PILOT with NT = 3                    cases[l5_* / e5a], plain_state_2, live_ring     split[2], [3]  high_dyn     kalman[*]
                                                  launch_boundaries, two_channels,
                                                  true_gps_l5_shape
    CF_DATA_SECONDARY                             cases[l5_* / e5a / b1i],          live_ring     split[2], [3]  high_dyn     kalman[*]
                                                  launch_boundaries, two_channels,
                                                  true_gps_l5_shape
    CF_HAS_SECONDARY with CF_SYMBOLS_GT1          cases[all six] (data-only with and live_ring     split[2], [3]  high_dyn     kalman[*]
                                                  without a data secondary code:
                                                  b1i_data, l5i_data), launch_boundaries,
                                                  two_channels, true_gps_l5_shape
    CF_HAS_SECONDARY with CF_EXTEND_GT1           cases[l5_pilot_ext10 / _ext5],    live_ring     --             --           kalman[l5_pilot_ext10]
                                                  launch_boundaries[l5_pilot_ext10],
                                                  two_channels

(cooperating work-groups and the high-dynamics correlator run l5_pilot, as the project's other tests of those flavours run one structure each)
"""
import numpy as np
import pytest

import oracle
import secondary_code_cases as cases
from helpers import golden_e1_l5_codes
from test_tracking_loop_gpu import _compare

pytestmark = pytest.mark.gpu

XMAX = 6.0      # _compare's default: the largest |sample component| of unit-variance noise plus signal


def _device_conf(name, **over):
    from gnss_sdr_amd.tracking_loop import set_symbol_sync, trk_conf
    conf = trk_conf(**cases.secondary_case_kw(name, **over))
    cases.secondary_case_sync(name, set_symbol_sync, conf)
    return conf


def _oracle_conf(name, **over):
    conf = oracle.trk_conf(**cases.secondary_case_kw(name, **over))
    cases.secondary_case_sync(name, oracle.set_symbol_sync, conf)
    return conf


def _launched(gpu, conf, x, code, dcode, cuts, max_len=1023, handover_hz=cases.SECONDARY_CASE_HANDOVER_HZ, prepare=None):
    """one channel, run(cuts[0]); run(cuts[1]); ... concatenated"""
    from gnss_sdr_amd.tracking_loop import TrackingLoop
    loop = TrackingLoop(conf, 1, max_len, device=gpu)
    if prepare is not None:
        prepare(loop)
    loop.set_stream_host(x)
    loop.start(0, code, 0, 0, handover_hz, data_code=dcode, pull_in_over=True)
    rec = []
    for m in cuts:
        r, done = loop.run(m)
        assert done[0] == m, (done, m)
        rec += r[0]
    loop.close()
    return rec


def _state_machine_equal(rec, ora, tag):
    """no tolerance: the state sequence, the symbol flags, the sign of every emitted symbol"""
    assert len(rec) == len(ora), (tag, len(rec), len(ora))
    assert [r.state for r in rec] == [r.state for r in ora], tag
    assert [r.symbol_flags for r in rec] == [r.symbol_flags for r in ora], tag
    g = np.array([r.p_data_accu[0] for r in rec if r.symbol_flags & 1])
    o = np.array([r.p_data_accu[0] for r in ora if r.symbol_flags & 1])
    assert len(o) >= 5 and np.array_equal(np.sign(g), np.sign(o)), tag
    return g, o


def _correlator_bars(rec, ora):
    """_compare's correlator bar of every period, by the regime _compare holds that period to: (regime, bar) with regime 'tight' (2e-4 of the prompt scale, every
    component), 'loose' (4 xmax + 3e-3 of the scale, every component; from the first chip-edge flip on) or 'shifted' (8 xmax + 1e-2 of the scale on the prompt's
    magnitude; from the first one-sample window offset on)"""
    out, flipped, shifted = [], False, False
    for g, o in zip(rec, ora):
        scale = max(np.hypot(o.corr[2], o.corr[3]), 50.0)
        if not shifted and g.sample_counter != o.sample_counter:
            shifted = True
        if shifted:
            out.append(("shifted", 8.0 * XMAX + 1e-2 * scale))
            continue
        dev = np.max(np.abs(np.array(list(g.corr)[:6]) - np.array(list(o.corr)[:6])))
        if dev > 2e-4 * scale:
            flipped = True
        out.append(("loose", 4.0 * XMAX + 3e-3 * scale) if flipped else ("tight", 2e-4 * scale))
    return out


def _accumulators_within_the_summed_bars(rec, ora, tag):
    """accu[] (the secondary-wiped running sums the discriminators work on, which _compare does not look at): every period's correlators are within _compare's bar
    of that period, a chip of +-1 multiplies them, so a sum over k periods is within the sum of their k bars -- one bar in state 2, up to `extend` in states 3 / 4."""
    bars = _correlator_bars(rec, ora)
    run_bar, worst = 0.0, 0.0
    for e, (g, o) in enumerate(zip(rec, ora)):
        regime, bar = bars[e]
        run_bar = bar if (o.state == 2 or e == 0 or ora[e - 1].state != 3) else run_bar + bar   # a new sum begins after state 2 / state 4
        ga, oa = np.array(list(g.accu)[:6]), np.array(list(o.accu)[:6])
        if regime == "shifted":
            dev = abs(np.hypot(ga[2], ga[3]) - np.hypot(oa[2], oa[3]))
        else:
            dev = float(np.max(np.abs(ga - oa)))
        worst = max(worst, dev / run_bar)
        assert dev <= run_bar, (tag, e, o.state, regime, dev, run_bar)
    return worst


def _prompt_data_worst(rec, ora):
    """largest |device - oracle| of the data tap's real part over the bar of test_galileo_e1_veml_pilot_and_data, 2e-4 max(50, |prompt_data|)"""
    return max(abs(g.prompt_data[0] - o.prompt_data[0]) / (2e-4 * max(50.0, abs(complex(*o.prompt_data)))) for g, o in zip(rec, ora))


def _hold_to_the_oracle(rec, ora, tag, pilot):
    """the assertions every case of the table has to meet"""
    g, o = _state_machine_equal(rec, ora, tag)
    ratio = float(np.max(np.abs(g - o)) / np.mean(np.abs(o)))
    pd = _prompt_data_worst(rec, ora) if pilot else 0.0
    print(f"{tag}: worst symbol |g - o| / mean |o| = {ratio:.3e}, worst prompt_data difference / bar = {pd:.3f}")
    stats = _compare(rec, ora, 3, tag)
    print(f"{tag}: flips {stats['flips']}, shifted_from {stats['shifted_from']}")
    assert ratio < 2e-2, (tag, ratio)                      # the bar of test_device_gps_l1_bit_synchronisation_matches_oracle
    assert stats["compared"] == len(ora)
    if pilot:
        assert pd <= 1.0, (tag, pd)
    worst = _accumulators_within_the_summed_bars(rec, ora, tag)
    print(f"{tag}: worst accu[] difference / summed bar = {worst:.3f}")
    return stats


# ---- the six structures, one launch each -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SECONDARY_CODE_CASES))
def test_secondary_code_structures_match_the_oracle(gpu, name):
    pilot = cases.SECONDARY_CODE_CASES[name][0]
    x, code, dcode, bits, ora = cases.secondary_case_oracle(name)
    rec = _launched(gpu, _device_conf(name), x, code, dcode, [cases.SECONDARY_CASE_PERIODS])
    _hold_to_the_oracle(rec, ora, name, pilot)
    assert 3 in [r.state for r in rec] or cases.SECONDARY_CODE_CASES[name][4] == 1
    assert abs(np.mean([r.carrier_doppler_hz for r in rec[-100:] if r.state != 3]) - cases.SECONDARY_CASE_DOPPLER_HZ) < 1.0


# ---- launch boundaries ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l5_pilot_ext10", "e5a_pilot"])
def test_symbol_counters_survive_launch_boundaries(gpu, name):
    """three launches: the first ends in state 2 with the search's buffer part full, the second behind the hand-over at a period where current_symbol and
    current_data_symbol are both nonzero and differ (in l5_pilot_ext10 inside a coherent integration as well)"""
    pilot, sec, dsec, spb, ext, first = cases.SECONDARY_CODE_CASES[name]
    x, code, dcode, bits, ora = cases.secondary_case_oracle(name)
    h = first + len(sec)
    cut1 = first + len(sec) // 2 + 3                      # state 2: the buffer holds a little more than half the code
    cut2 = h + len(dsec) + 3                              # periods since the hand-over: len(dsec) + 3 -> counters len(dsec) + 3 and 3
    since = cut2 - h
    assert 0 < cut1 < h and ora[cut1].state == 2 and ora[cut2].state == (3 if ext > 1 else 4)
    assert since % len(sec) != 0 and since % len(dsec) != 0 and since % len(sec) != since % len(dsec)
    if ext > 1:
        assert since % ext not in (0, ext - 1) and ora[cut2 - 1].state == 3    # neither the first nor the last period of the integration
    rec = _launched(gpu, _device_conf(name), x, code, dcode, [cut1, cut2 - cut1, len(ora) - cut2])
    _hold_to_the_oracle(rec, ora, f"{name} in three launches", pilot)


# ---- two channels in one handle -------------------------------------------------------------------------------------------------------------------------------
def test_symbol_counters_are_per_channel(gpu):
    """two pilot + data signals in one stream (C/A PRN 7 / 19 and 12 / 25) whose secondary codes begin at code periods 0 and 7: each channel must equal its own
    oracle run"""
    from gnss_sdr_amd.tracking_loop import TrackingLoop
    name, periods = "l5_pilot_ext10", 300
    pilot, sec, dsec, spb, ext, _ = cases.SECONDARY_CODE_CASES[name]
    sig = [(7, 19, 940.0, 0), (12, 25, -1310.0, 7)]
    n = 4000
    rng = np.random.default_rng(29)
    total = (periods + 3) * n
    x = rng.standard_normal(total) + 1j * rng.standard_normal(total)
    for k, (p, d, fd, first) in enumerate(sig):
        cases.pilot_data_with_secondary_codes(periods, 4e6, oracle.ca_code(p), oracle.ca_code(d), fd, cases.secondary_case_bits(name)[k:] , sec, dsec, spb,
                                              first=first, onto=x)
    x = x.astype(np.complex64)
    loop = TrackingLoop(_device_conf(name), 2, 1023, device=gpu)
    loop.set_stream_host(x)
    for ch, (p, d, fd, first) in enumerate(sig):
        loop.start(ch, oracle.ca_code(p), 0, 0, fd - 5.0, data_code=oracle.ca_code(d), pull_in_over=True)
    rec, done = loop.run(periods)
    loop.close()
    assert done == [periods, periods]
    hand_overs = []
    for ch, (p, d, fd, first) in enumerate(sig):
        ora = oracle.trk_run(_oracle_conf(name), oracle.ca_code(p), x, 0, 0, fd - 5.0, periods, data_code=oracle.ca_code(d), pull_in_over=True)
        hand_overs.append([r.state for r in ora].index(3))
        _hold_to_the_oracle(rec[ch], ora, f"two channels ch{ch}", pilot)
    assert hand_overs == [0 + len(sec), 7 + len(sec)]


# ---- E/P/L + the data tap in plain state 2 ---------------------------------------------------------------------------------------------------------------------
def test_epl_with_the_data_tap_in_plain_state_2(gpu):
    """the three-tap pilot flavour at its smallest: no symbol synchronisation, four-quadrant PLL (cloop = 0), four channels and one never started, as
    test_gps_l1_closed_loop_matches_oracle_and_locks runs E/P/L.  The data tap is one more correlator output of the same window, so it is held to _compare's
    correlator bar of the regime the period is in: 2e-4 of its magnitude (the bar of test_galileo_e1_veml_pilot_and_data) until the first chip-edge flip, 4 xmax +
    3e-3 from then on.  The 2e-4 bar alone cannot hold over 300 periods at these Dopplers: once the two loops' code phases differ in their last bits a sample on a
    chip edge picks the neighbouring chip of the data code on one side just as it does for the tracked code (measured on an MI355X: channel 1, two flips, the data
    tap 28.6 times the 2e-4 bar = 4.1, one sample's 2 |x[n]|; the other channels below it)."""
    from gnss_sdr_amd.tracking_loop import TrackingLoop, trk_conf
    fs, n, epochs = 4e6, 4000, 300
    kw = dict(fs_in=fs, vector_length=n, track_pilot=1, cloop=0, pll_bw_hz=35.0, dll_bw_hz=4.0)
    sig = [(3, 4, 1200.0), (9, 10, -2750.0), (17, 18, 4100.0), (22, 23, 35.0)]
    rng = np.random.default_rng(31)
    total = (epochs + 3) * n
    x = rng.standard_normal(total) + 1j * rng.standard_normal(total)
    for p, d, fd in sig:
        cases.pilot_data_with_secondary_codes(epochs, fs, oracle.ca_code(p), oracle.ca_code(d), fd, "1", "", "", 1, onto=x)
    x = x.astype(np.complex64)
    starts = [ch * n + (ch % 2) for ch in range(4)]         # whole code periods into the stream, every other channel one sample (0.26 chip) late
    loop = TrackingLoop(trk_conf(**kw), 5, 1023, device=gpu)
    loop.set_stream_host(x)
    for ch, (p, d, fd) in enumerate(sig):
        loop.start(ch, oracle.ca_code(p), starts[ch], 0, fd - 12.0, data_code=oracle.ca_code(d))
    rec, done = loop.run(epochs)
    loop.close()
    assert done == [epochs] * 4 + [0]
    for ch, (p, d, fd) in enumerate(sig):
        ora = oracle.trk_run(oracle.trk_conf(**kw), oracle.ca_code(p), x, starts[ch], 0, fd - 12.0, epochs, data_code=oracle.ca_code(d))
        stats = _compare(rec[ch], ora, 3, f"plain state 2 ch{ch}")
        pd = _prompt_data_worst(rec[ch], ora)
        print(f"plain state 2 ch{ch}: flips {stats['flips']}, shifted_from {stats['shifted_from']}, worst prompt_data difference / 2e-4 bar = {pd:.3f}")
        worst = 0.0
        for e, (rg, ro, (regime, _)) in enumerate(zip(rec[ch], ora, _correlator_bars(rec[ch], ora))):
            scale = max(50.0, abs(complex(*ro.prompt_data)))
            if regime == "shifted":
                dev, bar = abs(abs(complex(*rg.prompt_data)) - abs(complex(*ro.prompt_data))), 8.0 * XMAX + 1e-2 * scale
            else:
                dev = max(abs(rg.prompt_data[0] - ro.prompt_data[0]), abs(rg.prompt_data[1] - ro.prompt_data[1]))
                bar = 2e-4 * scale if regime == "tight" else 4.0 * XMAX + 3e-3 * scale
            worst = max(worst, dev / bar)
            assert dev <= bar, (ch, e, regime, dev, bar)
        print(f"plain state 2 ch{ch}: worst prompt_data difference / bar of the period's regime = {worst:.3f}")
        tail = rec[ch][-80:]
        assert abs(np.mean([r.carrier_doppler_hz for r in tail]) - fd) < 1.5, ch
        # pilot and data prompts both carry the same amplitude, the data one (bits all '1', pilot on +I) positive
        assert np.mean([r.prompt_data[0] for r in tail]) > 0.85 * np.mean([np.hypot(r.corr[2], r.corr[3]) for r in tail])


# ---- cooperating work-groups -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [2, 3])
def test_cooperating_work_groups_on_l5_pilot(gpu, groups):
    """4000 samples are four trips of 1024 at the pilot trip size: with two work-groups each owns two whole trips, with three the helpers own one each and the last
    one the partial trip.  Bars of test_cooperating_work_groups_with_the_pilot_and_data_taps: _compare and the data tap's 2e-4 bar against the oracle."""
    name = "l5_pilot"
    x, code, dcode, bits, ora = cases.secondary_case_oracle(name)
    rec = _launched(gpu, _device_conf(name), x, code, dcode, [250, 250], prepare=lambda loop: loop.set_split(groups))
    _hold_to_the_oracle(rec, ora, f"{name} split{groups}", True)


# ---- live ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_live_ring_through_the_secondary_code_and_the_extended_integration(gpu):
    """l5_pilot_ext10 as 8-bit items through a ring that wraps (test_live_at_the_baseline_shapes_equals_launched_run_and_oracle): the residency's records equal the
    launched run's byte for byte, and the first 200 meet _compare against the oracle loop on the same quantised samples"""
    from gnss_sdr_amd.sample_stream import SampleStream
    from gnss_sdr_amd.tracking_loop import TrackingLoop
    from test_tracking_live_gpu import _bytes, _drain
    name, scale, n = "l5_pilot_ext10", 20.0, 4000
    x, code, dcode, bits, _ = cases.secondary_case_oracle(name)
    x8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -127, 127).astype(np.int8)
    xf = (x8[:, 0].astype(np.float32) + 1j * x8[:, 1].astype(np.float32)).astype(np.complex64)
    total, epochs = len(xf), cases.SECONDARY_CASE_PERIODS
    flat = _launched(gpu, _device_conf(name), xf, code, dcode, [epochs])

    ring = SampleStream(9 * n + 7, 2 * n, device=gpu)      # shorter than the stream: it wraps
    live = TrackingLoop(_device_conf(name), 1, 1023, device=gpu)
    live.set_stream_ring(ring)
    live.start(0, code, 0, 0, cases.SECONDARY_CASE_HANDOVER_HZ, data_code=dcode, pull_in_over=True)
    got, lost = [[]], [False]
    pushed, blk = 0, 3 * n + n // 2
    while pushed < total:
        m = min(blk, total - pushed)
        ring.push(x8[pushed:pushed + m], "ibyte")
        pushed += m
        if live.live_in_flight() == 0:
            live.live_begin()
        _drain(live, got, lost, 3.0, [min(epochs, max(0, pushed // n - 1))])
    _drain(live, got, lost, 1.0)
    live.live_quiesce()
    _drain(live, got, lost, 0.2)
    live.close()
    ring.close()
    assert epochs <= len(got[0]) <= epochs + 4, len(got[0])
    assert _bytes(got[0][:epochs]) == _bytes(flat), "live records differ from the launched run"
    ora = oracle.trk_run(_oracle_conf(name), code, xf, 0, 0, cases.SECONDARY_CASE_HANDOVER_HZ, 200, data_code=dcode, pull_in_over=True)
    assert 3 in [r.state for r in ora] and sum(1 for r in ora if r.symbol_flags & 1) >= 5
    _state_machine_equal(got[0][:200], ora, "live")
    stats = _compare(got[0][:200], ora, 3, "l5_pilot_ext10 live", xmax=XMAX * scale)
    print(f"l5_pilot_ext10 live: flips {stats['flips']}, shifted_from {stats['shifted_from']}")
    assert stats["compared"] == 200


# ---- Kalman ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l5_pilot", "l5_pilot_ext10"])
def test_kalman_loop_on_l5_pilot_matches_the_model(gpu, name):
    """comparison helpers and bars of tests/test_kf_tracking_gpu.py: tight until the first chip-edge flip, then 2 x the model-against-perturbed-model differences.
    l5_pilot is the first test of the Kalman loop in a state 4 that no extended integration narrowed: update_kf_cn0 (kf.cc:952-969) then reads the spacing the
    constructor set, which gsh_trk_start used to leave at zero (code measurement variance 0; the filtered code error of the first state-4 period 0.0292 chip on the
    device against 0.0243 in the model)."""
    import test_kf_tracking_gpu as kf
    from gnss_sdr_amd.tracking_loop import kf_conf
    from kf_reference import KfTrackingModel
    periods = 300
    x, code, dcode, bits, _ = cases.secondary_case_oracle(name)
    conf = _device_conf(name, early_late_space_chips=0.25, spc=0.25)       # Kf_Conf's spacing

    def model(**kw):
        m = KfTrackingModel(conf, code, x, 0, 0, cases.SECONDARY_CASE_HANDOVER_HZ, data_code=dcode, **kw)
        m.pull_in_limit = 0                                                # the hand-over with the pull-in transitory over (GSH_TRK_START_PULL_IN_OVER)
        return m.run(periods)

    plain, pert = model(), model(perturb=1e-5, perturb_seed=5)
    assert [r.state for r in plain] == [r.state for r in pert]
    first = cases.SECONDARY_CODE_CASES[name][5]
    assert [r.state for r in plain].index(3 if "ext" in name else 4) == first + 20 and sum(1 for r in plain if r.symbol_flags & 1) >= 20
    loose = kf._loose_bars([(plain, pert)], 3, f"kalman {name}")
    rec = _launched(gpu, conf, x, code, dcode, [140, periods - 140], prepare=lambda loop: loop.set_kalman(kf_conf()))
    kf._compare(rec, plain, 3, f"kalman {name}", loose)
    g, o = _state_machine_equal(rec, plain, f"kalman {name}")
    worst = float(np.max(np.abs(g - o)) / np.mean(np.abs(o)))
    print(f"kalman {name}: worst symbol |g - o| / mean |o| = {worst:.3e} (bar {loose['corr']:.3e})")
    assert worst <= loose["corr"]                                          # (as test_gps_l1_symbol_sync_extended_integration_matches_the_model)
    for rg, ro in zip(rec, plain):
        assert abs(rg.prompt_data[0] - ro.prompt_data[0]) <= max(loose["corr"], 2e-4) * max(50.0, abs(complex(*ro.prompt_data)))


# ---- high dynamics ---------------------------------------------------------------------------------------------------------------------------------------------
def test_high_dyn_loop_on_l5_pilot(gpu):
    """under high_dyn the data tap is a correlation of its own (fused_data = !HD && pilot).  Bars of test_device_high_dyn_loop_matches_oracle -- those that do not
    scale with the Doppler rate, which is zero here: the rate estimate starts in the same period, Doppler within 1.5 Hz from period 50 on, nine windows in ten
    identical, mean prompt within 1 % -- and the state machine with no tolerance."""
    name = "l5_pilot"
    x, code, dcode, bits, _ = cases.secondary_case_oracle(name)
    over = dict(high_dyn=1, smoother_length=10)
    periods = cases.SECONDARY_CASE_PERIODS
    ora = oracle.trk_run(_oracle_conf(name, **over), code, x, 0, 0, cases.SECONDARY_CASE_HANDOVER_HZ, periods, data_code=dcode, pull_in_over=True)
    assert [r.state for r in ora].index(4) == 20 and len(ora) == periods
    rec = _launched(gpu, _device_conf(name, **over), x, code, dcode, [periods])
    g, o = _state_machine_equal(rec, ora, "high_dyn")
    ratio = float(np.max(np.abs(g - o)) / np.mean(np.abs(o)))
    assert all(r.carrier_phase_rate_step_rad == 0.0 for r in rec[:19]) and rec[19].carrier_phase_rate_step_rad != 0.0
    gd = np.array([r.carrier_doppler_hz for r in rec])
    od = np.array([r.carrier_doppler_hz for r in ora])
    same = sum(1 for a, b in zip(rec, ora) if a.sample_counter == b.sample_counter)
    gp = np.mean([np.hypot(r.corr[2], r.corr[3]) for r in rec[300:]])
    op = np.mean([np.hypot(r.corr[2], r.corr[3]) for r in ora[300:]])
    gq = np.mean([np.hypot(*r.prompt_data) for r in rec[300:]])
    oq = np.mean([np.hypot(*r.prompt_data) for r in ora[300:]])
    print(f"high_dyn l5_pilot: worst symbol |g - o| / mean |o| = {ratio:.3e}, Doppler difference {np.max(np.abs(gd[50:] - od[50:])):.3f} Hz, "
          f"{same} of {periods} windows identical, mean prompt {gp / op - 1:+.2e}, mean data prompt {gq / oq - 1:+.2e}")
    assert ratio < 2e-2
    assert np.max(np.abs(gd[50:] - od[50:])) < 1.5
    assert same >= 0.9 * periods
    assert abs(gp - op) < 0.01 * op and abs(gq - oq) < 0.01 * oq


# ---- the true GPS L5 shape -------------------------------------------------------------------------------------------------------------------------------------
def test_true_gps_l5_shape(gpu):
    """L5Q / L5I of PRN 5 (tests/golden/codes_e1_l5.npz): 10230 chips at 10.23 Mcps on 1176.45 MHz, 25 Msps, 25000 samples per period, NH20 on the pilot and NH10
    on the data component: two tables of 10230 floats -- more than 64 KiB of dynamic LDS -- beside the three-tap accumulators"""
    from gnss_sdr_amd.tracking_loop import set_symbol_sync, trk_conf
    g = golden_e1_l5_codes()
    k, periods, first = 4, 150, 3
    fs, chip_rate, carrier = 25e6, 10.23e6, 1176.45e6
    bits = cases.secondary_case_bits("l5_pilot")
    x, n = cases.pilot_data_with_secondary_codes(periods, fs, g["l5q"][k], g["l5i"][k], cases.SECONDARY_CASE_DOPPLER_HZ, bits, cases.GPS_L5Q_NH_CODE,
                                                 cases.GPS_L5I_NH_CODE, 10, first=first, chip_rate=chip_rate, carrier_hz=carrier, seed=19)
    assert n == 25000
    kw = cases.secondary_case_kw("l5_pilot", fs=fs, vector_length=n, code_chip_rate=chip_rate, signal_carrier_freq=carrier, code_length_chips=10230)
    conf_o = oracle.trk_conf(**kw)
    oracle.set_symbol_sync(conf_o, 10, cases.GPS_L5Q_NH_CODE, has_secondary=True, data_secondary_code=cases.GPS_L5I_NH_CODE)
    ora = oracle.trk_run(conf_o, g["l5q"][k], x, 0, 0, cases.SECONDARY_CASE_HANDOVER_HZ, periods, data_code=g["l5i"][k], pull_in_over=True)
    states = [r.state for r in ora]
    assert len(ora) == periods and states.index(4) == first + 20 and not any(r.flags & 2 for r in ora)
    conf = trk_conf(**kw)
    set_symbol_sync(conf, 10, cases.GPS_L5Q_NH_CODE, has_secondary=True, data_secondary_code=cases.GPS_L5I_NH_CODE)
    rec = _launched(gpu, conf, x, g["l5q"][k], g["l5i"][k], [periods], max_len=10230)
    _hold_to_the_oracle(rec, ora, "true GPS L5 shape", True)
