"""kf_tracking (kf.cc = src/algorithms/tracking/gnuradio_blocks/kf_tracking.cc) as a Python model: the checker of the device's Kalman loop.

The reference block cannot be compiled for the tests (its Armadillo algebra has no stand-in among the oracle's shims), so -- like tests/packed_reference.py for
the packed formats -- this is a RESTATEMENT with line citations, not the reference's code: the Kalman loop's parity with the reference is unpinned.
Built from the oracle's pieces: oracle.mcorr (the correlator), the oracle's discriminators (oracle_pll_*_atan, oracle_dll_nc_*), cn0_m2m4_estimator,
carrier_lock_detector, the Exponential_Smoother and the HistogramBitSynchronizer behind oracle.smoother_run / oracle.bit_sync_run (used statefully here, one
call per period).  The Kalman step itself goes through the HOST BUILD of gnss-sdr_amd/csrc/kalman_step.h (kf_host.HostKalman): the device compiles the same
text, so the comparison on the GPU is step for step, and tests/test_kalman_step_host.py holds that text to numpy's evaluation of the matrix expressions.

kf.cc against dll_pll_veml_tracking.cc (trk.cc), function by function -- where the shared machinery differs:
  * start_tracking / pull-in (kf.cc:680-860, 1740-1778): the same hand-over; plus init_kf(0.0, acq Doppler) (:1772).  d_carrier_phase_step_rad has no
    d_cfo_frequency_hz term anywhere (:1265).
  * cn0_and_tracking_lock_status (kf.cc:1040-1098 / trk.cc:1167-1224): identical text -- prompt buffer, M2M4 estimate, both smoothers, both fail counters,
    carrier_lock_detector(buffer, 1); d_CN0_SNV_dB_Hz is a double member there (kf_tracking.h:185) fed from the float smoother.
  * acquire_secondary (kf.cc:991-1033 / trk.cc:1118-1160): identical.
  * save_correlation_results (kf.cc:1330-1440 / trk.cc:1486-1596): identical (secondary-code wipe, data-symbol accumulation, d_cloop per track_pilot).
  * do_correlation_step (kf.cc:1105-1140 / trk.cc:1232-1257): identical.
  * the state switch, general_work (kf.cc:1690-2060 / trk.cc:1898-2290):
      state 2: run_Kf() where trk.cc has run_dll_pll(); at the switch to state 3 update_kf_narrow_integration_time() (:1891) where trk.cc re-parameterises
               its loop filters, called BEFORE d_trk_parameters.spc takes the narrow spacing (:1899, 1911); no Doppler correction.
      state 3: run_Kf is commented out (:1925); update_tracking_vars() runs on the frozen NCO commands, as in trk.cc.
      state 4: update_kf_cn0(d_CN0_SNV_dB_Hz) before every run_Kf() (:1973-1974).
  * update_tracking_vars (kf.cc:1251-1327 / trk.cc:1409-1483): code frequency and Doppler are the filter's; no frequency offset; d_acc_carrier_phase_rad
    takes the FLOAT remnant (:1297) where trk.cc subtracts the double product; d_rem_carr_phase_rad (a float, kf_tracking.h:204) is overwritten by the filter's
    carrier phase (:1215) before the remnant is added.  high_dyn (the smoother that overwrites x[3], :1269-1291) is not modelled.
  * log_data (kf.cc:1443-1539): see the record map in include/gnss_sdr_hip.h."""
import ctypes as C
import math

import numpy as np

import kf_host
import oracle
from gnss_sdr_amd._lib import TrkEpoch

TWO_PI = 2.0 * 3.1415926535898
f32 = np.float32


class _Smoother:
    def __init__(self, alpha, samples, min_value, offset):
        self.s = oracle.Smoother()
        self.L = oracle.lib()
        self.L.oracle_smoother_init(C.byref(self.s), alpha, samples, min_value, offset)

    def smooth(self, v):
        return float(self.L.oracle_smoother_smooth(C.byref(self.s), float(v)))


class _BitSync:
    def __init__(self, c):
        oracle.bit_sync_run(np.zeros(0, np.complex64), 1)  # (declares the argument types)
        self.L = oracle.lib()
        self.buf = C.create_string_buffer(1024)
        self.L.oracle_bit_sync_init(self.buf, c.symbols_per_bit, c.bs_min_events_for_lock, c.bs_stable_best_required, c.bs_dominance_ratio, c.bs_min_prompt_mag,
                                    c.bs_use_phase_dot_detector)

    def update(self, p):
        return self.L.oracle_bit_sync_update(self.buf, float(p.real), float(p.imag), 1)

    def until_next_edge(self):
        return self.L.oracle_bit_sync_epochs_until_next_edge(self.buf)


def _c64(re, im):
    return np.complex64(complex(float(re), float(im)))


class KfTrackingModel:
    """One channel.  conf: the gsh_trk_conf the device gets (gnss_sdr_amd.tracking_loop.trk_conf); perturb: relative size of a seeded perturbation of every
    correlator output (what test 5 of the issue measures its post-flip bars with), 0 = none."""

    def __init__(self, conf, code, x, start_sample, acq_sample_stamp, acq_doppler_hz, sd=kf_host.KF_DEFAULT_SD, data_code=None, perturb=0.0, perturb_seed=1):
        c = self.c = conf
        self.code = np.ascontiguousarray(code, f32)
        self.data_code = None if data_code is None else np.ascontiguousarray(data_code, f32)
        self.x = x
        self.perturb, self.rng = perturb, np.random.default_rng(perturb_seed)
        self.code_period = float(c.code_length_chips) / c.code_chip_rate
        self.kf = kf_host.HostKalman(self.code_period, acq_doppler_hz, sd, c.code_chip_rate, c.signal_carrier_freq)
        # start_tracking + the pull-in hand-over
        self.doppler = float(acq_doppler_hz)
        self.phase_step = TWO_PI * self.doppler / c.fs_in
        self.code_freq = c.code_chip_rate
        self.code_step = self.code_freq / c.fs_in
        self.rem_code_samples = self.rem_code_chips = 0.0
        self.acc_phase = 0.0
        self.rem_carr = f32(0.0)
        self.pos, self.acq_stamp, self.active = int(start_sample), int(acq_sample_stamp), True
        f = int(c.fs_in)
        self.pull_in_limit = (c.pull_in_time_s + 1) * f
        self.bit_sync_limit = (c.bit_synchronization_time_limit_s + 1) * f if (c.enable_bit_sync_time_limit and c.enable_symbol_sync) else None
        # lock detectors
        self.prompt_buffer = np.zeros(max(1, c.cn0_samples), np.complex64)
        self.cn0_counter = 0
        self.cn0_db_hz, self.carrier_lock_test = 0.0, 1.0
        self.code_fails = self.carr_fails = 0
        self.pull_in_latched = True
        cn0_init = c.cn0_smoother_samples // int(self.code_period * 1000.0)
        self.cn0_smoother = _Smoother(c.cn0_smoother_alpha, cn0_init, 25.0, 12.0)
        self.lock_smoother = _Smoother(c.carrier_lock_test_smoother_alpha, c.carrier_lock_test_smoother_samples, -1.0, 0.0)
        # symbol synchronisation
        self.state, self.cloop = 2, c.cloop
        self.ring = []
        self.current_symbol = self.current_data_symbol = 0
        self.flag_pll_180 = False
        self.acc_phase_initialized = False
        self.p_data_accu = _c64(0, 0)
        self.nt = 5 if c.veml else 3
        self.accv = np.zeros(self.nt, np.complex64)
        self.ext_count, self.narrow, self.spc_now, self.corr_time = 0, False, float(c.spc), 0.0
        self.use_hist = bool(c.enable_symbol_sync and c.use_histogram_bit_sync and not c.has_secondary and c.symbols_per_bit > 1)
        self.bs = _BitSync(c) if self.use_hist else None
        self.bs_epochs, self.bs_target, self.wait_for_bit_edge = 0, 0, False

    # ---- one period
    def _taps(self):
        c, spcf = self.c, f32(self.c.code_samples_per_chip)
        el = f32(c.early_late_space_narrow_chips if self.narrow else c.early_late_space_chips) * spcf
        vel = f32(c.very_early_late_space_narrow_chips if self.narrow else c.very_early_late_space_chips) * spcf
        return np.array([-vel, -el, 0.0, el, vel], f32) if c.veml else np.array([-el, 0.0, el], f32)

    def _lock_status(self, P, coh_time, pull_in, run_state):
        """cn0_and_tracking_lock_status, kf.cc:1040-1098: False = loss of lock"""
        c, ns = self.c, self.c.cn0_samples
        if self.pull_in_latched and not pull_in:  # kf.cc:1700-1706
            self.pull_in_latched = False
            self.code_fails = self.carr_fails = 0
        if self.bit_sync_limit is not None and run_state == 2 and (self.pos - self.acq_stamp) >= self.bit_sync_limit:
            self.carr_fails = 300000
        if self.cn0_counter < ns:
            self.prompt_buffer[self.cn0_counter] = P
            self.cn0_counter += 1
            return True
        self.prompt_buffer[self.cn0_counter % ns] = P
        self.cn0_counter += 1
        coh = f32(coh_time)
        raw = -100.0 if coh == 0.0 else oracle.cn0_m2m4_estimator(self.prompt_buffer, float(coh))
        self.cn0_db_hz = self.cn0_smoother.smooth(raw)
        self.carrier_lock_test = self.lock_smoother.smooth(oracle.carrier_lock_detector(self.prompt_buffer, 1))
        if not pull_in:
            if self.carrier_lock_test < c.carrier_lock_th:
                self.carr_fails += 1
            elif self.carr_fails > 0:
                self.carr_fails -= 1
            if self.cn0_db_hz < float(c.cn0_min):
                self.code_fails += 1
            elif self.code_fails > 0:
                self.code_fails -= 1
        if self.carr_fails > c.max_carrier_lock_fail or self.code_fails > c.max_code_lock_fail:
            self.carr_fails = self.code_fails = 0
            return False
        return True

    def step(self):
        c, L = self.c, oracle.lib()
        n = c.vector_length
        if not self.active or self.pos + n > len(self.x):
            return None
        r = TrkEpoch()
        spcf = f32(c.code_samples_per_chip)
        kw = dict(rem_carr=float(self.rem_carr), phase_step=float(f32(self.phase_step)), rem_code=float(f32(self.rem_code_chips) * spcf),
                  code_step=float(f32(self.code_step) * spcf))
        win = self.x[self.pos:self.pos + n]
        out = oracle.mcorr(self.code, self._taps(), win, **kw).copy()
        pdata = oracle.mcorr(self.data_code, np.zeros(1, f32), win, **kw)[0] if c.track_pilot else _c64(0, 0)
        if self.perturb:
            g = self.rng.standard_normal(2 * self.nt)
            out = (out.real * (1.0 + self.perturb * g[0::2])).astype(f32) + 1j * (out.imag * (1.0 + self.perturb * g[1::2])).astype(f32)
            out = out.astype(np.complex64)
        pull_in = (self.pos - self.acq_stamp) < self.pull_in_limit
        run_state = self.state if c.enable_symbol_sync else 0
        extend = c.extend_correlation_symbols if (c.enable_symbol_sync and c.extend_correlation_symbols > 1) else 1
        PR = self.nt // 2
        acc = out.copy()
        if run_state in (3, 4):  # save_correlation_results, kf.cc:1330-1440
            sgn = f32(1.0)
            if c.has_secondary:
                sgn = f32(1.0 if c.secondary_code[self.current_symbol] == ord("0") else -1.0)
                self.current_symbol = (self.current_symbol + 1) % c.secondary_code_length
            acc = np.array([_c64(f32(a.real) + sgn * f32(o.real), f32(a.imag) + sgn * f32(o.imag)) for a, o in zip(self.accv, out)], np.complex64)
            self.accv = acc.copy()
            pd = pdata if c.track_pilot else out[PR]
            if c.symbols_per_bit > 1:
                ds = f32(1.0)
                if c.data_secondary_code_length > 0:
                    ds = f32(1.0 if c.data_secondary_code[self.current_data_symbol] == ord("0") else -1.0)
                    self.current_data_symbol = (self.current_data_symbol + 1) % c.data_secondary_code_length
                else:
                    self.current_data_symbol = (self.current_data_symbol + 1) % c.symbols_per_bit
                self.p_data_accu = _c64(f32(self.p_data_accu.real) + ds * f32(pd.real), f32(self.p_data_accu.imag) + ds * f32(pd.imag))
            else:
                self.p_data_accu = np.complex64(pd)
            self.cloop = 0 if c.track_pilot else 1
        P = acc[PR]
        for t in range(self.nt):
            r.corr[2 * t], r.corr[2 * t + 1] = out[t].real, out[t].imag
            r.accu[2 * t], r.accu[2 * t + 1] = acc[t].real, acc[t].imag
        r.prompt_data[0], r.prompt_data[1] = pdata.real, pdata.imag
        r.sample_counter, r.state, r.flags = self.pos, run_state, 1 if pull_in else 0
        locked = True
        if c.enable_lock_detectors and run_state != 3:
            locked = self._lock_status(P, self.code_period * extend if run_state == 4 else self.code_period, pull_in, run_state)
        r.cn0_db_hz = self.cn0_db_hz if c.enable_lock_detectors else 0.0
        r.carrier_lock_test = self.carrier_lock_test if c.enable_lock_detectors else 0.0
        if not locked:  # kf.cc:1800-1805, 1966-1970
            r.flags |= 2
            self.active = False
            return r
        e_kf = 0.0
        if run_state != 3:  # run_Kf, kf.cc:1143-1218
            cloop = (self.cloop != 0) if c.enable_symbol_sync else (c.cloop != 0)
            atan = L.oracle_pll_cloop_two_quadrant_atan if cloop else L.oracle_pll_four_quadrant_atan
            carr_disc_hz = atan(float(P.real), float(P.imag)) / TWO_PI
            if c.veml:
                code_disc = L.oracle_dll_nc_vemlp_normalized(*[float(v) for a in (acc[0], acc[1], acc[3], acc[4]) for v in (a.real, a.imag)])
            else:
                spc = self.spc_now if (c.enable_symbol_sync and self.narrow) else c.spc
                code_disc = L.oracle_dll_nc_e_minus_l_normalized(float(acc[0].real), float(acc[0].imag), float(acc[2].real), float(acc[2].imag), spc, c.slope, c.y_intercept)
            if run_state == 4:
                self.kf.cn0(self.spc_now, self.cn0_db_hz)  # kf.cc:1973
            e_kf = self.kf.run(code_disc, carr_disc_hz)
            xk = self.kf.x
            self.doppler = float(xk[2])
            self.code_freq = c.code_chip_rate + self.doppler * c.code_chip_rate / c.signal_carrier_freq
            self.rem_code_samples += c.fs_in * e_kf / self.code_freq
            self.rem_carr = f32(xk[1])
            r.carr_phase_error_hz, r.code_error_chips, r.code_error_filt_chips = carr_disc_hz, code_disc, e_kf
            r.carr_error_filt_hz, r.carr_freq_error_hz = float(xk[2]), float(xk[3])
        # update_tracking_vars, kf.cc:1251-1327
        t_prn_samples = (1.0 / self.code_freq) * float(c.code_length_chips) * c.fs_in
        k_blk = t_prn_samples + self.rem_code_samples
        prn_len = int(math.floor(k_blk))
        self.phase_step = TWO_PI * self.doppler / c.fs_in
        remnant = f32(self.phase_step * float(prn_len) + 0.5 * 0.0 * float(prn_len) * float(prn_len))
        self.rem_carr = f32(f32(self.rem_carr) + remnant)
        self.rem_carr = f32(math.fmod(float(self.rem_carr), TWO_PI))
        self.acc_phase -= float(remnant)
        self.code_step = self.code_freq / c.fs_in
        self.rem_code_samples = k_blk - float(prn_len)
        self.rem_code_chips = self.code_freq * self.rem_code_samples / c.fs_in
        # the symbol machine, kf.cc:1807-1920 (state 2), :1921-1960 (state 3), :1976-2040 (state 4)
        sym_flags, rec_pdata = 0, _c64(0, 0)
        if c.enable_symbol_sync and run_state == 3:
            rec_pdata = self.p_data_accu
            if self.current_data_symbol == 0:
                sym_flags |= 1
                self.p_data_accu = _c64(0, 0)
            if self.flag_pll_180:
                sym_flags |= 2
            self.ext_count += 1
            if self.ext_count == extend - 1:
                self.ext_count, self.state = 0, 4
        elif c.enable_symbol_sync:
            if run_state == 2:
                next_state = False
                if not pull_in:
                    if not c.has_secondary and c.symbols_per_bit > 1 and self.use_hist:
                        lock_event = self.bs.update(out[PR])
                        self.bs_epochs += 1
                        k_now = self.bs_epochs - 1
                        if lock_event:
                            self.wait_for_bit_edge = True
                            wait = self.bs.until_next_edge() - 1
                            if wait < 0:
                                wait += c.symbols_per_bit
                            self.bs_target = k_now + wait
                        if self.wait_for_bit_edge and k_now == self.bs_target:
                            next_state, self.wait_for_bit_edge, self.use_hist = True, False, False
                    if not next_state and (c.has_secondary or c.symbols_per_bit > 1):
                        ln = c.secondary_code_length
                        self.ring.append(out[PR])
                        if len(self.ring) > ln:
                            self.ring.pop(0)
                        if ln > 0 and len(self.ring) == ln:  # acquire_secondary, kf.cc:991-1033
                            corr = 0
                            for i, p in enumerate(self.ring):
                                zero = c.secondary_code[i] == ord("0")
                                corr += (1 if zero else -1) if p.real < 0.0 else (-1 if zero else 1)
                            if abs(corr) == ln:
                                self.flag_pll_180 = corr < 0
                                next_state = True
                    if not c.has_secondary and not c.symbols_per_bit > 1:
                        next_state = True
                if next_state:
                    self.p_data_accu, self.ring = _c64(0, 0), []
                    self.current_symbol = self.current_data_symbol = 0
                    self.accv = np.zeros(self.nt, np.complex64)
                    if extend > 1:
                        self.ext_count = 0
                        self.corr_time = float(f32(extend) * f32(self.code_period))  # kf.cc:1882
                        self.state = 3
                        self.kf.narrow(extend, self.corr_time, c.spc, self.cn0_db_hz)  # :1891, before spc narrows
                        self.narrow, self.spc_now = True, float(c.early_late_space_narrow_chips)
                    else:
                        self.state = 4
            else:
                if not self.acc_phase_initialized:
                    self.acc_phase = -float(self.rem_carr)
                    self.acc_phase_initialized = True
                rec_pdata = self.p_data_accu
                if self.current_data_symbol == 0:
                    sym_flags |= 1
                    self.p_data_accu = _c64(0, 0)
                self.accv = np.zeros(self.nt, np.complex64)
                if extend > 1:
                    self.state = 3
            if self.flag_pll_180:
                sym_flags |= 2
        r.symbol_flags = sym_flags
        r.p_data_accu[0], r.p_data_accu[1] = rec_pdata.real, rec_pdata.imag
        r.prn_length_samples, r.rem_carr_phase_rad = prn_len, float(self.rem_carr)
        r.carrier_doppler_hz, r.code_freq_chips = self.doppler, self.code_freq
        r.rem_code_phase_samples, r.acc_carrier_phase_rad = self.rem_code_samples, self.acc_phase
        self.pos += prn_len
        return r

    def run(self, n_epochs):
        out = []
        for _ in range(n_epochs):
            r = self.step()
            if r is None:
                break
            out.append(r)
            if r.flags & 2:
                break
        return out
