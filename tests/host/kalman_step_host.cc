// Host build of gnss-sdr_amd/csrc/kalman_step.h for tests/test_kalman_step_host.py, tests/kf_reference.py and the replay test of
// tests/test_kf_tracking_gpu.py: the functions as they are, on a caller-owned gsh::KfState (mirrored field for field by kf_host.KfState).
#include "kalman_step.h"

extern "C"
{
    int gsh_test_kf_state_bytes() { return static_cast<int>(sizeof(gsh::KfState)); }

    void gsh_test_kf_init(gsh::KfState* s, const double* sd10, double code_chip_rate, double signal_carrier_freq, double Ti, double acq_code_phase_chips,
        double acq_doppler_hz)
    {
        gsh::kf_init(*s, sd10, gsh::kf_beta(code_chip_rate, signal_carrier_freq), Ti, acq_code_phase_chips, acq_doppler_hz);
    }

    double gsh_test_kf_run(gsh::KfState* s, double code_error_disc_chips, double carr_phase_error_disc_hz)
    {
        gsh::KfWork w;
        return gsh::kf_run(*s, w, code_error_disc_chips, carr_phase_error_disc_hz);
    }

    void gsh_test_kf_narrow(gsh::KfState* s, int extend_correlation_symbols, double Ti_new, float spc, double cn0_dbhz)
    {
        gsh::KfWork w;
        gsh::kf_narrow_integration_time(*s, w, extend_correlation_symbols, Ti_new, spc, cn0_dbhz);
    }

    double gsh_test_kf_exp10(double y) { return gsh::kf_exp10(y); }

    void gsh_test_kf_cn0(gsh::KfState* s, float spc, double cn0_dbhz) { gsh::kf_cn0(*s, spc, cn0_dbhz); }
}
