// Host build of gnss-sdr_amd/csrc/array_weights.h for tests/test_array_weights_host.py, tests/test_beam_adaptive_abi.py and the predictions of
// tests/test_beam_adaptive_gpu.py: the header's functions as they are, on caller-owned memory (tests/aw_host.py mirrors the structures).
#include "array_weights.h"
#include "gnss_sdr_hip.h"

extern "C"
{
    int gsh_test_aw_state_bytes() { return static_cast<int>(sizeof(gsh::AwState)); }
    int gsh_test_aw_conf_bytes() { return static_cast<int>(sizeof(gsh::AwConf)); }
    int gsh_test_beam_adapt_bytes() { return static_cast<int>(sizeof(gsh_beam_adapt)); }
    int gsh_test_beam_adapt_state_bytes() { return static_cast<int>(sizeof(struct gsh_beam_adapt_state)); }

    // R_acc <- lambda R_acc + R_block over the upper triangle (2 P doubles each)
    void gsh_test_aw_accumulate(int A, double lambda, const double* block, double* acc) { gsh::aw_accumulate(A, lambda, block, acc); }

    // one beam from an upper triangle: the loading, the factorisation and the solve.  v: A x (re, im) FP64; w: A x (re, im) float32, written only on
    // success (the caller's weights stay on a failure, as in a call).  Returns 1 on success.
    int gsh_test_aw_weights(int A, const double* acc, double loading_rel, double loading_abs, const double* c_iq, double* delta, double* v_iq, float* w_iq)
    {
        bool ok = true;
        for (int p = 0; p < A * (A + 1); p++) ok = ok && gsh::aw_finite(acc[p]);
        *delta = gsh::aw_loading(A, acc, loading_rel, loading_abs);
        double l_re[gsh::AW_MAX * gsh::AW_MAX], l_im[gsh::AW_MAX * gsh::AW_MAX], d[gsh::AW_MAX];
        ok = gsh::aw_factor(A, acc, *delta, l_re, l_im, d) && ok;
        double c[gsh::AW_MAX][2], v[gsh::AW_MAX][2];
        float w[gsh::AW_MAX][2];
        for (int a = 0; a < A; a++)
            {
                c[a][0] = c_iq[2 * a];
                c[a][1] = c_iq[2 * a + 1];
            }
        ok = gsh::aw_solve(A, l_re, l_im, d, c, v, w) && ok;
        for (int a = 0; a < A; a++)
            for (int q = 0; q < 2; q++)
                {
                    v_iq[2 * a + q] = v[a][q];
                    if (ok) w_iq[2 * a + q] = w[a][q];
                }
        return ok ? 1 : 0;
    }

    // a whole call on a caller-owned state
    int gsh_test_aw_step(int A, int n_beams, const gsh::AwConf* conf, const double* block, int reset, gsh::AwState* s)
    {
        return gsh::aw_step(A, n_beams, *conf, block, reset != 0, s) ? 1 : 0;
    }
}
