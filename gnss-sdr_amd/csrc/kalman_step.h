// The arithmetic core of gnss-sdr's kf_tracking (kf.cc = src/algorithms/tracking/gnuradio_blocks/kf_tracking.cc), restated in FP64 as plain C++: the same text
// runs on one lane of the closed tracking loop (tracking_loop.hip, the Kalman flavour of trk_loop_kernel) and -- for tests/test_kalman_step_host.py and as the
// step of tests/kf_reference.py -- on the host, with -ffp-contract=off on both sides (the pattern of exact_division.h).
//   kf_init                    init_kf                              kf.cc:871-909
//   kf_narrow_integration_time update_kf_narrow_integration_time    kf.cc:912-949
//   kf_cn0                     update_kf_cn0                        kf.cc:952-969
//   kf_run                     run_Kf, from "Kalman loop" on        kf.cc:1168-1217
//   kf_beta                    d_beta                               kf.cc:456-463
// State x = [code phase (chips), carrier phase (rad), Doppler (Hz), Doppler rate (Hz/s)]; P, Q 4 x 4 row-major, R 2 x 2 diagonal (kept as its two entries).
// F and H are functions of Ti = d_current_correlation_time_s and beta alone and every function that uses them rebuilds them from the Ti it was given last
// (the reference keeps d_F / d_H and rebuilds them in the same three places), so the block keeps Ti, not the matrices:
//   F = [1 0 beta Ti  beta Ti^2 / 2]      H = [1 0 -beta Ti / 2  beta Ti^2 / 6]
//       [0 1 2 pi Ti  pi Ti^2      ]          [0 1 -pi Ti        pi Ti^2 / 3  ]
//       [0 0 1        Ti           ]
//       [0 0 0        1            ]
// ORDER OF OPERATIONS.  The reference evaluates its matrix expressions with Armadillo, whose order of summation (and whether it calls a BLAS) is not fixed by
// its text.  Here every product is written out with the structure exploited -- a structural zero contributes no term, a structural one no multiplication --
// and every sum runs over the inner index in ascending order, left to right, as written below; (F P) F^T is evaluated as F P first, then times F^T;
// P^- H^T first, then H (P^- H^T); the 2 x 2 inverse is the closed form adj(S) / det(S), each entry divided by the determinant; K H first, then
// (I - K H) P^-, whose sum runs over all four inner indices.  P is NOT symmetrised: the reference does not.  No math-library call: the one pow() of the
// C/N0-to-linear conversion is written out too (kf_exp10).
// Intermediate matrices live in a caller-supplied work block (LDS on the device): one lane walks through them row by row with a handful of live values, which
// is what lets the flavour share a 128-register budget with the correlator.
#ifndef GSH_KALMAN_STEP_H
#define GSH_KALMAN_STEP_H

#ifdef __HIPCC__
#define GSH_KF_FN __device__ __host__ inline __attribute__((always_inline))
#else
#define GSH_KF_FN inline
#endif
// the end of a stage: what it left in the work block is re-read by the next one (bounds the live values; no effect on the arithmetic)
#define GSH_KF_STAGE() asm volatile("" ::: "memory")

namespace gsh
{
constexpr double KF_GNSS_PI = 3.1415926535898;  // src/core/system_parameters/MATH_CONSTANTS.h:47
constexpr double KF_TWO_PI = 2.0 * KF_GNSS_PI;  // :49

struct KfState  // per channel, resident in device memory between launches
{
    double x[4];   // d_x_old_old
    double P[16];  // d_P_old_old
    double Q[16];  // d_Q
    double R[2];   // d_R's diagonal
    double Ti;     // the d_current_correlation_time_s d_F and d_H were last built with
    double beta;   // d_beta
    double code_error_kf_chips;  // d_code_error_kf_chips
    double pad_;
};
struct KfWork  // intermediates of one step
{
    double xm[4];   // d_x_new_old
    double Pm[16];  // d_P_new_old
    double A[16];   // F P; later I - K H
    double B[8];    // P^- H^T (4 x 2)
    double K[8];    // the gain (4 x 2)
};
struct KfCoef
{
    double f02, f03, f12, f13, f23, h02, h03, h12, h13;
};

GSH_KF_FN double kf_beta(double code_chip_rate, double signal_carrier_freq)  // kf.cc:456-463
{
    return signal_carrier_freq > 1.0 ? code_chip_rate / signal_carrier_freq : 0.0;
}

GSH_KF_FN KfCoef kf_coef(double beta, double Ti)  // kf.cc:877-883 (= :929-935, :958-959)
{
    const double TiTi = Ti * Ti;
    KfCoef c;
    c.f02 = beta * Ti;
    c.f03 = beta * TiTi / 2.0;
    c.f12 = 2.0 * KF_GNSS_PI * Ti;
    c.f13 = KF_GNSS_PI * TiTi;
    c.f23 = Ti;
    c.h02 = -beta * Ti / 2.0;
    c.h03 = beta * TiTi / 6.0;
    c.h12 = -KF_GNSS_PI * Ti;
    c.h13 = KF_GNSS_PI * TiTi / 3.0;
    return c;
}

// out = F M F^T (+ Qadd when given), A: 16 doubles of work.  M and out may be the same matrix.
GSH_KF_FN void kf_fmft(const KfCoef& c, const double* M, const double* Qadd, double* A, double* out)
{
    for (int j = 0; j < 4; j++)  // A = F M
        {
            const double m2 = M[8 + j], m3 = M[12 + j];
            A[j] = (M[j] + c.f02 * m2) + c.f03 * m3;
            A[4 + j] = (M[4 + j] + c.f12 * m2) + c.f13 * m3;
            A[8 + j] = m2 + c.f23 * m3;
            A[12 + j] = m3;
            GSH_KF_STAGE();
        }
    for (int i = 0; i < 4; i++)  // out = A F^T + Qadd
        {
            const double a0 = A[4 * i], a1 = A[4 * i + 1], a2 = A[4 * i + 2], a3 = A[4 * i + 3];
            double o0 = (a0 + a2 * c.f02) + a3 * c.f03;
            double o1 = (a1 + a2 * c.f12) + a3 * c.f13;
            double o2 = a2 + a3 * c.f23;
            double o3 = a3;
            if (Qadd != nullptr)
                {
                    o0 = o0 + Qadd[4 * i];
                    o1 = o1 + Qadd[4 * i + 1];
                    o2 = o2 + Qadd[4 * i + 2];
                    o3 = o3 + Qadd[4 * i + 3];
                }
            out[4 * i] = o0;
            out[4 * i + 1] = o1;
            out[4 * i + 2] = o2;
            out[4 * i + 3] = o3;
            GSH_KF_STAGE();
        }
}

// 10^y, the one transcendental of the block (CN0_lin = pow(10.0, cn0 / 10.0), kf.cc:938, :962), written out so that host and device evaluate the same
// operations -- the device library's pow() alone needs more registers than the loop kernel has left (it put the flavour into scratch) and would make R the one
// quantity the host build cannot reproduce.  y log2(10) = n + f with n integral and |f| <= 1/2 (log2(10) split into two doubles, the product's low part
// recovered with one explicit FMA), 2^f = exp(f ln 2) by its Taylor series to degree 13 in Horner form (|f ln 2| <= 0.35: the first neglected term is below
// 5e-18), scaled by 2^n.  Rounding: f ln 2 and the last Horner steps, about 2 ulp in all (tests/test_kalman_step_host.py holds it to 4 ulp of the correctly
// rounded power over -20 .. 80 dB-Hz).  For |y| < 300.
GSH_KF_FN double kf_exp10(double y)
{
    constexpr double LOG2_10_HI = 3.321928094887362, LOG2_10_LO = 1.661617516973592e-16, LN_2 = 0.6931471805599453;
    const double n = __builtin_rint(y * LOG2_10_HI);
    const double f = __builtin_fma(y, LOG2_10_HI, -n) + y * LOG2_10_LO;
    const double u = f * LN_2;
    double p = 1.0 / 6227020800.0;  // 1 / 13!
    p = p * u + 1.0 / 479001600.0;
    p = p * u + 1.0 / 39916800.0;
    p = p * u + 1.0 / 3628800.0;
    p = p * u + 1.0 / 362880.0;
    p = p * u + 1.0 / 40320.0;
    p = p * u + 1.0 / 5040.0;
    p = p * u + 1.0 / 720.0;
    p = p * u + 1.0 / 120.0;
    p = p * u + 1.0 / 24.0;
    p = p * u + 1.0 / 6.0;
    p = p * u + 0.5;
    p = p * u + 1.0;
    p = p * u + 1.0;
    return __builtin_ldexp(p, static_cast<int>(n));
}

// d_R from a C/N0 [dB-Hz], kf.cc:938-944 = :962-968.  spc / (1 - spc) is the reference's (spc is a float there; it divides by zero for spc == 1 as written).
GSH_KF_FN void kf_r_from_cn0(KfState& s, double Ti, float spc, double cn0_dbhz)
{
    const double CN0_lin = kf_exp10(cn0_dbhz / 10.0);
    const double CN0_lin_Ti = CN0_lin * Ti;
    const double Sigma2_Phase = (1.0 / (2.0 * CN0_lin_Ti)) * (1.0 + 1.0 / (2.0 * CN0_lin_Ti));
    const double Sigma2_Tau = (1.0 / CN0_lin_Ti) * (spc + (spc / (1.0 - spc)) * (1.0 / (2.0 * CN0_lin_Ti)));
    s.R[0] = Sigma2_Tau;
    s.R[1] = Sigma2_Phase;
}

// init_kf(acq_code_phase_chips, acq_doppler_hz), kf.cc:871-909.  sd: the ten standard deviations in gsh_trk_kf_conf's order
// (code_disc, carrier_disc | code_phase, carrier_phase, carrier_freq, carrier_freq_rate | the same four, initial).  pow(sd, 2.0) is sd * sd, exactly.
GSH_KF_FN void kf_init(KfState& s, const double* sd, double beta, double Ti, double acq_code_phase_chips, double acq_doppler_hz)
{
    for (int i = 0; i < 16; i++) s.P[i] = s.Q[i] = 0.0;
    s.R[0] = sd[0] * sd[0];
    s.R[1] = sd[1] * sd[1];
    for (int i = 0; i < 4; i++)
        {
            s.Q[5 * i] = sd[2 + i] * sd[2 + i];
            s.P[5 * i] = sd[6 + i] * sd[6 + i];
        }
    s.x[0] = acq_code_phase_chips;
    s.x[1] = 0.0;
    s.x[2] = acq_doppler_hz;
    s.x[3] = 0.0;
    s.Ti = Ti;
    s.beta = beta;
    s.code_error_kf_chips = 0.0;
    s.pad_ = 0.0;
}

// update_kf_narrow_integration_time, kf.cc:912-949, at the entry to the extended integration (:1878-1891).  The loop is restated as written: every pass
// propagates d_Q through the OLD d_F (the one built with the Ti in force so far) and adds the result to Qnew, so Q becomes sum_{i=1..extend} F^i Q (F^i)^T;
// then F and H are rebuilt for Ti_new and R from the current C/N0.
GSH_KF_FN void kf_narrow_integration_time(KfState& s, KfWork& w, int extend_correlation_symbols, double Ti_new, float spc, double cn0_dbhz)
{
    const KfCoef c = kf_coef(s.beta, s.Ti);
    double* Qnew = w.Pm;
    for (int i = 0; i < 16; i++) Qnew[i] = 0.0;
    for (int n = 0; n < extend_correlation_symbols; n++)
        {
            kf_fmft(c, s.Q, nullptr, w.A, s.Q);                  // d_Q = d_F * d_Q * d_F.t()  (:921; the same product as the line above it)
            for (int i = 0; i < 16; i++) Qnew[i] = Qnew[i] + s.Q[i];  // Qnew += d_F * d_Q * d_F.t()  (:920)
            GSH_KF_STAGE();
        }
    for (int i = 0; i < 16; i++) s.Q[i] = Qnew[i];
    s.Ti = Ti_new;
    kf_r_from_cn0(s, Ti_new, spc, cn0_dbhz);
}

// update_kf_cn0, kf.cc:952-969: in state 4 before every run_Kf (:1973)
GSH_KF_FN void kf_cn0(KfState& s, float spc, double cn0_dbhz) { kf_r_from_cn0(s, s.Ti, spc, cn0_dbhz); }

// run_Kf from the prediction on, kf.cc:1168-1217.  z = [code discriminator (chips), carrier discriminator (Hz) * TWO_PI]: the reference divides its arctangent by
// TWO_PI (:1149, :1154) and multiplies back (:1176); the caller has done the division, the multiplication is here.  Returns d_code_error_kf_chips; x[0] is reset
// (:1185).  What the caller still does: d_code_freq_kf_chips_s (:1201), d_rem_code_phase_samples (:1214), d_rem_carr_phase_rad (:1215).
GSH_KF_FN double kf_run(KfState& s, KfWork& w, double code_error_disc_chips, double carr_phase_error_disc_hz)
{
    const KfCoef c = kf_coef(s.beta, s.Ti);
    // d_x_new_old = d_F * d_x_old_old
    {
        const double x2 = s.x[2], x3 = s.x[3];
        w.xm[0] = (s.x[0] + c.f02 * x2) + c.f03 * x3;
        w.xm[1] = (s.x[1] + c.f12 * x2) + c.f13 * x3;
        w.xm[2] = x2 + c.f23 * x3;
        w.xm[3] = x3;
    }
    // d_P_new_old = d_F * d_P_old_old * d_F.t() + d_Q
    kf_fmft(c, s.P, s.Q, w.A, w.Pm);
    // B = d_P_new_old * d_H.t()
    for (int i = 0; i < 4; i++)
        {
            const double p2 = w.Pm[4 * i + 2], p3 = w.Pm[4 * i + 3];
            w.B[2 * i] = (w.Pm[4 * i] + p2 * c.h02) + p3 * c.h03;
            w.B[2 * i + 1] = (w.Pm[4 * i + 1] + p2 * c.h12) + p3 * c.h13;
            GSH_KF_STAGE();
        }
    // S = d_H * B + d_R, its inverse in closed form, K = B * inv(S)
    {
        const double s00 = ((w.B[0] + c.h02 * w.B[4]) + c.h03 * w.B[6]) + s.R[0];
        const double s01 = (w.B[1] + c.h02 * w.B[5]) + c.h03 * w.B[7];
        const double s10 = (w.B[2] + c.h12 * w.B[4]) + c.h13 * w.B[6];
        const double s11 = ((w.B[3] + c.h12 * w.B[5]) + c.h13 * w.B[7]) + s.R[1];
        const double det = s00 * s11 - s01 * s10;
        const double i00 = s11 / det, i01 = -s01 / det, i10 = -s10 / det, i11 = s00 / det;
        for (int i = 0; i < 4; i++)
            {
                const double b0 = w.B[2 * i], b1 = w.B[2 * i + 1];
                w.K[2 * i] = b0 * i00 + b1 * i10;
                w.K[2 * i + 1] = b0 * i01 + b1 * i11;
            }
    }
    GSH_KF_STAGE();
    // d_x_new_new = d_x_new_old + K * z
    {
        const double z0 = code_error_disc_chips, z1 = carr_phase_error_disc_hz * KF_TWO_PI;
        for (int i = 0; i < 4; i++) s.x[i] = w.xm[i] + (w.K[2 * i] * z0 + w.K[2 * i + 1] * z1);
    }
    // d_P_new_new = (eye(4, 4) - K * d_H) * d_P_new_old
    for (int i = 0; i < 4; i++)
        {
            const double k0 = w.K[2 * i], k1 = w.K[2 * i + 1];
            w.A[4 * i] = (i == 0 ? 1.0 : 0.0) - k0;
            w.A[4 * i + 1] = (i == 1 ? 1.0 : 0.0) - k1;
            w.A[4 * i + 2] = (i == 2 ? 1.0 : 0.0) - (k0 * c.h02 + k1 * c.h12);
            w.A[4 * i + 3] = (i == 3 ? 1.0 : 0.0) - (k0 * c.h03 + k1 * c.h13);
            GSH_KF_STAGE();
        }
    for (int i = 0; i < 4; i++)
        {
            const double m0 = w.A[4 * i], m1 = w.A[4 * i + 1], m2 = w.A[4 * i + 2], m3 = w.A[4 * i + 3];
            for (int j = 0; j < 4; j++) s.P[4 * i + j] = ((m0 * w.Pm[j] + m1 * w.Pm[4 + j]) + m2 * w.Pm[8 + j]) + m3 * w.Pm[12 + j];
            GSH_KF_STAGE();
        }
    const double code_error_kf_chips = s.x[0];  // :1184-1185
    s.x[0] = 0.0;
    s.code_error_kf_chips = code_error_kf_chips;
    return code_error_kf_chips;
}
}  // namespace gsh

#endif
