// Adaptive array weights from the accumulated covariance: the arithmetic of the beamformer's adaptive mode (gsh_adaptive_beam_set, include/gnss_sdr_hip.h),
// the definition itself.  Plain FP64 C++ that the device (beamformer.hip, one work-group) and the host (tests/host/array_weights_host.cc) both compile with
// -ffp-contract=off: no math-library call (hence no square root), one rounding per written operation, every sum in ascending index order -- a step replayed
// on the host from the same inputs is the device's, bit for bit.
//   R_acc <- lambda R_acc + R_block                    per real number of the upper triangle, one multiplication and one addition; diagonal: imaginary part 0
//   delta  = loading_rel * (sum_i Re R_acc[i][i]) / A + loading_abs,    M = R_acc + delta I
//   M = L D L^H                                        column by column, no pivoting (L unit lower triangular, D real)
//   per beam:  L y = c,  z = y / D,  L^H u = z,  d = sum_i conj(c_i) u_i,  v = u conj(d) / |d|^2,  w = conj(v) rounded once to float32
// c = steering vector: MVDR, v = R^-1 s / (s^H R^-1 s); c = unit vector of the reference element: power inversion, v[ref] = (1, 0) exactly (u conj(d) and
// |d|^2 are then the same products in the same order).
#ifndef GSH_ARRAY_WEIGHTS_H
#define GSH_ARRAY_WEIGHTS_H

#ifdef __HIPCC__
#define GSH_AW_FN __device__ __host__ inline
#else
#define GSH_AW_FN inline
#endif

namespace gsh
{
constexpr int AW_MAX = 8;                         // GSH_ARRAY_MAX_ANTENNAS = GSH_ARRAY_MAX_BEAMS
constexpr int AW_PAIRS = AW_MAX * (AW_MAX + 1) / 2;

// what an adaptive handle keeps in device memory between calls
struct AwState
{
    double r_acc[2 * AW_PAIRS];  // (re, im) of the upper triangle, row by row: pair (i, j), i <= j, at aw_pair(i, j, A)
    double delta;                // the loading of the last call
    unsigned long long blocks, failures;
    unsigned long long solved;   // a call has succeeded since the mode was set: w below are its (or a later call's) weights
    float w[AW_MAX][AW_MAX][2];  // [beam][antenna] (re, im): the weights in force
};

// what a call is configured with (gsh_beam_adapt, and the caller's fixed weights for the calls before the first success)
struct AwConf
{
    double forgetting, loading_rel, loading_abs;
    double c[AW_MAX][AW_MAX][2];
    float fixed_w[AW_MAX][AW_MAX][2];
};

GSH_AW_FN int aw_pair(int i, int j, int A) { return i * A - i * (i - 1) / 2 + (j - i); }
GSH_AW_FN bool aw_finite(double x) { return x - x == 0.0; }  // false for an infinity and for a NaN

// R_acc <- lambda R_acc + R_block for pair p of the upper triangle
GSH_AW_FN void aw_accumulate_pair(int A, int p, double lambda, const double* block, double* acc)
{
    int i = 0, first = 0;  // first: the index of row i's diagonal pair
    while (i < A - 1 && p >= first + (A - i))
        {
            first += A - i;
            i++;
        }
    const double re = lambda * acc[2 * p];
    acc[2 * p] = re + block[2 * p];
    if (p == first)
        acc[2 * p + 1] = 0.0;
    else
        {
            const double im = lambda * acc[2 * p + 1];
            acc[2 * p + 1] = im + block[2 * p + 1];
        }
}

GSH_AW_FN void aw_accumulate(int A, double lambda, const double* block, double* acc)
{
    for (int p = 0; p < A * (A + 1) / 2; p++) aw_accumulate_pair(A, p, lambda, block, acc);
}

GSH_AW_FN double aw_loading(int A, const double* acc, double loading_rel, double loading_abs)
{
    double trace = 0.0;
    for (int i = 0; i < A; i++) trace += acc[2 * aw_pair(i, i, A)];
    const double scaled = loading_rel * trace;
    const double mean = scaled / static_cast<double>(A);
    return mean + loading_abs;
}

// M = acc + delta I = L D L^H.  l_re / l_im: AW_MAX x AW_MAX, row-major, the strictly lower triangle is written; d: AW_MAX.  false: the call fails.
GSH_AW_FN bool aw_factor(int A, const double* acc, double delta, double* l_re, double* l_im, double* d)
{
    bool ok = aw_finite(delta);
    for (int j = 0; j < A; j++)
        {
            double dj = acc[2 * aw_pair(j, j, A)] + delta;
            for (int k = 0; k < j; k++)
                {
                    const double lr = l_re[j * AW_MAX + k], li = l_im[j * AW_MAX + k];
                    const double m2 = lr * lr + li * li;
                    dj = dj - m2 * d[k];
                }
            d[j] = dj;
            ok = ok && dj > 0.0 && aw_finite(dj);
            for (int i = j + 1; i < A; i++)
                {
                    // M[i][j] = conj(M[j][i]), i > j
                    double sr = acc[2 * aw_pair(j, i, A)], si = -acc[2 * aw_pair(j, i, A) + 1];
                    for (int k = 0; k < j; k++)
                        {
                            // L[i][k] conj(L[j][k]) D[k]
                            const double ar = l_re[i * AW_MAX + k], ai = l_im[i * AW_MAX + k];
                            const double br = l_re[j * AW_MAX + k], bi = l_im[j * AW_MAX + k];
                            const double pr = ar * br + ai * bi;
                            const double pi = ai * br - ar * bi;
                            sr = sr - pr * d[k];
                            si = si - pi * d[k];
                        }
                    const double qr = sr / dj, qi = si / dj;
                    l_re[i * AW_MAX + j] = qr;
                    l_im[i * AW_MAX + j] = qi;
                    ok = ok && aw_finite(qr) && aw_finite(qi);
                }
        }
    return ok;
}

// one beam's solve with the factors of aw_factor.  c: A x (re, im).  v: A x (re, im) in FP64 (may be null); w: A x (re, im), conj(v) in float32.
// false: the call fails (w and v hold what came out all the same: the caller keeps the old weights).
GSH_AW_FN bool aw_solve(int A, const double* l_re, const double* l_im, const double* d, const double (*c)[2], double (*v)[2], float (*w)[2])
{
    double ur[AW_MAX], ui[AW_MAX];
    // L y = c, forward
    for (int i = 0; i < A; i++)
        {
            double yr = c[i][0], yi = c[i][1];
            for (int k = 0; k < i; k++)
                {
                    const double ar = l_re[i * AW_MAX + k], ai = l_im[i * AW_MAX + k];
                    const double pr = ar * ur[k] - ai * ui[k];
                    const double pi = ar * ui[k] + ai * ur[k];
                    yr = yr - pr;
                    yi = yi - pi;
                }
            ur[i] = yr;
            ui[i] = yi;
        }
    // z = y / D
    for (int i = 0; i < A; i++)
        {
            ur[i] = ur[i] / d[i];
            ui[i] = ui[i] / d[i];
        }
    // L^H u = z, backward: u[i] = z[i] - sum_{k > i} conj(L[k][i]) u[k], k ascending
    for (int i = A - 1; i >= 0; i--)
        {
            double xr = ur[i], xi = ui[i];
            for (int k = i + 1; k < A; k++)
                {
                    const double ar = l_re[k * AW_MAX + i], ai = l_im[k * AW_MAX + i];
                    const double pr = ar * ur[k] + ai * ui[k];
                    const double pi = ar * ui[k] - ai * ur[k];
                    xr = xr - pr;
                    xi = xi - pi;
                }
            ur[i] = xr;
            ui[i] = xi;
        }
    // d = sum_i conj(c_i) u_i
    double dr = 0.0, di = 0.0;
    for (int i = 0; i < A; i++)
        {
            const double pr = c[i][0] * ur[i] + c[i][1] * ui[i];
            const double pi = c[i][0] * ui[i] - c[i][1] * ur[i];
            dr = dr + pr;
            di = di + pi;
        }
    const double n2 = dr * dr + di * di;
    bool ok = n2 > 0.0 && aw_finite(n2);
    // v = u conj(d) / |d|^2, w = conj(v)
    for (int i = 0; i < A; i++)
        {
            const double tr = ur[i] * dr + ui[i] * di;
            const double ti = ui[i] * dr - ur[i] * di;
            const double vr = tr / n2, vi = ti / n2;
            const float wr = static_cast<float>(vr), wi = static_cast<float>(-vi);
            ok = ok && aw_finite(ur[i]) && aw_finite(ui[i]) && aw_finite(vr) && aw_finite(vi) && aw_finite(static_cast<double>(wr)) &&
                 aw_finite(static_cast<double>(wi));
            if (v)
                {
                    v[i][0] = vr;
                    v[i][1] = vi;
                }
            w[i][0] = wr;
            w[i][1] = wi;
        }
    return ok;
}

// the end of a call: the counters and the weights in force, from the new weights of every beam and whether every step of every beam went through
GSH_AW_FN void aw_commit_counters(bool ok, AwState* s)
{
    s->blocks += 1;
    if (ok)
        s->solved = 1;
    else
        s->failures += 1;
}

// A whole call as one lane would run it (the device shares the factorisation between its lanes: the same functions, the same bits).
// block: the block's covariance, upper triangle as r_acc.  reset: the mode was set since the last call.  true: the call succeeded.
GSH_AW_FN bool aw_step(int A, int n_beams, const AwConf& conf, const double* block, bool reset, AwState* s)
{
    if (reset)
        {
            for (int p = 0; p < 2 * AW_PAIRS; p++) s->r_acc[p] = 0.0;
            s->blocks = s->failures = s->solved = 0;
        }
    aw_accumulate(A, conf.forgetting, block, s->r_acc);
    bool ok = true;
    for (int p = 0; p < A * (A + 1); p++) ok = ok && aw_finite(s->r_acc[p]);
    const double delta = aw_loading(A, s->r_acc, conf.loading_rel, conf.loading_abs);
    s->delta = delta;
    double l_re[AW_MAX * AW_MAX], l_im[AW_MAX * AW_MAX], d[AW_MAX];
    ok = aw_factor(A, s->r_acc, delta, l_re, l_im, d) && ok;
    float w[AW_MAX][AW_MAX][2];
    for (int b = 0; b < n_beams; b++) ok = aw_solve(A, l_re, l_im, d, conf.c[b], nullptr, w[b]) && ok;
    const bool had = s->solved != 0;
    aw_commit_counters(ok, s);
    for (int b = 0; b < n_beams; b++)
        for (int a = 0; a < A; a++)
            for (int q = 0; q < 2; q++)
                {
                    if (ok)
                        s->w[b][a][q] = w[b][a][q];
                    else if (!had)
                        s->w[b][a][q] = conf.fixed_w[b][a][q];
                }
    return ok;
}
}  // namespace gsh

#endif  // GSH_ARRAY_WEIGHTS_H
