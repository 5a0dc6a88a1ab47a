// The two scalar functions of the non-coherent output channel of PR-GAMP (csrc/ace_prgamp.hip), usable from host and
// device code so that a host program can check them (tests/test_bessel_host.py):
//   bessel_log_i0e(x)   log(besseli(0, x, 1)) = log(I0(|x|) exp(-|x|)), the Bessel term of ncCAwgnEstimOut.logScale;
//   bessel_i1i0_amos(B) min(B / sqrt(B^2 + 4), B / (0.5 + sqrt(B^2 + 0.25))), the two upper bounds of Amos for
//                       I1(B) / I0(B) as ncCAwgnEstimOut.estim:61-62 combines them.
//
// log I0e, three branches in a = |x| (crossovers ACE_BESSEL_X1 = 1 and ACE_BESSEL_X2 = 20):
//   a < 1          log1p(S) - a with S = sum_{k >= 1} (a^2 / 4)^k / (k!)^2: near 0 the value is -a + a^2 / 4 - ..., and
//                  neither term is formed from a number near 1, so nothing cancels (log(I0e) would lose the a^2 / 4);
//   1 <= a < 20    log(exp(-a) (1 + S)): the product lies in [0.08, 0.47], so the large log I0(a) ~ a is never formed
//                  (its half ulp alone would be 16 u at a = 20); every term of S is positive;
//   a >= 20        -log(2 pi a) / 2 + log1p(sum_{k >= 1} c_k / a^k), c_k = c_{k-1} (2k - 1)^2 / (8 k): Hankel's
//                  expansion, summed until a term no longer changes the sum (its smallest term is about exp(-2 a),
//                  4e-18 at the crossover).  No exp: nothing overflows, a = inf gives -inf as the reference's log(0).
// NaN stays NaN.
#ifndef ACE_BESSEL_HPP_
#define ACE_BESSEL_HPP_

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ACE_BESSEL_HD __host__ __device__
#else
#define ACE_BESSEL_HD
#endif

#define ACE_BESSEL_X1 1.0
#define ACE_BESSEL_X2 20.0

namespace ace {

ACE_BESSEL_HD inline double bessel_log_i0e(double x) {
    const double a = fabs(x);
    if (!(a < ACE_BESSEL_X2)) {
        if (!(a == a)) return a;   // NaN
        double s = 0.0, term = 1.0;
        for (int k = 1; k <= 64; ++k) {
            const double f = (double)((2 * k - 1) * (2 * k - 1)) / ((double)(8 * k) * a);
            if (!(f < 1.0)) break;   // (past the smallest term; not reached for a >= 20 before the sum has settled)
            term *= f;
            const double sn = s + term;
            if (sn == s) break;
            s = sn;
        }
        return log1p(s) - 0.5 * log(6.283185307179586476925286766559 * a);
    }
    const double t = 0.25 * a * a;
    double s = 0.0, term = 1.0;
    for (int k = 1; k <= 80; ++k) {
        term *= t / (double)(k * k);
        const double sn = s + term;
        if (sn == s) break;
        s = sn;
    }
    if (a < ACE_BESSEL_X1) return log1p(s) - a;
    return log(exp(-a) * (1.0 + s));
}

ACE_BESSEL_HD inline double bessel_i1i0_amos(double B) {
    const double b2 = B * B;
    const double q1 = B / sqrt(b2 + 4.0);
    const double q2 = B / (0.5 + sqrt(b2 + 0.25));
    return q2 < q1 ? q2 : q1;   // min(q1, q2); NaN stays NaN
}

}  // namespace ace

#endif  // ACE_BESSEL_HPP_
