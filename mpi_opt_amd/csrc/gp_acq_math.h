// Device arithmetic shared by the acquisition kernels (gp.hip, gp_ps.hip, gp_grad.h): scipy's
// ndtr, the normal pdf and the (value, index) order of the top-k lists and of the samplers'
// argmin (gp_joint.hip, gp_paths.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace mpo {

constexpr double kSqrt1_2 = 0.707106781186547524400844362104849039;
constexpr double kSqrt2Pi = 2.506628274631000502415765284811045253;

// scipy.special.ndtr, the kernel of scipy.stats.norm.cdf (skopt's EI / PI): cephes
// ndtr.c's own algorithm -- erf as x T(x^2) / U(x^2) for |x| <= 1, erfc as
// exp(-x^2) P(x) / Q(x) (1 <= x < 8) or R(x) / S(x) (x >= 8), Horner without FMA
// contraction as the host build evaluates it -- instead of the device libm's
// erf / erfc: with the same exp the results are scipy's bits (CPU check of these
// constants: 98.5% of 300k points bit-exact, the rest within 4.4e-16 relative).  The
// scoring pass times the same (1.40 vs 1.40 ms median, same box, profiles/r05/ei_ndtr_ab_ad.log).
namespace cephes {
__constant__ constexpr double kP[9] = {2.46196981473530512524E-10, 5.64189564831068821977E-1, 7.46321056442269912687E0,
                                       4.86371970985681366614E1,   1.96520832956077098242E2, 5.26445194995477358631E2,
                                       9.34528527171957607540E2,   1.02755188689515710272E3, 5.57535335369399327526E2};
__constant__ constexpr double kQ[8] = {1.32281951154744992508E1, 8.67072140885989742329E1, 3.54937778887819891062E2,
                                       9.75708501743205489753E2, 1.82390916687909736289E3, 2.24633760818710981792E3,
                                       1.65666309194161350182E3, 5.57535340817727675546E2};
__constant__ constexpr double kR[6] = {5.64189583547755073984E-1, 1.27536670759978104416E0, 5.01905042251180477414E0,
                                       6.16021097993053585195E0,  7.40974269950448939160E0, 2.97886665372100240670E0};
__constant__ constexpr double kS[6] = {2.26052863220117276590E0, 9.39603524938001434673E0, 1.20489539808096656605E1,
                                       1.70814450747565897222E1, 9.60896809063285878198E0, 3.36907645100081516050E0};
__constant__ constexpr double kT[5] = {9.60497373987051638749E0, 9.00260197203842689217E1, 2.23200534594684319226E3,
                                       7.00332514112805075473E3, 5.55923013010394962768E4};
__constant__ constexpr double kU[5] = {3.35617141647503099647E1, 5.21357949780152679795E2, 4.59432382970980127987E3,
                                       2.26290000613890934246E4, 4.92673942608635921086E4};
constexpr double kMaxLog = 7.09782712893383996843E2;

template <int N>
__device__ __forceinline__ double polevl(double x, const double (&c)[N]) {
#pragma clang fp contract(off)
    double y = c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) y = y * x + c[i];
    return y;
}
template <int N>   // leading coefficient 1
__device__ __forceinline__ double p1evl(double x, const double (&c)[N]) {
#pragma clang fp contract(off)
    double y = x + c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) y = y * x + c[i];
    return y;
}
// erf for |x| <= 1
__device__ __forceinline__ double erf_small(double x) {
#pragma clang fp contract(off)
    const double z = x * x;
    return x * polevl(z, kT) / p1evl(z, kU);
}
// erfc for x >= 1
__device__ __forceinline__ double erfc_large(double x) {
#pragma clang fp contract(off)
    const double z = -x * x;
    if (z < -kMaxLog) return 0.0;
    const double e = exp(z);
    const double y = x < 8.0 ? (e * polevl(x, kP)) / p1evl(x, kQ) : (e * polevl(x, kR)) / p1evl(x, kS);
    return y;
}
}  // namespace cephes

__device__ __forceinline__ double ndtr(double a) {
#pragma clang fp contract(off)
    if (isnan(a)) return a;
    const double x = a * kSqrt1_2;
    const double z = fabs(x);
    if (z < kSqrt1_2) return 0.5 + 0.5 * cephes::erf_small(x);
    // z >= sqrt(1/2); cephes erfc(z) takes its 1 - erf(z) branch below 1
    const double y = 0.5 * (z < 1.0 ? 1.0 - cephes::erf_small(z) : cephes::erfc_large(z));
    return x > 0.0 ? 1.0 - y : y;
}

__device__ __forceinline__ double norm_pdf(double x) { return exp(-x * x / 2.0) / kSqrt2Pi; }

// (value, index) lexicographic order: smaller value first, lower index on ties.
__device__ __forceinline__ bool lex_less(double v, long long i, double w, long long j) {
    return v < w || (v == w && i < j);
}

__device__ __forceinline__ void wave_lex_min(double& v, long long& i) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double w = __shfl_xor(v, off);
        long long j = __shfl_xor(i, off);
        if (lex_less(w, j, v, i)) { v = w; i = j; }
    }
}

}  // namespace mpo
