// gp.hip -- fp64 GP posterior + acquisition scoring for gfx950 (MI355X).
//
// Hot path G1-G4 of SURVEY §8a: the skopt "ask" step.  The reference reaches it
// through Coordinator.fit/ask (/root/reference/coordinator.py:63-79, 46-50) ->
// skopt.Optimizer -> GaussianProcessRegressor.predict + gaussian_ei/pi/lcb.
//
// Kernels
//   scale_rows_kernel    xs = X / ls (dims zero-padded to DP)
//   bc_*_kernel          blocked K = L L^T, W = L^-1, alpha (mpo_gp_prepare)
//   ap_*_kernel          rank-one append of one observation at fixed theta (mpo_gp_append)
//   chol_kernel          in-place lower Cholesky (one workgroup; mpo_chol_f64)
//   trsm_kernel          L X = B / L^T X = B, one thread per right-hand side (mpo_trsm_f64)
//   pack_wfrag_kernel    L^-1 -> MFMA B-fragment stream (lower triangle only)
//   gp_score_kernel      per 16/32/64-candidate block:
//                          phase 1 (VALU): K*[m][i] = Matern52 into LDS in MFMA
//                                          A-fragment order, mu partials
//                          phase 2 (MFMA): V = K* . L^-T on v_mfma_f64_16x16x4,
//                                          only the lower-triangular k-steps,
//                                          ||V_row||^2 accumulated in registers
//                          phase 3:        sd, mu, -EI/-PI/LCB, block top-k
//   gp_score_streamed_kernel  the same posterior for models whose K* tile does not
//                        fit the LDS (n <= 2048): K* one panel of observations at a
//                        time, later panels' partial rows in the score workspace
//   topk_merge_kernel    workgroup top-k lists -> global top-k (lowest index ties)
//   acq_grad_kernel      acquisition value + gradient at a few points (the polish objective),
//                        a caller of gp_grad.h's posterior_grad / acq_value_grad
//
// Why the triangular form: skopt evaluates sd^2 = amp - k^T K_inv k with an
// explicit K_inv (86 kFLOP/candidate at N=200, catastrophic cancellation);
// sd^2 = amp - ||L^-1 k||^2 is the same posterior with half the MFMA work and
// ~1000x less rounding error (DESIGN.md "GP posterior formulation").

#include "gp_grad.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

using mpo::kSqrt5;
using mpo::matern52;   // mpo_internal.h: shared with gp_joint.hip
using mpo::ndtr;       // gp_acq_math.h: shared with gp_ps.hip
using mpo::norm_pdf;
using mpo::lex_less;
using mpo::wave_lex_min;
constexpr double kJitter = 1e-10;
  // sklearn GPR alpha default (_gpr.py:207)

// exp(-k) for k >= 0 without the generic exp's special-case handling (k is a
// scaled distance: never negative, never NaN): Cody-Waite reduction
// -k = t ln2 + s, |s| <= ln2/2, with t = round(-k log2 e) from the 1.5*2^52
// rounding constant (no v_rndne), a degree-11 polynomial of e^s fitted at the
// Chebyshev nodes (8.6e-18 relative in exact arithmetic; 13 Taylor terms before),
// 2^t by ldexp from the saturating v_cvt_i32 of t: exp(-k) underflows to exactly
// 0 for every k past ~745 and stays finite for every k < ~1e20 (|xs| far beyond
// what a [0,1]-transformed space with skopt's length-scale bounds produces), so
// no clamp instruction is needed.  Within 2 ulp of exp(-k).
// a*b + c with the constant c read from an SGPR pair.  Written as plain fma the
// compiler keeps loop-invariant coefficients in VGPRs and turns each Horner step
// into v_mov_b64 + v_fmac_f64 (10 extra moves and 20 VGPRs per Matern).
__device__ __forceinline__ double fma_sc(double a, double b, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

__device__ __forceinline__ double exp_neg(double k) {
    constexpr double kRound = 6755399441055744.0;           // 1.5 * 2^52
    const double t = fma(k, -1.44269504088896340736, kRound) - kRound;
    double x = fma(t, -6.93147180369123816490e-01, -k);
    x = fma(t, -1.90821492927058770002e-10, x);
    double p = 2.511274345242859e-08;
    p = fma_sc(p, x, 2.76326459433635e-07);
    p = fma_sc(p, x, 2.755723242556338e-06);
    p = fma_sc(p, x, 2.4801485486569327e-05);
    p = fma_sc(p, x, 0.00019841269899541455);
    p = fma_sc(p, x, 0.0013888888952271288);
    p = fma_sc(p, x, 0.008333333333315002);
    p = fma_sc(p, x, 0.04166666666648857);
    p = fma_sc(p, x, 0.1666666666666669);
    p = fma_sc(p, x, 0.5000000000000018);
    p = fma(p, x, 1.0);
    p = fma(p, x, 1.0);
    return ldexp(p, (int)t);
}

// sqrt of r2 >= 1e-300 (the distance loops start their sum at 1e-300, so a zero
// distance never reaches v_rsq as 0) by v_rsq_f64, a Goldschmidt step and one
// Newton correction (ocml's sequence without its denormal scaling and 0/inf
// fix-ups).  Within 2 ulp; an ulp of r moves K* by <= 1e-14 relative.
__device__ __forceinline__ double sqrt_pos(double r2) {
    const double y = __builtin_amdgcn_rsq(r2);
    double s = r2 * y, h = 0.5 * y;
    const double e0 = fma(-h, s, 0.5);
    s = fma(s, e0, s);
    h = fma(h, e0, h);
    const double e1 = fma(-s, s, r2);
    return fma(e1, h, s);
}

// first term of every pairwise squared-distance sum (see sqrt_pos)
constexpr double kR2Floor = 1e-300;

// max(acc[r], kR2Floor) of an MFMA distance tile, one v_max_f64 per register with the
// floor in an SGPR pair.  fmax() compiles to two: it first canonicalises its argument
// (v_max x, x, x), which only matters for a signalling NaN, and an MFMA result never
// is one.  The bits are fmax's.  The compiler does not count inline asm among the
// VALU readers of an MFMA result, so the block carries the wait states itself: 19
// between a v_mfma_f64_16x16x4_f64 and the first VALU read of its result, what the
// compiler puts in front of fmax().
__device__ __forceinline__ void clamp_r2x4(f64x4 acc, double (&r2)[4]) {
    asm("s_nop 15\n\ts_nop 2" : "+v"(acc));   // tied to the whole result tuple: it stays behind the MFMAs
#pragma unroll
    for (int r = 0; r < 4; ++r) asm("v_max_f64 %0, %1, %2" : "=v"(r2[r]) : "v"(acc[r]), "s"(kR2Floor));
}

// The scoring kernel's Matern WITHOUT the ConstantKernel amplitude:
// (1 + k + k^2/3) exp(-k), k = sqrt(5 r2), k^2/3 = r2 * 5/3.  The kernel folds amp
// into mu (amp * K'.alpha) and into q (amp^2 ||L^-1 K'||^2): one multiply fewer per
// candidate-observation pair -- fp64 VALU and fp64 MFMA work do not overlap on
// gfx950 (scripts/probes/coexec.hip), so every VALU op per pair is kernel time.
__device__ __forceinline__ double matern52_unit(double r2) {
    const double k = sqrt_pos(r2) * kSqrt5;
    return fma(r2, 5.0 / 3.0, 1.0 + k) * exp_neg(k);
}

// Sum over the 16 lanes of a row group: with the f64 MFMA C/D map (col = lane & 15,
// row = (lane >> 4) + 4 r) the sum of a C register over the tile's 16 columns, for
// four registers at once (colsum16x4 below).
// The four steps are DPP moves of the two 32-bit halves (no LDS round trip) plus one
// v_add_f64 each: quad_perm [1,0,3,2] and [2,3,0,1] are lane ^ 1 and lane ^ 2 exactly.
// After them every quad is uniform, so row_half_mirror's lane 7 - i holds what lane
// i ^ 4 holds; after that step every group of 8 is uniform, so row_mirror's lane
// 15 - i holds what lane i ^ 8 holds.  fp64 addition is commutative: every lane adds
// the same two values as the xor butterfly (v += shfl_xor(v, 1 / 2 / 4 / 8)) did, and
// every bit of the sum is the butterfly's.  A DPP move reads nothing from a lane that
// EXEC masks off: the callers are wave-uniform code of kernels launched with whole
// 64-lane waves (both scoring kernels' mu / q folds).
template <int CTRL>
__device__ __forceinline__ double dpp_move_f64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// four registers folded step by step, so that the four chains interleave
__device__ __forceinline__ void colsum16x4(double (&v)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += dpp_move_f64<0xB1>(v[r]);    // quad_perm:[1,0,3,2]
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += dpp_move_f64<0x4E>(v[r]);    // quad_perm:[2,3,0,1]
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += dpp_move_f64<0x141>(v[r]);   // row_half_mirror
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += dpp_move_f64<0x140>(v[r]);   // row_mirror
}

// Rows [n, rows) of xs are zero padding (alpha and the L^-1 fragments are zero
// there): a scoring loop may run over whole 16-observation groups without bounds
// checks; the padding K* values are finite and contribute nothing.
constexpr int kXsPadRows = 32;   // rows = np16 + kXsPadRows: the scoring kernel reads one 16-row step past np16

__global__ void scale_rows_kernel(const double* __restrict__ X, int n, int rows, int d, int dp,
                                  const double* __restrict__ ls, double* __restrict__ xs,
                                  double* __restrict__ ls_pad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < rows * dp) {
        const int i = t / dp, c = t % dp;
        xs[t] = (c < d && i < n) ? X[(size_t)i * d + c] / ls[c] : 0.0;
    }
    if (ls_pad && t < dp) ls_pad[t] = t < d ? ls[t] : 1.0;
}

__global__ void zero_kernel(double* __restrict__ p, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = 0.0;
}

// MFMA form of the candidate-observation distance (gp_score_kernel<.., MD = 1>):
// xb row i = (-2 xs_i, 1, |xs_i|^2, 0 ...), so that [c, |c|^2, 1, 0 ...] . xb_i =
// |c - xs_i|^2 with an absolute rounding error of a few eps (|c|^2 + |xs_i|^2).
// One block; xb[rows * dp] = 1.0 when every |xs_i|^2 <= kDistNorm, else 0.0.
constexpr double kDistNorm = 2.0;
__global__ __launch_bounds__(256) void xb_kernel(const double* __restrict__ xs, int rows, int d, int dp,
                                                 double* __restrict__ xb) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < rows; i += 256) {
        double xx = 0.0;
        for (int c = 0; c < d; ++c) xx = fma(xs[(size_t)i * dp + c], xs[(size_t)i * dp + c], xx);
        for (int c = 0; c < dp; ++c)
            xb[(size_t)i * dp + c] = c < d ? -2.0 * xs[(size_t)i * dp + c] : c == d ? 1.0 : c == d + 1 ? xx : 0.0;
        if (!(xx <= kDistNorm)) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) xb[(size_t)rows * dp] = bad ? 0.0 : 1.0;
}

// Self-check of the expanded distance on the model's own observations (r2 = 0 at
// each one's own row and the smallest sd: its worst case): clears the xb flag
// unless both (mu_n, q) rows -- direct and expanded -- agree within 1e-10: q
// relative to sd^2 = amp - q, mu_n relative to its summand scale amp sum |alpha_i|
// (the conditioning of K*.alpha; the parity tests measure mu against the same kind
// of scale).
__global__ __launch_bounds__(256) void xb_check_kernel(const double* __restrict__ mqd, const double* __restrict__ mqm,
                                                       const double* __restrict__ alpha, int n, double amp,
                                                       double* __restrict__ flag) {
    __shared__ int bad;
    __shared__ double red[4];
    if (threadIdx.x == 0) bad = 0;
    double sa = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) sa += fabs(alpha[i]);
    for (int o = 32; o > 0; o >>= 1) sa += __shfl_down(sa, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sa;
    __syncthreads();
    const double mu_scale = amp * (red[0] + red[1] + red[2] + red[3]);
    for (int i = threadIdx.x; i < n; i += 256) {
        const double mud = mqd[2 * i], qd = mqd[2 * i + 1], mum = mqm[2 * i], qm = mqm[2 * i + 1];
        const bool ok = fabs(qm - qd) <= 1e-10 * fmax(amp - qd, 1e-300) && fabs(mum - mud) <= 1e-10 * mu_scale;
        if (!ok) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad) flag[0] = 0.0;
}

// K from unscaled X (mpo_gp_kernel_matrix has no workspace for xs): divides
// by ls inline, like sklearn's pdist(X / length_scale).
__global__ void kernel_matrix_unscaled_kernel(const double* __restrict__ X, int n, int d,
                                              const double* __restrict__ ls, double amp,
                                              double diag_add, double* __restrict__ K, int ldk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n) return;
    double r2 = 0.0;
    for (int c = 0; c < d; ++c) {
        const double t = X[(size_t)i * d + c] / ls[c] - X[(size_t)j * d + c] / ls[c];
        r2 += t * t;
    }
    double v = matern52(sqrt(r2), amp);
    if (i == j) v += diag_add;
    K[(size_t)i * ldk + j] = v;
}

// Right-looking unblocked Cholesky in one workgroup; A stays in global memory
// (L2-resident at the sizes skopt reaches).  Off the per-candidate hot path:
// run once per GP refit.
__global__ __launch_bounds__(1024) void chol_kernel(double* __restrict__ A, int n, int lda,
                                                    int32_t* __restrict__ info) {
    __shared__ int fail;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwave = nt >> 6;
    if (tid == 0) fail = 0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        if (tid == 0) {
            const double djj = A[(size_t)j * lda + j];
            if (!(djj > 0.0) || !isfinite(djj)) fail = j + 1;
            else A[(size_t)j * lda + j] = sqrt(djj);
        }
        __syncthreads();
        if (fail) break;
        const double ljj = A[(size_t)j * lda + j];
        for (int i = j + 1 + tid; i < n; i += nt) A[(size_t)i * lda + j] /= ljj;
        __syncthreads();
        for (int i = j + 1 + wave; i < n; i += nwave) {
            const double lij = A[(size_t)i * lda + j];
            for (int k = j + 1 + lane; k <= i; k += 64)
                A[(size_t)i * lda + k] -= lij * A[(size_t)k * lda + j];
        }
        __syncthreads();
    }
    if (tid == 0) *info = fail;
}

// One thread per right-hand-side column; the solution vector lives in LDS
// ([n][cb], conflict-free across the cb columns of a block).
__global__ __launch_bounds__(64) void trsm_kernel(const double* __restrict__ L, int n, int lda,
                                                  double* __restrict__ B, int nrhs, int ldb,
                                                  int trans, int cb) {
    extern __shared__ __attribute__((aligned(16))) double xsol[];
    const int lc = threadIdx.x;
    const int col = blockIdx.x * cb + lc;
    const bool active = lc < cb && col < nrhs;
    if (!active) return;
    if (!trans) {
        for (int i = 0; i < n; ++i) {
            double s = B[(size_t)i * ldb + col];
            const double* Li = L + (size_t)i * lda;
            for (int k = 0; k < i; ++k) s -= Li[k] * xsol[k * cb + lc];
            const double x = s / Li[i];
            xsol[i * cb + lc] = x;
            B[(size_t)i * ldb + col] = x;
        }
    } else {
        for (int i = n - 1; i >= 0; --i) {
            double s = B[(size_t)i * ldb + col];
            for (int k = i + 1; k < n; ++k) s -= L[(size_t)k * lda + i] * xsol[k * cb + lc];
            const double x = s / L[(size_t)i * lda + i];
            xsol[i * cb + lc] = x;
            B[(size_t)i * ldb + col] = x;
        }
    }
}

// B-fragment streams of W^T (W = L^-1 lower), one per scoring wave.
// Column tile jt (16 columns) needs the k-steps ks < 4(jt+1) (rows i <= 16 jt + 15):
// jt+1 groups of 4 k-steps; lane l of k-step ks holds
//   W^T[4 ks + (l>>4)][16 jt + (l&15)] = W[16 jt + (l&15)][4 ks + (l>>4)].
// The T tiles are dealt to the block's 4 waves by LPT on their group counts, and each
// wave's tiles are stored back to back, so a wave reads one contiguous stream across
// its tile boundaries (a software pipeline that never drains), followed by
// kStreamSlack groups of zeros for the prefetch that runs past its end.
// wmeta (int32): wave record w at w*(T+4): [group offset, groups, tiles, jt...];
//                tile_off[jt] at 4*(T+4) + jt (group offset of tile jt's first group).
constexpr int kStreamSlack = 2;   // = the ring depth of the scoring kernel's B pipeline
inline size_t wfrag_elems(int np16) {
    const size_t T = np16 / 16;
    return (T * (T + 1) / 2 + 4 * kStreamSlack) * 256;
}
inline size_t wmeta_elems(int np16) {
    const int T = np16 / 16;
    return (size_t)4 * (T + 4) + T + 4;
}

__global__ void wave_plan_kernel(int T, int32_t* __restrict__ meta) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int load[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
    for (int jt = T - 1; jt >= 0; --jt) {       // LPT: costliest tile to the least loaded wave
        int w = 0;
        for (int v = 1; v < 4; ++v)
            if (load[v] < load[w]) w = v;
        meta[w * (T + 4) + 3 + cnt[w]++] = jt;
        load[w] += jt + 1;
    }
    int off = 0;
    for (int w = 0; w < 4; ++w) {
        int32_t* r = meta + w * (T + 4);
        r[0] = off;
        r[1] = load[w];
        r[2] = cnt[w];
        for (int t = cnt[w]; t <= T; ++t) r[3 + t] = 0;
        int g = off;
        for (int t = 0; t < cnt[w]; ++t) {
            meta[4 * (T + 4) + r[3 + t]] = g;
            g += r[3 + t] + 1;
        }
        off += load[w] + kStreamSlack;
    }
}

__global__ void pack_wfrag_kernel(const double* __restrict__ W, int n, int ldw, int T,
                                  const int32_t* __restrict__ meta, double* __restrict__ wfrag) {
    const int jt = blockIdx.y;
    if (jt >= T) return;
    const int nks = 4 * (jt + 1);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nks * 64) return;
    const int ks = e >> 6, l = e & 63;
    const int i = 4 * ks + (l >> 4), j = 16 * jt + (l & 15);
    const double v = (i < n && j < n && i <= j) ? W[(size_t)j * ldw + i] : 0.0;
    wfrag[(size_t)meta[4 * (T + 4) + jt] * 256 + e] = v;
}

// ---------------------------------------------------------------------------
constexpr int kBM = 16;   // candidates per scoring workgroup (one 16-row MFMA m-tile)

struct ScoreArgs {
    int n, np16, T, d;
    double amp, y_mean, y_std;
    const double* xs;
    const double* xb;     // MD = 1: augmented observation rows (xb_kernel)
    const double* xb_ok;  // MD = 1: device flag, every |xs_i|^2 <= kDistNorm
    const double* ls;
    const double* alpha;
    const double* wfrag;
    const int32_t* wmeta;
    const double* cand;
    long long m;
    double y_opt, xi, kappa;
    unsigned flags;
    int ei_positive;  // write +EI (mpo_gp_ei_score) instead of -EI into vals
    int dbg;          // MPO_GP_DEBUG phase switches (timing experiments only; results invalid):
                      // bit 0 skips the MFMA phase, bit 1 the Matern arithmetic, bit 2 the top-k,
                      // bit 3 the finish's posterior / acquisition arithmetic
    double* mu;
    double* sd;
    double* vals;
    int k;
    long long* part_idx;  // [nparts][3][k]
    double* part_val;
    double* mq;           // [m][2] raw (mu_n, q) rows (FIN = 0 only: the prepare-time self-check)
    // streamed path only (gp_score_streamed_kernel)
    int panel;            // observation rows per K* panel (a multiple of 16)
    double* part;         // [grid][T - panel/16][256] partial rows of the later panels' column tiles
};

// One wave, 64 candidates (lane = candidate; invalid lanes contribute nothing): the
// posterior and acquisitions as score_finish_kernel computes them, the requested
// output rows, then the candidates merged into the workgroup's running top-k lists
// (tk_val / tk_idx [3][MPO_TOPK_MAX], sorted, LDS).  A lane takes part only while its
// (value, index) beats the list's k-th entry; each round inserts the group minimum
// among those lanes (lane 0 shifts the list), so at most k rounds run and usually none.
__device__ __attribute__((noinline)) void score_finish_group(const ScoreArgs& a, bool valid, long long gm, double mu_n,
                                                   double q, int lane, double* tk_val, long long* tk_idx) {
    double mu = 0.0, sd = 0.0, vei = 0.0, vpi = 0.0, vlcb = 0.0;
    if (valid && (a.dbg & 8)) {   // timing only: the posterior / acquisition arithmetic skipped
        mu = mu_n;
        sd = q;
    } else if (valid) {
        double var = a.amp - q;
        if (var < 0.0) var = 0.0;
        sd = sqrt(var) * a.y_std;
        mu = a.y_std * mu_n + a.y_mean;
        if (sd > 0.0) {
            const double improve = a.y_opt - a.xi - mu;
            const double scaled = improve / sd;
            const double cdf = ndtr(scaled);
            vei = -(improve * cdf + sd * norm_pdf(scaled));
            vpi = -cdf;
        } else {
            vei = -0.0;
            vpi = -0.0;
        }
        vlcb = mu - a.kappa * sd;
        if (a.mu) a.mu[gm] = mu;
        if (a.sd) a.sd[gm] = sd;
        if (a.vals) {
            if (a.flags & MPO_ACQ_EI) a.vals[gm] = a.ei_positive ? -vei : vei;
            if (a.flags & MPO_ACQ_PI) a.vals[a.m + gm] = vpi;
            if (a.flags & MPO_ACQ_LCB) a.vals[2 * a.m + gm] = vlcb;
        }
    }
    if (a.k <= 0 || (a.dbg & 4)) return;
    const double inf = __builtin_huge_val();
    const long long big = 0x7fffffffffffffffLL;
    const int k = a.k;
#pragma unroll
    for (int acq = 0; acq < 3; ++acq) {
        if (!(a.flags & (1u << acq))) continue;
        const double v = valid ? (acq == 0 ? vei : (acq == 1 ? vpi : vlcb)) : inf;
        const long long idx = valid ? gm : big;
        double* lv = tk_val + acq * MPO_TOPK_MAX;
        long long* li = tk_idx + acq * MPO_TOPK_MAX;
        bool cand = valid && lex_less(v, idx, lv[k - 1], li[k - 1]);
        while (__any(cand)) {
            double bv = cand ? v : inf;
            long long bi = cand ? idx : big;
            wave_lex_min(bv, bi);
            if (lane == 0) {
                int pos = k - 1;
                while (pos > 0 && lex_less(bv, bi, lv[pos - 1], li[pos - 1])) {
                    lv[pos] = lv[pos - 1];
                    li[pos] = li[pos - 1];
                    --pos;
                }
                lv[pos] = bv;
                li[pos] = bi;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // lane 0's list stores before every lane's reads
            cand = cand && idx != bi && lex_less(v, idx, lv[k - 1], li[k - 1]);
        }
    }
}

// The finish of a looped scoring kernel (tiles blockIdx.x, += gridDim.x): this
// workgroup's own (mu_n, q) rows (written in its tile loop, mostly still in this
// XCD's L2), 64 candidates per wave at a time with every lane live; one running
// top-k list per wave in the (now free) K* LDS region kc, written out as partial
// lists 4 blockIdx.x + wave.
// The finish reads its arguments through a pointer to the kernarg segment: the
// out-of-line score_finish_group given `a` itself would copy the by-value struct to
// the stack (and the scoring variants must stay scratch-free, see launch_looped);
// the asm keeps the loads out of the tile loop.  This holds only for a kernel whose
// only argument is one by-value ScoreArgs.
__device__ __forceinline__ void score_finish_own_rows(double* kc, int wave, int lane) {
    constexpr int BM = kBM;
    __syncthreads();   // the rows of the tile loop (global writes, workgroup-scope visibility)
    const ScoreArgs* ap = (const ScoreArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    const ScoreArgs& f = *ap;
    double* tk_val = kc + wave * 3 * MPO_TOPK_MAX;
    long long* tk_idx = reinterpret_cast<long long*>(kc + 4 * 3 * MPO_TOPK_MAX) + wave * 3 * MPO_TOPK_MAX;
    if (lane < 3 * MPO_TOPK_MAX) {
        tk_val[lane] = __builtin_huge_val();
        tk_idx[lane] = 0x7fffffffffffffffLL;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const long long ntl = ((f.m + BM - 1) / BM - blockIdx.x + gridDim.x - 1) / gridDim.x;   // this workgroup's tiles
    for (long long c0 = (long long)wave * 64; c0 < ntl * BM; c0 += 256) {
        const long long cl = c0 + lane;
        const long long gm = (blockIdx.x + (cl >> 4) * (long long)gridDim.x) * BM + (cl & 15);
        const bool valid = cl < ntl * BM && gm < f.m;
        double2 v = {0.0, 0.0};
        if (valid) v = *reinterpret_cast<const double2*>(f.mq + 2 * gm);
        score_finish_group(f, valid, gm, v.x, v.y, lane, tk_val, tk_idx);
    }
    if (f.k > 0 && lane < 3 * f.k) {
        const int acq = lane / f.k, r = lane - acq * f.k;
        const size_t part = (size_t)blockIdx.x * 4 + wave;
        f.part_val[(part * 3 + acq) * f.k + r] = tk_val[acq * MPO_TOPK_MAX + r];
        f.part_idx[(part * 3 + acq) * f.k + r] = tk_idx[acq * MPO_TOPK_MAX + r];
    }
}

// Pieces of both scoring kernels' bodies (macros: they read and update the
// kernels' locals c, row, kc, mu_acc, acc0, acc1).
// One group of B fragments (4 k-steps x 64 lanes of the wfrag stream) at lane
// pointer P into the ring slot B[0..3]: asm loads the compiler cannot see or wait
// for; every use of B is tied to an explicit s_waitcnt vmcnt (tests/test_isa_ring.py
// checks the generated code of both kernels).
#define MPO_LD(D, P, OFF) asm volatile("global_load_dwordx2 %0, %1, off offset:" #OFF : "=v"(D) : "v"(P) : "memory")
#define MPO_LD4(B, P) { MPO_LD(B[0], P, 0); MPO_LD(B[1], P, 512); MPO_LD(B[2], P, 1024); MPO_LD(B[3], P, 1536); }
// 4 MFMAs of one group on two accumulation chains: A fragments at lane pointer AP
// (k-steps 64 doubles apart), B fragments B0..B3
#define MPO_MFMA4(AP, B0, B1, B2, B3)                                                              \
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((AP)[0], B0, acc0, 0, 0, 0);                       \
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((AP)[64], B1, acc1, 0, 0, 0);                      \
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((AP)[128], B2, acc0, 0, 0, 0);                     \
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((AP)[192], B3, acc1, 0, 0, 0);
// one observation row on the direct distance: r2, Matern, mu partial, K* into the
// LDS at (panel-local) observation index LI
#define MPO_EI_PAIR(XC, AC, LI)                                                                    \
    {                                                                                              \
        double r2 = kR2Floor;                                                                      \
        _Pragma("unroll") for (int q = 0; q < D; ++q) {                                            \
            const double t = c[q] - XC[q];                                                         \
            r2 = fma(t, t, r2);                                                                    \
        }                                                                                          \
        const double kv = matern52_unit(r2);   /* amp folded into mu and q */                      \
        mu_acc = fma(kv, AC, mu_acc);                                                              \
        kc[(size_t)((LI) >> 2) * 64 + row + ((LI) & 3) * 16] = kv;                                 \
    }

// One workgroup = 4 waves looping over 16-candidate tiles (kBM) tile = blockIdx.x,
// += gridDim.x (the grid is sized to the resident capacity).  Two workgroup
// barriers per tile: B after phase 1 (K* complete) and D after phase 2.  The next
// tile's candidate rows are staged into cs between them (cs is read only before B),
// the rows of the tile after that load meanwhile, and the mu / q partials travel
// through red without a barrier of their own (mu in two halves by tile parity; the
// argument is at the two barriers).  A wave runs at raised priority (s_setprio 2)
// everywhere except phase 2's MFMA stream (priority 0): the CU's five workgroups are
// independent, and what a wave does outside phase 2 is short VALU work that its three
// siblings wait for at the next barrier.
// FIN = 1 (every scoring launch): after its tile loop the workgroup finishes its own
// candidates -- the (mu_n, q) rows it wrote (still largely in this XCD's L2) read
// back 64 per wave with every lane live, the posterior and acquisitions as
// score_finish_group computes them, one running top-k list per wave -- instead of a
// separate finish launch over rows written by workgroups on every XCD.  (An in-loop
// finish was built first: the loop already holds 101 SGPRs and 96 VGPRs at
// occupancy 5, and the finish's invariants spilled it.)  FIN = 0 stops at the rows
// (mpo_gp_prepare's self-check of the expanded form).
template <int DP, int D, int OCC, int MD, int FIN>
__global__ __launch_bounds__(256, OCC) void gp_score_kernel(ScoreArgs a) {
    static_assert(!MD || D + 2 <= DP, "the MFMA distance needs two spare columns");
    constexpr int BM = kBM;
    constexpr int S = 16;            // i-slots per block in phase 1 (4 per wave)
    constexpr int EPT = (BM * DP + 255) / 256;   // candidate elements per thread in phase 0
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int np16 = a.np16;
    double* kc = smem;                          // [np16/4][64]: k-step ks at kc[ks*64]
    double* cs = kc + (size_t)np16 * BM;        // [BM][DP]
    double* red = cs + BM * DP;                 // mu partials [2][4][BM] (tile parity, share), then
    double* redq = red + 2 * 4 * BM;            // q partials [4][BM] (wave); the last quarter of [S][BM] is unused
    int32_t* mls = reinterpret_cast<int32_t*>(red + S * BM);   // the 4 wave records of wmeta

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long ntiles = (a.m + BM - 1) / BM;

    for (int e = tid; e < 4 * (a.T + 4); e += 256) mls[e] = a.wmeta[e];

    const bool xb_ok = MD && *a.xb_ok != 0.0;   // read once: the model-level guard of the expanded distance
    // thread tid owns elements tid + 256 u of the [BM][DP] candidate tile
    double raw[EPT], ls_e[EPT];
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
        const int c = (tid + 256 * u) % DP;
        ls_e[u] = c < a.d ? a.ls[c] : 1.0;
    }
#define MPO_LOAD_TILE(TILE)                                                                    \
    _Pragma("unroll") for (int u = 0; u < EPT; ++u) {                                          \
        const int e = tid + 256 * u, r = e / DP, c = e % DP;                                   \
        const long long gm = (TILE) * BM + r;                                                  \
        raw[u] = (e < BM * DP && gm < a.m && c < a.d) ? __builtin_nontemporal_load(a.cand + gm * a.d + c) : 0.0; \
    }
    // candidate tile / ls -> LDS
#define MPO_STAGE_TILE                                                                         \
    _Pragma("unroll") for (int u = 0; u < EPT; ++u)                                            \
        if (tid + 256 * u < BM * DP) cs[tid + 256 * u] = raw[u] / ls_e[u];
    // prologue: the first tile staged, the second one loading
    MPO_LOAD_TILE((long long)blockIdx.x)
    MPO_STAGE_TILE
    MPO_LOAD_TILE((long long)blockIdx.x + gridDim.x)
    __syncthreads();
    // the finishing wave (mu fold, phase 3, FIN's group finish): the wave whose phase-2
    // B stream (sw = (wave + blockIdx.x) & 3, below) carries the fewest groups
    int fw = 0;
    {
        int lw = 0;
        for (int q = 1; q < 4; ++q)
            if (mls[q * (a.T + 4) + 1] < mls[lw * (a.T + 4) + 1]) lw = q;
        fw = __builtin_amdgcn_readfirstlane((lw - (int)blockIdx.x) & 3);
    }

    // Phase-2 B-fragment stream of this wave, rotated by block.  (The rotation was
    // meant to keep the heaviest stream off one SIMD.  The workgroups resident on one
    // CU are blockIdx.x apart by multiples of 256 and share blockIdx.x & 3, so it
    // does not do that; the hardware's varying wave placement does,
    // scripts/probes/wave_simd.hip.  It stays: the q fold's association follows it.)
    // B fragments arrive through asm loads
    // with explicit vmcnt waits: the compiler's own waitcnt placement drained the
    // ring every iteration (vmcnt(0) before register copies).  The ring lives
    // inside phase 2 only and is drained at its end: a compiler copy of a ring
    // register across a loop back-edge would read it before its load lands (a
    // ring kept in flight across candidate tiles failed parity exactly so).
    const int sw = (wave + (int)blockIdx.x) & 3;
    const int32_t* mw = mls + sw * (a.T + 4);        // LDS: no vmcnt wait at tile ends
    const int G = (a.dbg & 1) ? 0 : __builtin_amdgcn_readfirstlane(mw[1]);
    const double* bs = a.wfrag + (size_t)__builtin_amdgcn_readfirstlane(mw[0]) * 256 + lane;

    // Phase-1 share of this wave: the observations are dealt to four shares (MFMA
    // form: blocks of 16, t = share, += 4, so share 0 carries the extra block of
    // T % 4 == 1; direct form: i-slots 4 share + (lane >> 4), += 16).  The share moves
    // to the next wave every tile, so over four tiles every wave carries every share
    // once.  With the shares pinned to the wave index, the two-barrier loop lost 4% at
    // n = 600 (supposed cause: nothing re-aligns the waves between B and the next B
    // any more, so where the wave with the extra block is also fw, its phase 3 and
    // its longer phase 1 are on the critical path of every tile); with them moving
    // it gains at every n measured.  A share's mu partial goes to the share's row of
    // red whichever wave computed it: the fold below adds the rows in share order,
    // and the bits do not depend on the rotation.
    int vs = (wave + (int)blockIdx.x) & 3;
    double* redm = red;   // this tile's mu rows; the other parity's: red + 4 * BM

    // Static wave priority: raised everywhere but in phase 2's MFMA stream.  A CU holds
    // the waves of five independent workgroups, each SIMD one wave of each.  A wave in
    // phase 1, a fold or phase 3 runs a short VALU stretch that its three siblings on
    // the other SIMDs wait for at the next barrier; a wave in phase 2 issues 64-cycle
    // MFMAs back to back and loses little when the arbiter lets a sibling workgroup's
    // VALU instruction through first.  Measured: -3.6% at the flagship shape, bits
    // unchanged (DESIGN 3.1 "Wave priority by phase"; a third level for the folds and
    // phase 3 measured the same as two).
    __builtin_amdgcn_s_setprio(2);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = tile * BM;

    // ---- phase 1: K*[row][i] (Matern52) in A-fragment order, mu partials.  The
    // tile's rows were staged in cs before the last barrier (the prologue's, or the
    // previous tile's barrier D).  xs and alpha are zero from row n to
    // np16 + kXsPadRows (the note above scale_rows_kernel): no bounds check on i, and
    // the next observation row is loaded while the current one is evaluated.
    {
        const int row = lane & 15;
        const int slot = vs * 4 + (lane >> 4);
        double c[D];
#pragma unroll
        for (int q = 0; q < D; ++q) c[q] = cs[row * DP + q];
        double mu_acc = 0.0;
        bool md = false;   // this tile on the MFMA distance (every |c|^2 <= kDistNorm)
        if constexpr (MD) {
            double cc = 0.0;
#pragma unroll
            for (int q = 0; q < D; ++q) cc = fma(c[q], c[q], cc);
            md = xb_ok && __all(cc <= kDistNorm);
            if (md && !(a.dbg & 2)) {
                // K*[16 candidates][16 observations] per tile t of this wave: r2 as one
                // augmented dot product on f64 MFMA (A = [c, |c|^2, 1], B = xb), then the
                // Matern per C element.  f64 C/D map: col = lane & 15 (observation),
                // row = (lane >> 4) + 4 r (candidate).
                const int kr = lane >> 4;
                double af[DP / 4];
#pragma unroll
                for (int s = 0; s < DP / 4; ++s) {
                    const int kk = 4 * s + kr;
                    const double v = cs[row * DP + kk];
                    af[s] = kk == D ? cc : kk == D + 1 ? 1.0 : v;
                }
                const int T16 = np16 >> 4;
                double mu4[4] = {0.0, 0.0, 0.0, 0.0};
                // Block t's xb fragments and alpha arrive through asm loads issued one
                // block ahead, right behind block t - 4's MFMAs (bq is dead from there),
                // so their latency runs under that block's Matern instead of in front
                // of this block's MFMAs.  As for phase 2's ring, the compiler neither
                // sees nor waits for these loads: every use of bq / al is tied to the
                // explicit wait at the loop's top, alpha is copied out of its load
                // register by an asm move directly behind that wait (a plain copy was
                // sunk below the next load's issue), and the loop drains before the mu
                // fold, so a tile on the direct form never meets a load in flight.  The
                // last block's prefetch re-reads that block (a scalar select): nothing
                // past the wave's own blocks is touched, and a wave whose share is
                // empty (vs >= T16) neither loads nor waits.
                const int xoff = ((lane & 15) * DP + kr) * 8, aoff = (lane & 15) * 8;   // lane byte offsets
                double bq[DP / 4], al;
#define MPO_P1_LD(S)                                                                               \
                if constexpr (S < DP / 4)                                                          \
                    asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3"                        \
                                 : "=v"(bq[S]) : "v"(xoff), "s"(xp), "n"(32 * S) : "memory");
#define MPO_P1_LOAD(TT)                                                                            \
                {                                                                                  \
                    const double* xp = a.xb + (size_t)(TT) * 16 * DP;                              \
                    const double* alp = a.alpha + (size_t)(TT) * 16;                               \
                    MPO_P1_LD(0) MPO_P1_LD(1) MPO_P1_LD(2) MPO_P1_LD(3)                            \
                    MPO_P1_LD(4) MPO_P1_LD(5) MPO_P1_LD(6) MPO_P1_LD(7)                            \
                    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(al) : "v"(aoff), "s"(alp) : "memory"); \
                }
                static_assert(DP / 4 <= 8, "MPO_P1_LOAD issues at most 8 fragment loads");
                if (vs < T16) {
                    MPO_P1_LOAD(vs)
                    for (int t = vs; t < T16; t += 4) {
                        asm volatile("s_waitcnt vmcnt(0)" : "+v"(al));
#pragma unroll
                        for (int s = 0; s < DP / 4; ++s) asm volatile("" : "+v"(bq[s]));
                        double alc;
                        asm volatile("v_mov_b64 %0, %1" : "=v"(alc) : "v"(al));
                        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int s = 0; s < DP / 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[s], bq[s], acc, 0, 0, 0);
                        const int tn = t + 4 < T16 ? t + 4 : t;
                        MPO_P1_LOAD(tn)
                        const int i = t * 16 + (lane & 15);
                        double r2[4];
                        clamp_r2x4(acc, r2);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double kv = matern52_unit(r2[r]);
                            kc[(size_t)(i >> 2) * 64 + kr + 4 * r + (i & 3) * 16] = kv;
                            mu4[r] = fma(kv, alc, mu4[r]);
                        }
                    }
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(al));
#pragma unroll
                    for (int s = 0; s < DP / 4; ++s) asm volatile("" : "+v"(bq[s]));
                }
#undef MPO_P1_LOAD
#undef MPO_P1_LD
                colsum16x4(mu4);
                // the share's row of this tile's mu partials
                if ((lane & 15) == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) redm[vs * BM + kr + 4 * r] = mu4[r];
                }
            }
        }
        if (md && !(a.dbg & 2)) {
        } else if (a.dbg & 2) {
            for (int i = slot; i < np16; i += S) kc[(size_t)(i >> 2) * 64 + row + (i & 3) * 16] = c[0];
        } else {
            for (int i = slot; i < np16; i += S) {
                const double* xr = a.xs + (size_t)i * DP;
                MPO_EI_PAIR(xr, a.alpha[i], i)
            }
        }
        if (!md || (a.dbg & 2)) {
            // the share's 4 slots (lane >> 4) into one row
            mu_acc += __shfl_xor(mu_acc, 16);
            mu_acc += __shfl_xor(mu_acc, 32);
            if (lane < BM) redm[vs * BM + row] = mu_acc;
        }
    }
    // Barrier B: K* complete.  It also orders two reuses that need no barrier of
    // their own.  (1) Every read of cs (phase 1's c and af) is behind it, so the
    // next tile's rows go into cs right below; barrier D publishes them.  (2) The q
    // partials below overwrite redq, which wave fw read for the previous tile: fw
    // did so before it arrived here.  The mu rows written above need no guard at
    // all: they went to this tile's parity half of red, and what fw may still have
    // been reading when a run-ahead wave wrote them is the other half.
    __syncthreads();

    // ---- the next tile's rows (in raw since the previous tile) -> cs; the one
    // after starts loading and is not waited for before the next tile's barrier B
    MPO_STAGE_TILE
    MPO_LOAD_TILE(tile + 2 * (long long)gridDim.x)

    // ---- phase 2: V = K* L^-T on f64 MFMA, lower-triangular k-steps only.  The
    // wave walks its B-fragment stream (wave_plan_kernel) two 4-k-step groups ahead
    // (in the four-barrier loop, loading the ring's first groups before the barriers
    // instead measured the same).
    {
        __builtin_amdgcn_s_setprio(0);   // behind the staging: the MFMA stream yields to the other workgroups' VALU phases
        double b0[4], b1[4];
        MPO_LD4(b0, bs);
        MPO_LD4(b1, bs + 256);
        const double* bp = bs + 512;
        const double* kl = kc + lane;
        double sq[4] = {0.0, 0.0, 0.0, 0.0};
        f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        int t = 0, kg = 0, tlen = __builtin_amdgcn_readfirstlane(mw[3] + 1);
        // the next column tile's length, read one tile ahead: the LDS read at a
        // column tile's end is for the tile after the next, so nothing at the MFMA
        // drain waits for it.  (The record's jt list is zero-filled to T + 1 entries;
        // the read one past that, taken only by the wave that owns every tile of a
        // T = 1 model, stays inside mls and its value is never used.)
        int tnext = __builtin_amdgcn_readfirstlane(mw[4] + 1);
        // one group: 4 MFMAs on two accumulation chains, then the ring slot is
        // refilled with the group two ahead; at a column tile's last group
        // ||V_row||^2 takes the tile's columns
#define MPO_EI_GROUP(B)                                                                            \
        {                                                                                          \
            asm volatile("s_waitcnt vmcnt(4)" : "+v"(B[0]), "+v"(B[1]), "+v"(B[2]), "+v"(B[3])); \
            const double* ap = kl + kg * 256;                                                      \
            MPO_MFMA4(ap, B[0], B[1], B[2], B[3])                                                  \
            MPO_LD4(B, bp);                                                                        \
            bp += 256;                                                                             \
            if (++kg == tlen) {                                                                    \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                    \
                    const double v = acc0[r] + acc1[r];                                            \
                    sq[r] = fma(v, v, sq[r]);                                                      \
                }                                                                                  \
                acc0 = f64x4{0.0, 0.0, 0.0, 0.0};                                                  \
                acc1 = f64x4{0.0, 0.0, 0.0, 0.0};                                                  \
                kg = 0;                                                                            \
                tlen = tnext;                                                                      \
                tnext = __builtin_amdgcn_readfirstlane(mw[4 + (++t)] + 1);                         \
            }                                                                                      \
        }
        for (int g = 0; g < G; g += 2) {
            MPO_EI_GROUP(b0)
            if (g + 1 >= G) break;
            MPO_EI_GROUP(b1)
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b1[0]),
                     "+v"(b1[1]), "+v"(b1[2]), "+v"(b1[3]));
#undef MPO_EI_GROUP
        __builtin_amdgcn_s_setprio(2);   // the q fold, barrier D, phase 3 and the next phase 1
        // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 r.  Sum the columns:
        // all four folds first, then the stores
        colsum16x4(sq);
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) redq[wave * BM + (lane >> 4) + 4 * r] = sq[r];
        }
    }
    // Barrier D: every wave is done with K* (the next phase 1 rewrites kc), and the
    // mu and q partials and the next tile's cs are visible.  The waves other than fw
    // run ahead into the next tile's phase 1 while fw reads red below: they write
    // only the other parity's mu rows there, and stop at barrier B, which fw reaches
    // after its reads; redq is next written behind that barrier, and this parity's
    // mu rows two tiles on, behind the next barrier D.
    __syncthreads();

    // ---- phase 3: (mu_n, q) rows out (wave fw): the 4 shares' mu rows and the 4
    // waves' q rows, each folded in a fixed order
    if (wave == fw && lane < BM && m0 + lane < a.m) {
        double mu_n = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) mu_n += redm[s * BM + lane];
        mu_n *= a.amp;
        const double q = (redq[0 * BM + lane] + redq[1 * BM + lane] + redq[2 * BM + lane] + redq[3 * BM + lane]) *
                         (a.amp * a.amp);
        *reinterpret_cast<double2*>(a.mq + 2 * (m0 + lane)) = double2{mu_n, q};
    }
    vs = (vs + 1) & 3;
    redm = redm == red ? red + 4 * BM : red;
    }  // tile loop
    if constexpr (FIN) score_finish_own_rows(kc, wave, lane);
#undef MPO_STAGE_TILE
#undef MPO_LOAD_TILE
}

// ---------------------------------------------------------------------------
// Streamed scoring: the same posterior for models whose K* tile (16 candidates x
// np16 observations) does not fit the LDS.  The observation axis is cut into
// panels of a.panel rows (PT = panel / 16 column tiles); with k = [k_0; k_1; ...]
// and W = L^-1 block lower-triangular, v_I = sum_{J <= I} W[I,J] k_J.  Per
// candidate tile the workgroup walks the panels J in order:
//   phase 1 (VALU)  K*[16][panel J] (direct distance form) into the LDS, mu partials
//   phase 2 (MFMA)  for every column tile jt at or below panel J (dealt to the 4
//                   waves by jt mod 4, rotated by workgroup), the k-step groups of
//                   panel J only: groups t0..jt inside the panel (the triangular
//                   part), all of t0..t1-1 for the later panels (rectangular).  A
//                   tile inside panel J is complete: its ||V_row||^2 joins sq.  A
//                   later tile's partial row u = W[jt, 0..J] k goes to this
//                   workgroup's slice of the score workspace and seeds the
//                   accumulator when the next panel reaches the tile.
// The slice is written and read back by the same lane of the same wave (no
// barrier, no atomics); it holds (T - PT) x 2 KiB and stays in L2.  Registers
// cannot hold it in general (n = 2048 at the largest panel: 13 later tiles per wave =
// 104 VGPRs per lane, with static indexing only; a forced 16-row panel: 127 tiles).  W is read
// from the resident path's fragment stream: tile jt's groups lie back to back at
// tile_off[jt] (wmeta), so no second packing exists.  Worst-case growth of the
// score workspace: n = 2048, dp = 12, panel 1232 -> 51 tiles x 2 KiB x 256
// workgroups = 25.5 MiB (26 MiB at dp = 32, panel 1216; streamed_grid_cap keeps any
// forced panel under 48 MiB).
// The finish is the resident kernel's (score_finish_own_rows).
template <int DP, int D>
__global__ __launch_bounds__(256) void gp_score_streamed_kernel(ScoreArgs a) {
    constexpr int BM = kBM;
    constexpr int S = 16;            // i-slots per block in phase 1 (4 per wave)
    static_assert(4 * 3 * MPO_TOPK_MAX * 16 <= 16 * kBM * 8, "the finish's top-k lists live in the smallest panel");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int T = a.T, PT = a.panel >> 4;
    double* kc = smem;                          // [panel/4][64]: local k-step ks at kc[ks*64]
    double* cs = kc + (size_t)a.panel * BM;     // [BM][DP]
    double* red = cs + BM * DP;                 // [S][BM] (mu) + [4][BM] (q)
    int32_t* toff = reinterpret_cast<int32_t*>(red + (S + 4) * BM);   // [T] group offset of tile jt in wfrag

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long ntiles = (a.m + BM - 1) / BM;
    const int row = lane & 15;
    const int slot = wave * 4 + (lane >> 4);
    double* part = a.part + (size_t)blockIdx.x * (size_t)(T > PT ? T - PT : 0) * 256 + lane;

    for (int e = tid; e < T; e += 256) toff[e] = a.wmeta[4 * (T + 4) + e];

    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long m0 = tile * BM;
        // ---- phase 0: candidate tile / ls -> LDS
        for (int e = tid; e < BM * DP; e += 256) {
            const int r = e / DP, c = e % DP;
            const long long gm = m0 + r;
            cs[e] = (gm < a.m && c < a.d) ? __builtin_nontemporal_load(a.cand + gm * a.d + c) / a.ls[c] : 0.0;
        }
        __syncthreads();
        double c[D];
#pragma unroll
        for (int q = 0; q < D; ++q) c[q] = cs[row * DP + q];
        double mu_acc = 0.0;
        double sq[4] = {0.0, 0.0, 0.0, 0.0};

        for (int t0 = 0; t0 < T; t0 += PT) {
            const int t1 = min(T, t0 + PT);
            // ---- phase 1: K*[row][r0..r1) in A-fragment order (panel-local k-steps)
            for (int i = t0 * 16 + slot; i < t1 * 16; i += S) {
                const double* xr = a.xs + (size_t)i * DP;
                const int li = i - t0 * 16;
                MPO_EI_PAIR(xr, a.alpha[i], li)
            }
            __syncthreads();
            // ---- phase 2: this panel's k-steps of every column tile at or below it
            for (int jt = t0 + ((wave - t0 - (int)blockIdx.x) & 3); jt < T; jt += 4) {
                const int ng = min(jt, t1 - 1) - t0 + 1;   // groups of 4 k-steps
                f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
                double* pr = part + (size_t)(jt - PT) * 256;   // used only when jt >= PT
                if (t0 > 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc0[r] = pr[r * 64];
                }
                const double* bp = a.wfrag + ((size_t)__builtin_amdgcn_readfirstlane(toff[jt]) + t0) * 256 + lane;
                const double* ap = kc + lane;
                // B fragments through a three-group register ring filled by asm loads with
                // explicit vmcnt waits, as in gp_score_kernel (compiler-visible loads
                // were drained every iteration: the compiler rotated them to the loop
                // top and waited vmcnt(0) at its end).  Loads return in order, so
                // vmcnt(8) leaves only the two younger groups in flight.  The ring
                // lives inside one column tile and is drained at its end; loads past
                // the tile's last group re-read that group, so nothing outside the
                // tile's own fragments is touched.
#define MPO_ST_LD(B, G)                                                                        \
                {                                                                              \
                    const double* p = bp + (size_t)min((G), ng - 1) * 256;                     \
                    MPO_LD4(B, p)                                                              \
                }
#define MPO_ST_GROUP(B, G)                                                                     \
                {                                                                              \
                    asm volatile("s_waitcnt vmcnt(8)" : "+v"(B[0]), "+v"(B[1]), "+v"(B[2]), "+v"(B[3]));  \
                    const double* q = ap + (size_t)(G) * 256;                                  \
                    MPO_MFMA4(q, B[0], B[1], B[2], B[3])                                       \
                    MPO_ST_LD(B, (G) + 3)                                                      \
                }
                // The ring loop runs whole rotations only, without a branch in its body
                // (a body with exits made the compiler copy ring registers between
                // blocks while their loads were in flight); the ng % 3 groups left over
                // go first, through ordinary loads, under the ring's initial fill.
                const int rem = ng % 3;
                double b0[4], b1[4], b2[4];
                MPO_ST_LD(b0, rem)
                MPO_ST_LD(b1, rem + 1)
                MPO_ST_LD(b2, rem + 2)
                for (int g = 0; g < rem; ++g) {
                    const double* p = bp + (size_t)g * 256;
                    const double* q = ap + (size_t)g * 256;
                    MPO_MFMA4(q, p[0], p[64], p[128], p[192])
                }
                for (int g = rem; g < ng; g += 3) {
                    MPO_ST_GROUP(b0, g)
                    MPO_ST_GROUP(b1, g + 1)
                    MPO_ST_GROUP(b2, g + 2)
                }
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b1[0]),
                             "+v"(b1[1]), "+v"(b1[2]), "+v"(b1[3]), "+v"(b2[0]), "+v"(b2[1]), "+v"(b2[2]), "+v"(b2[3]));
#undef MPO_ST_GROUP
#undef MPO_ST_LD
                if (jt < t1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double v = acc0[r] + acc1[r];
                        sq[r] = fma(v, v, sq[r]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[r * 64] = acc0[r] + acc1[r];
                }
            }
            __syncthreads();   // the panel's K* is rewritten by the next phase 1
        }

        // ---- (mu_n, q) row: mu over the 16 slots, q over the 4 waves' column sums
        // (f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 r)
        red[slot * BM + row] = mu_acc;
        colsum16x4(sq);
        if ((lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(S + wave) * BM + (lane >> 4) + 4 * r] = sq[r];
        }
        __syncthreads();
        if (wave == 0 && lane < BM && m0 + lane < a.m) {
            double mu_n = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) mu_n += red[s * BM + lane];
            mu_n *= a.amp;
            const double q = (red[(S + 0) * BM + lane] + red[(S + 1) * BM + lane] + red[(S + 2) * BM + lane] +
                              red[(S + 3) * BM + lane]) * (a.amp * a.amp);
            *reinterpret_cast<double2*>(a.mq + 2 * (m0 + lane)) = double2{mu_n, q};
        }
        // red and cs are next written behind the next tile's barriers
    }

    score_finish_own_rows(kc, wave, lane);
}
#undef MPO_EI_PAIR
#undef MPO_MFMA4
#undef MPO_LD4
#undef MPO_LD

// Merge per-block top-k lists.  grid = (G, 3): block g of acquisition y merges
// the partial lists [g*chunk, min((g+1)*chunk, nparts)) and writes one list.
// Stage 1 writes the partial layout [(g*3 + acq)*k + r]; the final stage (G = 1)
// writes out[acq*out_stride + r] with index -1 for missing entries.
__global__ __launch_bounds__(256) void topk_merge_kernel(const long long* __restrict__ part_idx,
                                                         const double* __restrict__ part_val,
                                                         int nparts, int chunk, int k, unsigned flags,
                                                         long long* __restrict__ out_idx,
                                                         double* __restrict__ out_val,
                                                         int out_stride, int final_stage) {
    __shared__ double lv[256 * MPO_TOPK_MAX];
    __shared__ long long li[256 * MPO_TOPK_MAX];
    const int acq = blockIdx.y;
    if (!(flags & (1u << acq))) return;
    const int tid = threadIdx.x;
    const double inf = __builtin_huge_val();
    const long long big = 0x7fffffffffffffffLL;
    const int p0 = blockIdx.x * chunk;
    const int p1 = min(nparts, p0 + chunk);
    double bv[MPO_TOPK_MAX];
    long long bi[MPO_TOPK_MAX];
#pragma unroll
    for (int r = 0; r < MPO_TOPK_MAX; ++r) { bv[r] = inf; bi[r] = big; }
    const long long total = (long long)(p1 - p0) * k;
    for (long long e = tid; e < total; e += 256) {
        const long long blk = p0 + e / k, r = e % k;
        const size_t off = ((size_t)blk * 3 + acq) * k + r;
        double v = part_val[off];
        long long i = part_idx[off];
#pragma unroll
        for (int s = 0; s < MPO_TOPK_MAX; ++s) {
            if (s < k && lex_less(v, i, bv[s], bi[s])) {
                const double tv = bv[s];
                const long long ti = bi[s];
                bv[s] = v; bi[s] = i; v = tv; i = ti;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < MPO_TOPK_MAX; ++r) { lv[tid * MPO_TOPK_MAX + r] = bv[r]; li[tid * MPO_TOPK_MAX + r] = bi[r]; }
    __syncthreads();
    if (tid >= 64) return;
    // wave 0: k rounds of a 256-list merge; lane owns lists lane, lane+64, ...
    int ptr[4] = {0, 0, 0, 0};
    for (int r = 0; r < k; ++r) {
        double v = inf;
        long long i = big;
        int src = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lst = tid + 64 * q;
            if (ptr[q] < k) {
                const double w = lv[lst * MPO_TOPK_MAX + ptr[q]];
                const long long j = li[lst * MPO_TOPK_MAX + ptr[q]];
                if (lex_less(w, j, v, i)) { v = w; i = j; src = q; }
            }
        }
        double gv = v;
        long long gi = i;
        wave_lex_min(gv, gi);
        if (src >= 0 && gi == i && gv == v) {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (q == src) ptr[q]++;
        }
        if (tid == 0) {
            if (final_stage) {
                out_val[acq * out_stride + r] = gv;
                out_idx[acq * out_stride + r] = gi == big ? -1 : gi;
            } else {
                out_val[((size_t)blockIdx.x * 3 + acq) * k + r] = gv;
                out_idx[((size_t)blockIdx.x * 3 + acq) * k + r] = gi;
            }
        }
    }
}

__global__ void argmax_from_topk_kernel(const long long* __restrict__ topk_idx, long long* __restrict__ argmax) {
    *argmax = topk_idx[0];
}

// The (padded row width DP, distance dims D) instances of the scoring kernels, DP
// ascending: d = 5 and d = 10 (the reference's mnist space and the BASELINE config)
// get exact-width distance loops, listed ahead of their width's general instance.
// pad_dims, score_plan's test of a model's width and launch_scoring's dispatch all
// read this list.
#define MPO_SCORE_DIMS(X) X(4, 4) X(8, 5) X(8, 8) X(12, 10) X(12, 12) X(16, 16) X(32, 32)

// padded row width of d dims; -1 past the widest
inline int pad_dims(int d) {
#define MPO_X(DP, D) if (d <= DP) return DP;
    MPO_SCORE_DIMS(MPO_X)
#undef MPO_X
    return -1;
}

using mpo::kMaxLds;
constexpr int kMergeGroups = 256;  // stage-1 top-k merge groups
// Scoring grid bound: the resident capacity is <= 8 workgroups of 4 waves per CU
// (32 waves), 256 CUs on MI355X; workspace for top-k lists is sized from this.
constexpr int kScoreGridCap = 8 * 256;

size_t score_lds_bytes(int dp, int np16) {
    const int T = np16 / 16;
    // kc (after the tile loop: FIN's per-wave top-k lists, 4 x 3 x MPO_TOPK_MAX x 16 B <= np16 x kBM x 8 B),
    // cs, red | wave records
    return ((size_t)np16 * kBM + (size_t)kBM * dp + 16 * kBM) * sizeof(double) + (size_t)4 * (T + 4) * sizeof(int32_t);
}

bool score_fits(int dp, int np16) { return score_lds_bytes(dp, np16) <= kMaxLds; }

// ---- streamed path (gp_score_streamed_kernel): models past score_fits, n <= mpo::kMaxObs
constexpr size_t kStreamPartCap = (size_t)48 << 20;   // bytes of partial rows per scoring call

// one K* panel, cs, red (mu slots + q) | tile offsets
size_t streamed_lds_bytes(int dp, int np16, int panel) {
    return ((size_t)panel * kBM + (size_t)kBM * dp + 20 * kBM) * sizeof(double) + (size_t)(np16 / 16) * sizeof(int32_t);
}

// Streamed grid bound, from host arithmetic only (the workspace query runs without a
// device): the resident capacity at this LDS size on 256 CUs, lowered until the
// partial rows of all workgroups fit kStreamPartCap.
int streamed_grid_cap(int dp, int np16, int panel) {
    const int per_cu = (int)std::min<size_t>(8, kMaxLds / streamed_lds_bytes(dp, np16, panel));
    int cap = std::min(kScoreGridCap, std::max(1, per_cu) * 256);
    const size_t slice = (size_t)(np16 - panel) * kBM * sizeof(double);
    if (slice) cap = (int)std::min<size_t>(cap, std::max<size_t>(1, kStreamPartCap / slice));
    return cap;
}

// What serves one scoring call: built once per entry point by score_plan.
struct ScorePlan {
    int path;            // 0 resident (gp_score_kernel), 1 streamed (gp_score_streamed_kernel)
    int panel;           // streamed: observation rows per K* panel
    size_t lds;          // the kernel's dynamic LDS bytes
    int grid_cap;        // grid bound the workspace is sized from (the launch may stay below it)
    size_t part_elems;   // streamed: doubles of partial rows for the call's m candidates
};

// The plan for scoring m candidates against a model, or the refusal: MPO_ENOTSUP
// past mpo::kMaxObs, MPO_EINVAL for a malformed model or switch, with the message
// set under the entry point's name `who` (null: a silent query).  Host arithmetic
// only.  MPO_GP_SCORE=streamed forces the streamed kernel at any n ("resident" or
// unset: resident whenever it fits); MPO_GP_PANEL=<rows> (a multiple of 16, >= 16)
// sets the panel, clamped to the largest one that fits the LDS.
int score_plan(const char* who, const MpoGpModel* model, int64_t m, ScorePlan* plan) {
    const int n = model->n, dp = model->dp, np16 = model->np16;
    auto refuse = [&](int rc) {
        if (who)
            mpo::set_error(rc == MPO_ENOTSUP
                               ? "%s: n=%d exceeds the supported maximum of %d observations"
                               : "%s: malformed model (n=%d) or MPO_GP_PANEL (a multiple of 16, >= 16; max n %d)",
                           who, n, mpo::kMaxObs);
        return rc;
    };
    if (n <= 0 || np16 < n || np16 - n >= 16 || (np16 & 15) || dp <= 0 || pad_dims(dp) != dp)
        return refuse(MPO_EINVAL);   // pad_dims is the identity on the supported widths only
    if (n > mpo::kMaxObs) return refuse(MPO_ENOTSUP);
    const char* e = getenv("MPO_GP_SCORE");
    const bool forced = e && std::string(e) == "streamed";
    if (!forced && score_fits(dp, np16)) {
        *plan = ScorePlan{0, 0, score_lds_bytes(dp, np16), kScoreGridCap, 0};
        return MPO_OK;
    }
    int p = np16;
    while (p > 16 && streamed_lds_bytes(dp, np16, p) > kMaxLds) p -= 16;
    if (const char* pe = getenv("MPO_GP_PANEL"); pe && *pe) {
        char* end = nullptr;
        const long v = strtol(pe, &end, 10);
        if (*end || v < 16 || v % 16) return refuse(MPO_EINVAL);
        p = (int)std::min<long>(p, v);
    }
    const int cap = streamed_grid_cap(dp, np16, p);
    const int64_t grid = std::min<int64_t>((m + kBM - 1) / kBM, cap);
    *plan = ScorePlan{1, p, streamed_lds_bytes(dp, np16, p), cap, (size_t)grid * (size_t)(np16 - p) * kBM};
    return MPO_OK;
}

using ScoreKernel = void (*)(ScoreArgs);

// One launch of a looped scoring kernel (tiles blockIdx.x, += gridDim.x): grid =
// min(tiles, cap (the workspace is sized from it), the device's resident capacity
// at this LDS size); *grid_out receives it (one top-k list per wave of the grid).
// The B ring's asm loads are invisible to the compiler: a spill of a ring register
// would store it before its load lands.  A variant that spills is refused instead
// of run.
hipError_t launch_looped(ScoreKernel kern, const ScoreArgs& a, int ntiles, size_t lds, int cap, hipStream_t s,
                         int* grid_out) {
    const void* fn = reinterpret_cast<const void*>(kern);
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess || fa.localSizeBytes != 0) return hipErrorInvalidDeviceFunction;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int dev = 0, cus = 0, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds);
    const int grid = std::max(1, std::min(std::min(ntiles, cap), std::max(1, per_cu) * std::max(1, cus)));
    if (grid_out) *grid_out = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <int DP, int D, int OCC, int MD, int FIN>
bool spill_free() {
    static int ok = -1;
    if (ok < 0) {
        hipFuncAttributes fa;
        ok = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(gp_score_kernel<DP, D, OCC, MD, FIN>)) ==
                 hipSuccess &&
             fa.localSizeBytes == 0;
    }
    return ok == 1;
}

// occupancy hint (min waves per SIMD -> VGPR cap): the highest spill-free one;
// MPO_GP_OCC (2, 4, 5, 6) forces one for experiments
template <int DP, int D, int MD, int FIN>
ScoreKernel resident_kernel_occ() {
    const char* e = getenv("MPO_GP_OCC");
    int occ = e ? atoi(e) : 0;
    if (occ != 2 && occ != 4 && occ != 5 && occ != 6)
        occ = spill_free<DP, D, 6, MD, FIN>()   ? 6
              : spill_free<DP, D, 5, MD, FIN>() ? 5
              : spill_free<DP, D, 4, MD, FIN>() ? 4
                                                : 2;
    switch (occ) {
        case 6: return gp_score_kernel<DP, D, 6, MD, FIN>;
        case 5: return gp_score_kernel<DP, D, 5, MD, FIN>;
        case 4: return gp_score_kernel<DP, D, 4, MD, FIN>;
        default: return gp_score_kernel<DP, D, 2, MD, FIN>;
    }
}

// MD = 1 (the MFMA distance) when the model carries xb (d + 2 <= dp; the kernel
// reads the self-check's device flag); MPO_GP_DIST=0 forces the direct form.
// fin = false: raw (mu_n, q) rows only.
template <int DP, int D>
ScoreKernel resident_kernel(const ScoreArgs& a, bool fin) {
    if constexpr (D + 2 <= DP) {
        const char* e = getenv("MPO_GP_DIST");
        if (a.xb && a.xb_ok && !(e && e[0] == '0'))
            return fin ? resident_kernel_occ<DP, D, 1, 1>() : resident_kernel_occ<DP, D, 1, 0>();
    }
    return fin ? resident_kernel_occ<DP, D, 0, 1>() : resident_kernel_occ<DP, D, 0, 0>();
}

// The plan's kernel for a model of padded width dp and d dims, launched over ntiles
// candidate tiles (fin = false: the resident kernel only)
hipError_t launch_scoring(int dp, int d, const ScorePlan& p, const ScoreArgs& a, int ntiles, hipStream_t s, bool fin,
                          int* grid_out = nullptr) {
    ScoreKernel kern = nullptr;
#define MPO_X(DP, D)                                       \
    if (!kern && dp == DP && (d == D || D == DP))          \
        kern = p.path == 1 ? gp_score_streamed_kernel<DP, D> : resident_kernel<DP, D>(a, fin);
    MPO_SCORE_DIMS(MPO_X)
#undef MPO_X
    if (!kern) return hipErrorInvalidValue;
    return launch_looped(kern, a, ntiles, p.lds, p.grid_cap, s, grid_out);
}

int trsm_cols_per_block(int n) {
    size_t cb = 64;
    while (cb > 1 && (size_t)n * cb * sizeof(double) > kMaxLds - 1024) cb >>= 1;
    return (int)cb;
}

int trsm_launch(const double* L, int n, int lda, double* B, int nrhs, int ldb, int trans,
                hipStream_t s) {
    const int cb = trsm_cols_per_block(n);
    const size_t lds = (size_t)n * cb * sizeof(double);
    if (lds > kMaxLds) {
        mpo::set_error("mpo_trsm_f64: n=%d too large", n);
        return MPO_ENOTSUP;
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(trsm_kernel),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(trsm_kernel, dim3((nrhs + cb - 1) / cb), dim3(64), lds, s, L, n, lda, B,
                       nrhs, ldb, trans, cb);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

// ---------------------------------------------------------------------------
// Blocked factorisation for mpo_gp_prepare: K = L L^T and W = L^-1 over 32-wide
// blocks on the padded np x np matrix (np = n rounded up to 32, identity on the
// padding, so padded rows never couple to K).  The one-workgroup right-looking
// chol_kernel + one-thread-per-column trsm_kernel took ~27 ms at n = 500 (a cl_min
// batch pays one prepare per lie); here the sequential depth is one 32x32 block
// per step and everything else is MFMA work over many workgroups:
//   per block k:  bc_diag_kernel   (one wave) L_kk = chol(A_kk) in registers and
//                                  D_k = L_kk^-1 (row-wise forward substitution)
//                 bc_panel_kernel  L_ik = A_ik D_k^T for the 16-row tiles below
//                 bc_update_kernel A_IJ -= L_Ik L_Jk^T over the trailing lower tiles
//   per block row I of W:  bc_winv_kernel  W_II = D_I,
//                                          W_IJ = -D_I sum_{K=J}^{I-1} L_IK W_KJ
//   alpha = K^-1 y = W^T (W y)   (bc_wy_kernel, bc_wtv_kernel)
// All sums run in a fixed order: the results do not depend on the launch geometry.
constexpr int kBc = 32;
__host__ __device__ inline int bc_np(int n) { return (n + kBc - 1) / kBc * kBc; }

// A (padded, row-major [np][np]): the lower triangle and the full diagonal 32x32 blocks
__global__ void bc_kmat_kernel(const double* __restrict__ xs, int n, int dp, double amp, double diag_add,
                               double* __restrict__ A, int np) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= np || j > (i | (kBc - 1))) return;
    double v;
    if (i >= n || j >= n) {
        v = i == j ? 1.0 : 0.0;
    } else {
        double r2 = 0.0;
        for (int c = 0; c < dp; ++c) {
            const double t = xs[(size_t)i * dp + c] - xs[(size_t)j * dp + c];
            r2 += t * t;
        }
        v = matern52(sqrt(r2), amp);
        if (i == j) v += diag_add;
    }
    A[(size_t)i * np + j] = v;
}

// One wave: lane l (and l + 32, mirrored) holds row l of the diagonal block.  Column
// c of the factor is broadcast through the LDS at each step; a non-positive or
// non-finite pivot records info = first failing column + 1 (sklearn's LinAlgError).
__global__ __launch_bounds__(64) void bc_diag_kernel(double* __restrict__ A, int np, int k,
                                                     double* __restrict__ Dinv, double* __restrict__ Wp,
                                                     int32_t* __restrict__ info) {
    __shared__ double col[kBc];
    __shared__ double qrow[kBc];
    const int lane = threadIdx.x, l = lane & (kBc - 1);
    const int k0 = k * kBc;
    double* Akk = A + (size_t)k0 * np + k0;
    double r[kBc];
#pragma unroll
    for (int j = 0; j < kBc; ++j) r[j] = j <= l ? Akk[(size_t)l * np + j] : 0.0;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < kBc; ++c) {
        if (lane < kBc) col[l] = r[c];
        __syncthreads();
        const double d = col[c];
        if (!(d > 0.0) || !isfinite(d)) bad = bad ? bad : c + 1;
        const double lcc = sqrt(d);
        const double inv = 1.0 / lcc;
        if (l > c) r[c] *= inv;
        if (l == c) r[c] = lcc;
#pragma unroll
        for (int j = c + 1; j < kBc; ++j)
            if (j <= l) r[j] = fma(-r[c], col[j] * inv, r[j]);
        __syncthreads();
    }
    // D = L_kk^-1: row c = (e_c - sum_{m<c} L[c][m] D[m]) / L[c][c]; lane l keeps its
    // partial row p and finishes it at step c = l
    double p[kBc];
#pragma unroll
    for (int j = 0; j < kBc; ++j) p[j] = j == l ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < kBc; ++c) {
        if (lane == c) {
            const double inv = 1.0 / r[c];
#pragma unroll
            for (int j = 0; j <= c; ++j) {
                p[j] *= inv;
                qrow[j] = p[j];
            }
        }
        __syncthreads();
        if (l > c) {
#pragma unroll
            for (int j = 0; j <= c; ++j) p[j] = fma(-r[c], qrow[j], p[j]);
        }
        __syncthreads();
    }
    if (lane < kBc) {
#pragma unroll
        for (int j = 0; j < kBc; ++j) {
            if (j <= l) Akk[(size_t)l * np + j] = r[j];
            Dinv[(size_t)k * kBc * kBc + l * kBc + j] = j <= l ? p[j] : 0.0;
            if (Wp) Wp[(size_t)(k0 + l) * np + k0 + j] = j <= l ? p[j] : 0.0;
        }
    }
    if (lane == 0 && bad && info[0] == 0) info[0] = k0 + bad;
}

// L_ik = A_ik D_k^T for the 16-row tiles below block k, one tile per wave
// (two 16-column MFMA outputs, K = 32).  f64 16x16x4 operands: A[m = lane & 15][kk =
// lane >> 4], B[kk = lane >> 4][n = lane & 15]; C/D: col = lane & 15, row = (lane >> 4) + 4 q.
__global__ __launch_bounds__(256) void bc_panel_kernel(double* __restrict__ A, int np, int k,
                                                       const double* __restrict__ Dinv) {
    const int lane = threadIdx.x & 63;
    const int R = (k + 1) * 2 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (R >= np / 16) return;
    const int k0 = k * kBc;
    const double* D = Dinv + (size_t)k * kBc * kBc;
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    double a[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) a[ks] = A[(size_t)(16 * R + (lane & 15)) * np + k0 + 4 * ks + (lane >> 4)];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int kk = 4 * ks + (lane >> 4);
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], D[(lane & 15) * kBc + kk], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], D[(16 + (lane & 15)) * kBc + kk], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double* row = A + (size_t)(16 * R + (lane >> 4) + 4 * q) * np + k0;
        row[lane & 15] = acc0[q];
        row[16 + (lane & 15)] = acc1[q];
    }
}

// A_IJ -= L_Ik L_Jk^T over the lower 16x16 tiles of the trailing matrix (I >= J past
// block k), one tile per wave at a time, K = 32 (8 MFMAs)
__global__ __launch_bounds__(256) void bc_update_kernel(double* __restrict__ A, int np, int k) {
    const int lane = threadIdx.x & 63;
    const int t0 = (k + 1) * 2;                 // first trailing 16-tile
    const int T = np / 16 - t0;
    const int ntl = T * (T + 1) / 2;
    const int k0 = k * kBc;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nw = gridDim.x * 4;
    for (int t = gw; t < ntl; t += nw) {
        int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (I * (I + 1) / 2 > t) --I;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int J = t - I * (I + 1) / 2;
        const int gi = 16 * (t0 + I), gj = 16 * (t0 + J);
        f64x4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = A[(size_t)(gi + (lane >> 4) + 4 * q) * np + gj + (lane & 15)];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int kk = k0 + 4 * ks + (lane >> 4);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-A[(size_t)(gi + (lane & 15)) * np + kk],
                                                       A[(size_t)(gj + (lane & 15)) * np + kk], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) A[(size_t)(gi + (lane >> 4) + 4 * q) * np + gj + (lane & 15)] = acc[q];
    }
}

// Block row I of W = L^-1, block column J = blockIdx.x < I: wave w computes the
// 16x16 tile (a, b) = (w >> 1, w & 1) of S = sum_{K=J}^{I-1} L_IK W_KJ into the LDS,
// then W_IJ = -D_I S.
__global__ __launch_bounds__(256) void bc_winv_kernel(const double* __restrict__ L, double* __restrict__ Wp, int np,
                                                      int I, const double* __restrict__ Dinv) {
    __shared__ double S[kBc][kBc + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = w >> 1, b = w & 1;
    const int J = blockIdx.x;
    const int I0 = I * kBc, J0 = J * kBc;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int K = J; K < I; ++K) {
        const int K0 = K * kBc;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int kk = 4 * ks + (lane >> 4);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(L[(size_t)(I0 + 16 * a + (lane & 15)) * np + K0 + kk],
                                                       Wp[(size_t)(K0 + kk) * np + J0 + 16 * b + (lane & 15)], acc,
                                                       0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) S[16 * a + (lane >> 4) + 4 * q][16 * b + (lane & 15)] = acc[q];
    __syncthreads();
    const double* D = Dinv + (size_t)I * kBc * kBc;
    f64x4 o = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int kk = 4 * ks + (lane >> 4);
        o = __builtin_amdgcn_mfma_f64_16x16x4f64(D[(16 * a + (lane & 15)) * kBc + kk], S[kk][16 * b + (lane & 15)], o,
                                                 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) Wp[(size_t)(I0 + 16 * a + (lane >> 4) + 4 * q) * np + J0 + 16 * b + (lane & 15)] = -o[q];
}

// v = W y (one wave per row, fixed butterfly), then alpha = W^T v (one thread per column)
__global__ __launch_bounds__(256) void bc_wy_kernel(const double* __restrict__ Wp, int np, int n,
                                                    const double* __restrict__ y, double* __restrict__ v) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= np) return;
    double s = 0.0;
    for (int j = lane; j <= i && j < n; j += 64) s = fma(Wp[(size_t)i * np + j], y[j], s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) v[i] = s;
}

__global__ void bc_wtv_kernel(const double* __restrict__ Wp, int np, int n, const double* __restrict__ v,
                              double* __restrict__ alpha) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int i = j; i < np; ++i) s = fma(Wp[(size_t)i * np + j], v[i], s);
    alpha[j] = s;
}

// padded factors -> the model's [n][n] L and W (lower triangles, zeros above)
__global__ void bc_copy_out_kernel(const double* __restrict__ A, const double* __restrict__ Wp, int np, int n,
                                   double* __restrict__ L, double* __restrict__ W) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n) return;
    L[(size_t)i * n + j] = j <= i ? A[(size_t)i * np + j] : 0.0;
    W[(size_t)i * n + j] = j <= i ? Wp[(size_t)i * np + j] : 0.0;
}

// The block steps of A = L L^T in place on the padded np x np matrix (np a multiple of 32;
// info zeroed by the caller).  Wp: the padded L^-1 whose diagonal blocks receive D_k, or
// nullptr when only the factor is wanted (mpo::blocked_chol).
void factor_blocks(double* A, int np, double* Dinv, double* Wp, int32_t* info, hipStream_t s) {
    const int nbk = np / kBc;
    for (int k = 0; k < nbk; ++k) {
        hipLaunchKernelGGL(bc_diag_kernel, dim3(1), dim3(64), 0, s, A, np, k, Dinv, Wp, info);
        const int below = np / 16 - (k + 1) * 2;
        if (below <= 0) continue;
        hipLaunchKernelGGL(bc_panel_kernel, dim3((below + 3) / 4), dim3(256), 0, s, A, np, k, Dinv);
        const int ntl = below * (below + 1) / 2;
        hipLaunchKernelGGL(bc_update_kernel, dim3(std::max(1, std::min(1024, (ntl + 3) / 4))), dim3(256), 0, s,
                           A, np, k);
    }
}

// The launch sequence of the blocked factorisation (+ alpha) on stream s.
hipError_t blocked_factor(const double* xs, int n, int dp, double amp, double diag_add, const double* y_norm,
                          double* A, double* Wp, double* Dinv, double* v, double* L, double* W, double* alpha,
                          int32_t* info, hipStream_t s) {
    const int np = bc_np(n), nbk = np / kBc;
    (void)hipMemsetAsync(info, 0, sizeof(int32_t), s);
    (void)hipMemsetAsync(Wp, 0, (size_t)np * np * sizeof(double), s);
    hipLaunchKernelGGL(bc_kmat_kernel, dim3((np + 63) / 64, np), dim3(64), 0, s, xs, n, dp, amp, diag_add, A, np);
    factor_blocks(A, np, Dinv, Wp, info, s);
    for (int I = 1; I < nbk; ++I)
        hipLaunchKernelGGL(bc_winv_kernel, dim3(I), dim3(256), 0, s, A, Wp, np, I, Dinv);
    hipLaunchKernelGGL(bc_wy_kernel, dim3((np + 3) / 4), dim3(256), 0, s, Wp, np, n, y_norm, v);
    hipLaunchKernelGGL(bc_wtv_kernel, dim3((n + 255) / 256), dim3(256), 0, s, Wp, np, n, v, alpha);
    hipLaunchKernelGGL(bc_copy_out_kernel, dim3((n + 63) / 64, n), dim3(64), 0, s, A, Wp, np, n, L, W);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Rank-one append for mpo_gp_append: the factor of n + 1 observations from the factor
// of n at the same hyper-parameters.  With k* = K(X, x_new), l = W k* (W = L^-1) and
// delta^2 = K(x_new, x_new) - |l|^2:
//   L' = [L 0; l^T delta]     W' = [W 0; -(1/delta) l^T W   1/delta]
// l and l^T W are bc_wy_kernel / bc_wtv_kernel on the old W (leading dimension n), so
// every sum runs in the fixed order of the blocked factorisation; what is new here is
// k*, delta and the copy of both triangles to the leading dimension n + 1.

// k*_i = amp Matern52(|xs_i - xs_n|), i < n: row n of bc_kmat_kernel's matrix
__global__ void ap_kstar_kernel(const double* __restrict__ xs, int n, int dp, double amp, double* __restrict__ ks) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double r2 = 0.0;
    for (int c = 0; c < dp; ++c) {
        const double t = xs[(size_t)n * dp + c] - xs[(size_t)j * dp + c];
        r2 += t * t;
    }
    ks[j] = matern52(sqrt(r2), amp);
}

// One workgroup: dl = (delta, 1 / delta) from delta^2 = kdiag - sum l_i^2 (thread t sums
// i = t, t + 256, ... in order, a fixed butterfly per wave, the four waves in order), and
// the new model's info: the base's when that failed, else n + 1 (the column mpo_chol_f64
// reports) for a non-positive or non-finite pivot.
__global__ __launch_bounds__(256) void ap_delta_kernel(const double* __restrict__ l, int n, double kdiag,
                                                       const int32_t* __restrict__ base_info,
                                                       double* __restrict__ dl, int32_t* __restrict__ info) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s = fma(l[i], l[i], s);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double d2 = kdiag - (((red[0] + red[1]) + red[2]) + red[3]);
        const bool bad = !(d2 > 0.0) || !isfinite(d2);
        const double dlt = sqrt(d2);
        dl[0] = dlt;
        dl[1] = 1.0 / dlt;
        const int32_t bi = base_info[0];
        info[0] = bi ? bi : bad ? n + 1 : 0;
    }
}

// Both triangles at the new leading dimension n + 1 (zeros above the diagonal): rows
// i < n from the base, row n = (l^T, delta) of L and (-(1/delta) t^T, 1/delta) of W,
// t = W^T l.
__global__ void ap_copy_kernel(const double* __restrict__ L0, const double* __restrict__ W0, int n,
                               const double* __restrict__ l, const double* __restrict__ t,
                               const double* __restrict__ dl, double* __restrict__ L, double* __restrict__ W) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    const int n1 = n + 1;
    if (j >= n1) return;
    double lv, wv;
    if (i < n) {
        lv = j <= i ? L0[(size_t)i * n + j] : 0.0;
        wv = j <= i ? W0[(size_t)i * n + j] : 0.0;
    } else {
        lv = j < n ? l[j] : dl[0];
        wv = j < n ? -dl[1] * t[j] : dl[1];
    }
    L[(size_t)i * n1 + j] = lv;
    W[(size_t)i * n1 + j] = wv;
}

// The launch sequence of the append (+ alpha) on stream s; sc: 3 (n + 1) + 2 doubles of scratch.
hipError_t append_factor(const double* xs, int n, int dp, double amp, double diag_add, const double* y_norm,
                         const double* L0, const double* W0, const int32_t* info0, double* sc, double* v, double* L,
                         double* W, double* alpha, int32_t* info, hipStream_t s) {
    const int n1 = n + 1;
    double *ks = sc, *l = sc + n1, *t = sc + 2 * (size_t)n1, *dl = sc + 3 * (size_t)n1;
    hipLaunchKernelGGL(ap_kstar_kernel, dim3((n + 255) / 256), dim3(256), 0, s, xs, n, dp, amp, ks);
    hipLaunchKernelGGL(bc_wy_kernel, dim3((n + 3) / 4), dim3(256), 0, s, W0, n, n, ks, l);
    hipLaunchKernelGGL(ap_delta_kernel, dim3(1), dim3(256), 0, s, l, n, amp + diag_add, info0, dl, info);
    hipLaunchKernelGGL(bc_wtv_kernel, dim3((n + 255) / 256), dim3(256), 0, s, W0, n, n, l, t);
    hipLaunchKernelGGL(ap_copy_kernel, dim3((n1 + 63) / 64, n1), dim3(64), 0, s, L0, W0, n, l, t, dl, L, W);
    hipLaunchKernelGGL(bc_wy_kernel, dim3((n1 + 3) / 4), dim3(256), 0, s, W, n1, n1, y_norm, v);
    hipLaunchKernelGGL(bc_wtv_kernel, dim3((n1 + 255) / 256), dim3(256), 0, s, W, n1, n1, v, alpha);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Acquisition value + gradient at a few points, the polish objective: one workgroup of NW
// waves per point b, f[b] and g[b][d] of acquisition acq[b] from mpo::posterior_grad and
// mpo::acq_value_grad (gp_grad.h, shared with gp_ps.hip's cost-aware kernel).
template <int NW>
__global__ __launch_bounds__(NW * 64) void acq_grad_kernel(
        int n, int d, mpo::GradModel gm, const double* __restrict__ x, const int32_t* __restrict__ acq, double y_opt,
        double xi, double kappa, double* __restrict__ f, double* __restrict__ g) {
    extern __shared__ double sm[];
    __shared__ double xp[32];
    constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;
    __shared__ double red[kGradThreads];
    __shared__ double ga[kGroups][32], gu[kGroups][32];
    const int b = blockIdx.x, tid = threadIdx.x;
    double mu = 0.0, sd = 0.0, mu_g = 0.0, sd_g = 0.0;
    mpo::posterior_grad<NW>(gm, n, d, x + (size_t)b * d, sm, xp, red, ga, gu, mu, sd, mu_g, sd_g);
    if (tid < d) {
        double fv, gv;
        mpo::acq_value_grad(acq[b], mu, sd, mu_g, sd_g, y_opt, xi, kappa, fv, gv);
        g[(size_t)b * d + tid] = gv;
        if (tid == 0) f[b] = fv;
    }
}

// Scoring workspace: per-wave partial top-k lists, the stage-1 merge lists, a
// 3-entry tail (mpo_gp_ei_score's top-1) and the (mu_n, q) rows.
struct ScoreWs {
    long long* part_idx;
    double* part_val;
    long long* mid_idx;
    double* mid_val;
    long long* tail_idx;
    double* tail_val;
    double* mq;
    double* part;   // streamed path: the workgroups' partial-row slices (part_elems doubles)
    size_t used;    // bytes carved
};

// top-k lists: 4 per workgroup (one per wave); a workgroup has at least one tile
// and the grid never exceeds kScoreGridCap (tiles are looped over)
inline int64_t score_nparts(int64_t m) { return 4 * std::min<int64_t>((m + kBM - 1) / kBM, kScoreGridCap); }

// ws = null: the size query (pointers null, used valid)
inline ScoreWs carve_score_ws(void* ws, int64_t m, int k, size_t part_elems = 0) {
    const int64_t nparts = score_nparts(m);
    const int kk = std::max(k, 1);
    mpo::WsCarver c(ws);
    ScoreWs w;
    w.part_idx = c.take<long long>((size_t)nparts * 3 * kk);
    w.part_val = c.take<double>((size_t)nparts * 3 * kk);
    w.mid_idx = c.take<long long>((size_t)kMergeGroups * 3 * kk);
    w.mid_val = c.take<double>((size_t)kMergeGroups * 3 * kk);
    w.tail_idx = c.take<long long>(3 * kk);
    w.tail_val = c.take<double>(3 * kk);
    w.mq = c.take<double>((size_t)m * 2);
    w.part = c.take<double>(part_elems);
    w.used = c.used;
    return w;
}

// The prepare workspace: the model's arrays (MpoGpModel points into them, and
// export_factor / from_factor ship these bytes between ranks: the order and sizes
// are a format), the self-check's rows and the blocked factorisation's scratch.
struct PrepareWs {
    double* xs;        // [np16 + kXsPadRows][dp] (zero padding rows)
    double* ls_pad;    // [dp]
    double* L;         // [n][n]
    double* W;         // [n][n]
    double* alpha;     // [np16 + kXsPadRows] (zero padding)
    double* wfrag;
    int32_t* info;
    int32_t* wmeta;
    double* xb;        // [np16 + kXsPadRows][dp] + its guard flag (xb_flag)
    double* mqc;       // [2][n][2] xb self-check (mu_n, q) rows, direct and expanded
    double* Ab;        // blocked factorisation: padded A -> L
    double* Wb;        //                        padded W
    double* Db;        //                        diagonal-block inverses
    double* vb;        //                        W y
    size_t used;       // bytes carved
};

// ws = null: the size query (pointers null, used valid)
inline PrepareWs carve_prepare_ws(void* ws, int n, int dp) {
    const int np16 = (n + 15) / 16 * 16;
    const size_t xrows = np16 + kXsPadRows, np = bc_np(n);
    mpo::WsCarver c(ws);
    PrepareWs w;
    w.xs = c.take<double>(xrows * dp);
    w.ls_pad = c.take<double>(dp);
    w.L = c.take<double>((size_t)n * n);
    w.W = c.take<double>((size_t)n * n);
    w.alpha = c.take<double>(xrows);
    w.wfrag = c.take<double>(wfrag_elems(np16));
    w.info = c.take<int32_t>(4);
    w.wmeta = c.take<int32_t>(wmeta_elems(np16));
    w.xb = c.take<double>(xrows * dp + 8);
    w.mqc = c.take<double>(4 * (size_t)n);
    w.Ab = c.take<double>(np * np);
    w.Wb = c.take<double>(np * np);
    w.Db = c.take<double>(np * kBc);
    w.vb = c.take<double>(np);
    w.used = c.used;
    return w;
}

// the expanded distance's device flag, behind the rows of xb (xb_kernel writes it)
template <class T>
inline T* xb_flag(T* xb, int np16, int dp) { return xb + (size_t)(np16 + kXsPadRows) * dp; }

// The model's part of a scoring call's arguments; the call's own part is zero.
inline ScoreArgs model_score_args(const MpoGpModel& md) {
    ScoreArgs a{};
    a.n = md.n;
    a.np16 = md.np16;
    a.T = md.np16 / 16;
    a.d = md.d;
    a.amp = md.amp;
    a.y_mean = md.y_mean;
    a.y_std = md.y_std;
    a.xs = md.xs;
    a.xb = md.xb;
    a.xb_ok = md.xb ? xb_flag(md.xb, md.np16, md.dp) : nullptr;
    a.ls = md.ls;
    a.alpha = md.alpha;
    a.wfrag = md.wfrag;
    a.wmeta = md.wmeta;
    return a;
}

// The model's pointers into its carved workspace (xb: finish_prepared, once the self-check ran)
inline void point_model(MpoGpModel& md, const PrepareWs& w) {
    md.xs = w.xs;
    md.ls = w.ls_pad;
    md.alpha = w.alpha;
    md.wfrag = w.wfrag;
    md.L = w.L;
    md.W = w.W;
    md.info = w.info;
    md.wmeta = w.wmeta;
    md.xb = nullptr;
}

// The tail of a prepared model, shared by mpo_gp_prepare and mpo_gp_append: L^-1 packed for
// the scoring kernel and, on the resident path with d + 2 <= dp, xb and its self-check.
// md: everything but xb set; X: the model's n observations (the self-check's candidates).
int finish_prepared(MpoGpModel& md, const PrepareWs& w, const ScorePlan& plan, const double* X, hipStream_t s) {
    const int n = md.n, d = md.d, dp = md.dp, np16 = md.np16;
    const int xrows = np16 + kXsPadRows;
    const double amp = md.amp;
    const int T = np16 / 16;
    const size_t nw = wfrag_elems(np16);
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w.wfrag, (int)nw);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(wave_plan_kernel, dim3(1), dim3(64), 0, s, T, w.wmeta);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_wfrag_kernel, dim3((4 * T * 64 + 255) / 256, T), dim3(256), 0, s, w.W, n, n, T, w.wmeta,
                       w.wfrag);
    MPO_LAUNCH_CHECK();
    // The expanded (MFMA) distance |c|^2 + |x|^2 - 2 c.x (d + 2 <= dp) carries an absolute
    // error of a few eps (|c|^2 + |x|^2) instead of the direct form's eps r2.  Its device
    // flag is set only when every |x|^2 <= kDistNorm and, scoring the observations
    // themselves both ways, (mu_n, q) agree within 1e-10; candidate tiles with some
    // |c|^2 > kDistNorm take the direct form in the kernel.  MPO_GP_DIST=0: never.
    const char* de = getenv("MPO_GP_DIST");
    // A streamed model (score_plan) always scores with the direct form: no xb, no self-check.
    if (plan.path == 0 && d + 2 <= dp && !(de && de[0] == '0')) {
        double* flag = xb_flag(w.xb, np16, dp);
        hipLaunchKernelGGL(xb_kernel, dim3(1), dim3(256), 0, s, w.xs, xrows, d, dp, w.xb);
        MPO_LAUNCH_CHECK();
        ScoreArgs sa = model_score_args(md);           // md.xb still null: the direct form
        sa.cand = X;
        sa.m = n;
        sa.flags = 1;
        const int nt = (n + kBM - 1) / kBM;
        double* mqm = w.mqc + 2 * (size_t)n;
        sa.mq = w.mqc;
        bool ok = launch_scoring(dp, d, plan, sa, nt, s, /*fin=*/false) == hipSuccess;
        sa.mq = mqm;                                   // expanded form
        sa.xb = w.xb;
        sa.xb_ok = flag;
        // a refused variant (MPO_GP_OCC forcing a spilling one) just leaves xb out
        ok = ok && launch_scoring(dp, d, plan, sa, nt, s, /*fin=*/false) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(xb_check_kernel, dim3(1), dim3(256), 0, s, w.mqc, mqm, w.alpha, n, amp, flag);
            MPO_LAUNCH_CHECK();
            md.xb = w.xb;
        }
    }
    return MPO_OK;
}

}  // namespace

// The blocked Cholesky of mpo_gp_prepare on a caller's padded matrix (gp_joint.hip factors
// the sample covariance with it): the same kernels and step order, no L^-1.
hipError_t mpo::blocked_chol(double* A, int np, double* Dinv, int32_t* info, hipStream_t s) {
    (void)hipMemsetAsync(info, 0, sizeof(int32_t), s);
    factor_blocks(A, np, Dinv, nullptr, info, s);
    return hipGetLastError();
}

// The two-stage merge of per-wave top-k lists (layout [part][3][k]) into out[acq * k + r]:
// stage 1 merges G groups of ~64 lists each into `mid` (kTopkMergeGroups x 3 x k entries),
// stage 2 those into one list, index -1 for missing entries.  gp_ps.hip merges with it too.
hipError_t mpo::topk_merge(const long long* part_idx, const double* part_val, int nparts, int k, unsigned flags,
                           long long* mid_idx, double* mid_val, long long* out_idx, double* out_val,
                           hipStream_t s) {
    static_assert(kMergeGroups == mpo::kTopkMergeGroups, "the mid lists' size is shared through mpo_internal.h");
    const int chunk = std::max(64, (nparts + kMergeGroups - 1) / kMergeGroups);
    const int G = (nparts + chunk - 1) / chunk;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(G, 3), dim3(256), 0, s, part_idx, part_val, nparts, chunk, k, flags,
                       mid_idx, mid_val, k, 0);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(1, 3), dim3(256), 0, s, mid_idx, mid_val, G, G, k, flags, out_idx,
                       out_val, k, 1);
    return hipGetLastError();
}

// ===========================================================================
extern "C" {

int mpo_gp_kernel_matrix(const double* X, int n, int d, const double* ls, double amp,
                         double diag_add, double* K, int ldk, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(X && ls && K, "mpo_gp_kernel_matrix: null pointer");
    MPO_CHECK_ARG(n > 0 && d > 0 && ldk >= n, "mpo_gp_kernel_matrix: bad shape n=%d d=%d ldk=%d", n, d, ldk);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kernel_matrix_unscaled_kernel, dim3((n + 63) / 64, n), dim3(64), 0, s, X, n, d, ls, amp, diag_add, K, ldk);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_chol_f64(double* A, int n, int lda, int32_t* info, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(A && info, "mpo_chol_f64: null pointer");
    MPO_CHECK_ARG(n > 0 && lda >= n, "mpo_chol_f64: bad shape n=%d lda=%d", n, lda);
    hipLaunchKernelGGL(chol_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), A, n, lda, info);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_trsm_f64(const double* L, int n, int lda, double* B, int nrhs, int ldb, int trans, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(L && B, "mpo_trsm_f64: null pointer");
    MPO_CHECK_ARG(n > 0 && nrhs > 0 && lda >= n && ldb >= nrhs, "mpo_trsm_f64: bad shape");
    MPO_CHECK_ARG(trans == 0 || trans == 1, "mpo_trsm_f64: trans must be 0 or 1");
    return trsm_launch(L, n, lda, B, nrhs, ldb, trans, static_cast<hipStream_t>(stream));
    MPO_GUARD_END
}

size_t mpo_gp_prepare_ws_bytes(int n, int d) {
    const int dp = pad_dims(d);
    if (n <= 0 || n > mpo::kMaxObs || dp < 0) return 0;
    return carve_prepare_ws(nullptr, n, dp).used + 256;
}

int mpo_gp_prepare(const double* X, const double* y_norm, int n, int d, const double* ls,
                   double amp, double noise, double y_mean, double y_std,
                   MpoGpModel* model, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(X && y_norm && ls && model && ws, "mpo_gp_prepare: null pointer");
    const int dp = pad_dims(d);
    MPO_CHECK_ARG(n > 0 && d > 0, "mpo_gp_prepare: bad shape n=%d d=%d", n, d);
    if (dp < 0) { mpo::set_error("mpo_gp_prepare: d=%d > 32 unsupported", d); return MPO_ENOTSUP; }
    MPO_CHECK_ARG(ws_bytes >= mpo_gp_prepare_ws_bytes(n, d), "mpo_gp_prepare: workspace too small (%zu < %zu)",
                  ws_bytes, mpo_gp_prepare_ws_bytes(n, d));
    const int np16 = (n + 15) / 16 * 16;
    const int xrows = np16 + kXsPadRows;
    MpoGpModel md{};
    md.n = n;
    md.d = d;
    md.dp = dp;
    md.np16 = np16;
    md.amp = amp;
    md.y_mean = y_mean;
    md.y_std = y_std;
    ScorePlan plan;
    if (const int rc = score_plan("mpo_gp_prepare", &md, n, &plan)) return rc;
    const PrepareWs w = carve_prepare_ws(ws, n, dp);
    point_model(md, w);
    hipStream_t s = static_cast<hipStream_t>(stream);

    hipLaunchKernelGGL(scale_rows_kernel, dim3((xrows * dp + 255) / 256), dim3(256), 0, s, X, n, xrows, d, dp, ls, w.xs,
                       w.ls_pad);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(zero_kernel, dim3((xrows + 255) / 256), dim3(256), 0, s, w.alpha, xrows);
    MPO_LAUNCH_CHECK();
    MPO_HIP(blocked_factor(w.xs, n, dp, amp, noise + kJitter, y_norm, w.Ab, w.Wb, w.Db, w.vb, w.L, w.W, w.alpha, w.info,
                           s));
    if (const int rc = finish_prepared(md, w, plan, X, s)) return rc;
    *model = md;
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_append(const MpoGpModel* base, const double* X, const double* y_norm, const double* ls, double noise,
                  double y_mean, double y_std, MpoGpModel* model, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(base && X && y_norm && ls && model && ws, "mpo_gp_append: null pointer");
    const int n = base->n, d = base->d, dp = base->dp, n1 = n + 1;
    MPO_CHECK_ARG(n > 0 && d > 0 && dp > 0 && pad_dims(d) == dp, "mpo_gp_append: malformed base model n=%d d=%d dp=%d",
                  n, d, dp);
    if (n1 > mpo::kMaxObs) {
        mpo::set_error("mpo_gp_append: n=%d exceeds the supported maximum of %d observations", n1, mpo::kMaxObs);
        return MPO_ENOTSUP;
    }
    MPO_CHECK_ARG(ws_bytes >= mpo_gp_prepare_ws_bytes(n1, d), "mpo_gp_append: workspace too small (%zu < %zu)",
                  ws_bytes, mpo_gp_prepare_ws_bytes(n1, d));
    MPO_CHECK_ARG(base->L && base->W && base->info, "mpo_gp_append: base model not prepared");
    const int np16 = (n1 + 15) / 16 * 16;
    const int xrows = np16 + kXsPadRows;
    MpoGpModel md{};
    md.n = n1;
    md.d = d;
    md.dp = dp;
    md.np16 = np16;
    md.amp = base->amp;
    md.y_mean = y_mean;
    md.y_std = y_std;
    ScorePlan plan;
    if (const int rc = score_plan("mpo_gp_append", &md, n1, &plan)) return rc;
    const PrepareWs w = carve_prepare_ws(ws, n1, dp);
    MPO_CHECK_ARG(w.xs != base->xs, "mpo_gp_append: ws is the base model's workspace (the append is not in place)");
    point_model(md, w);
    hipStream_t s = static_cast<hipStream_t>(stream);

    hipLaunchKernelGGL(scale_rows_kernel, dim3((xrows * dp + 255) / 256), dim3(256), 0, s, X, n1, xrows, d, dp, ls, w.xs,
                       w.ls_pad);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(zero_kernel, dim3((xrows + 255) / 256), dim3(256), 0, s, w.alpha, xrows);
    MPO_LAUNCH_CHECK();
    MPO_HIP(append_factor(w.xs, n, dp, md.amp, noise + kJitter, y_norm, base->L, base->W, base->info, w.Db, w.vb, w.L,
                          w.W, w.alpha, w.info, s));
    if (const int rc = finish_prepared(md, w, plan, X, s)) return rc;
    *model = md;
    return MPO_OK;
    MPO_GUARD_END
}

size_t mpo_gp_score_ws_bytes(const MpoGpModel* model, int64_t m, int k) {
    if (!model || m <= 0 || k < 0 || k > MPO_TOPK_MAX) return 0;
    ScorePlan plan;
    if (score_plan(nullptr, model, m, &plan)) return 0;
    return carve_score_ws(nullptr, m, k, plan.part_elems).used + 256;
}

// `who`: the entry point named in the plan's refusals and the workspace check.
// ei_argmax (mpo_gp_ei_score): +EI instead of -EI in vals, and the top-1 index goes
// to *ei_argmax through the tail of the workspace instead of topk_idx / topk_val.
static int gp_score_impl(const char* who, const MpoGpModel* model, const double* cand, int64_t m, double y_opt,
                  double xi, double kappa, unsigned flags, int64_t* ei_argmax, double* mu,
                  double* sd, double* vals, int k, int64_t* topk_idx, double* topk_val,
                  void* ws, size_t ws_bytes, hipStream_t s) {
    MPO_CHECK_ARG(model && cand, "mpo_gp_acq_score: null model/candidates");
    MPO_CHECK_ARG(m > 0, "mpo_gp_acq_score: m must be > 0");
    MPO_CHECK_ARG((flags & ~7u) == 0 && flags != 0, "mpo_gp_acq_score: bad flags %u", flags);
    MPO_CHECK_ARG(k >= 0 && k <= MPO_TOPK_MAX, "mpo_gp_acq_score: k=%d outside [0,%d]", k, MPO_TOPK_MAX);
    MPO_CHECK_ARG(k == 0 || ei_argmax || (topk_idx && topk_val), "mpo_gp_acq_score: topk outputs required for k>0");
    MPO_CHECK_ARG(k > 0 || mu || sd || vals, "mpo_gp_acq_score: nothing to compute");
    ScorePlan plan;
    if (const int rc = score_plan(who, model, m, &plan)) return rc;
    MPO_CHECK_ARG(ws && ws_bytes >= carve_score_ws(nullptr, m, k, plan.part_elems).used + 256,
                  "%s: workspace too small", who);
    const ScoreWs w = carve_score_ws(ws, m, k, plan.part_elems);
    const int64_t ntiles64 = (m + kBM - 1) / kBM;
    MPO_CHECK_ARG(ntiles64 < (1LL << 31), "mpo_gp_acq_score: too many candidates");
    const int ntiles = (int)ntiles64;
    if (ei_argmax) {
        topk_idx = reinterpret_cast<int64_t*>(w.tail_idx);
        topk_val = w.tail_val;
    }

    ScoreArgs a = model_score_args(*model);
    a.cand = cand;
    a.m = m;
    a.y_opt = y_opt;
    a.xi = xi;
    a.kappa = kappa;
    a.flags = flags;
    a.ei_positive = ei_argmax != nullptr;
    {
        const char* e = getenv("MPO_GP_DEBUG");
        a.dbg = e ? atoi(e) : 0;
    }
    a.mu = mu;
    a.sd = sd;
    a.vals = vals;
    a.k = k;
    a.part_idx = w.part_idx;
    a.part_val = w.part_val;
    a.mq = w.mq;   // the workgroup's own rows, finished inside the scoring kernel
    a.panel = plan.panel;
    a.part = w.part;
    int grid = 0;
    MPO_HIP(launch_scoring(model->dp, model->d, plan, a, ntiles, s, /*fin=*/true, &grid));
    const int nparts = 4 * grid;
    if (k > 0) {
        MPO_HIP(mpo::topk_merge(w.part_idx, w.part_val, nparts, k, flags, w.mid_idx, w.mid_val,
                                reinterpret_cast<long long*>(topk_idx), topk_val, s));
    }
    if (ei_argmax) {
        hipLaunchKernelGGL(argmax_from_topk_kernel, dim3(1), dim3(1), 0, s, w.tail_idx,
                           reinterpret_cast<long long*>(ei_argmax));
        MPO_LAUNCH_CHECK();
    }
    return MPO_OK;
}

int mpo_gp_score_path(const MpoGpModel* model) {
    if (!model) return -MPO_EINVAL;
    ScorePlan plan;
    const int rc = score_plan(nullptr, model, 1, &plan);
    return rc ? -rc : plan.path;
}

int mpo_gp_acq_score(const MpoGpModel* model, const double* cand, int64_t m, double y_opt, double xi,
                     double kappa, unsigned flags, double* mu, double* sd, double* vals, int k,
                     int64_t* topk_idx, double* topk_val, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    return gp_score_impl("mpo_gp_acq_score", model, cand, m, y_opt, xi, kappa, flags, nullptr, mu, sd, vals, k, topk_idx,
                         topk_val, ws, ws_bytes, static_cast<hipStream_t>(stream));
    MPO_GUARD_END
}

int mpo_gp_ei_score(const MpoGpModel* model, const double* cand, int64_t m, double y_opt, double xi,
                    double* mu, double* sd, double* ei, int64_t* argmax, void* ws, size_t ws_bytes,
                    void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(argmax, "mpo_gp_ei_score: null argmax");
    MPO_CHECK_ARG(model && m > 0, "mpo_gp_ei_score: null model or m <= 0");
    return gp_score_impl("mpo_gp_ei_score", model, cand, m, y_opt, xi, 1.96, MPO_ACQ_EI, argmax, mu, sd, ei, 1, nullptr,
                         nullptr, ws, ws_bytes, static_cast<hipStream_t>(stream));
    MPO_GUARD_END
}

// The form mpo_gp_acq_grad launches for this model (mpo::grad_plan, with acq_grad_kernel's
// own static LDS): the launch and mpo_gp_acq_grad_path both ask here.
static int acq_grad_plan(const char* who, const MpoGpModel* model, int* waves, size_t* lds) {
    if (!(model && model->n > 0 && model->d > 0 && model->d <= 32 && model->W)) {
        if (who) mpo::set_error("%s: model not prepared", who);
        return MPO_EINVAL;
    }
    static const size_t st16 = mpo::static_lds_bytes(reinterpret_cast<const void*>(acq_grad_kernel<16>));
    static const size_t st4 = mpo::static_lds_bytes(reinterpret_cast<const void*>(acq_grad_kernel<4>));
    return mpo::grad_plan(who, model->n, st16, st4, waves, lds);
}

int mpo_gp_acq_grad_path(const MpoGpModel* model) {
    int waves = 0;
    size_t lds = 0;
    const int rc = acq_grad_plan(nullptr, model, &waves, &lds);
    return rc ? -rc : waves;
}

int mpo_gp_acq_grad(const MpoGpModel* model, const double* x, int batch, const int32_t* acq, double y_opt,
                    double xi, double kappa, double* f, double* g, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(model && x && acq && f && g, "mpo_gp_acq_grad: null pointer");
    MPO_CHECK_ARG(batch > 0 && batch <= 65535, "mpo_gp_acq_grad: batch=%d outside [1, 65535]", batch);
    int waves = 0;
    size_t lds = 0;
    if (const int rc = acq_grad_plan("mpo_gp_acq_grad", model, &waves, &lds)) return rc;
    const bool wide = waves == 16;
    auto kern = wide ? acq_grad_kernel<16> : acq_grad_kernel<4>;
    MPO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(batch), dim3(wide ? 1024 : 256), lds, static_cast<hipStream_t>(stream),
                       model->n, model->d, mpo::grad_model(*model), x, acq, y_opt, xi, kappa, f, g);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_acq_grad_host(const MpoGpModel* model, const double* x_host, int batch, const int32_t* acq_host,
                         double y_opt, double xi, double kappa, double* f_host, double* g_host, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(x_host && acq_host && f_host && g_host, "mpo_gp_acq_grad_host: null pointer");
    return mpo::pinned_round("mpo_gp_acq_grad_host", stream, x_host, acq_host, f_host, g_host, nullptr,
                             [&](const double* x, const int32_t* acq, double* f, double* g, double*) -> int {
        return mpo_gp_acq_grad(model, x, batch, acq, y_opt, xi, kappa, f, g, stream);
    });
    MPO_GUARD_END
}

}  // extern "C"
