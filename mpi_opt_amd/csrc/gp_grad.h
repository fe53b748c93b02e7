// The polish objectives' shared device code (gp.hip acq_grad_kernel, gp_ps.hip
// acq_ps_grad_kernel): the posterior and its gradient at one point per workgroup, the
// acquisition value and gradient from them, and the rule that picks the kernels' wave form.
#pragma once

#include "mpo_internal.h"
#include "gp_acq_math.h"

namespace mpo {

// What a polish kernel reads of one prepared model.
struct GradModel {
    double amp, y_mean, y_std;
    const double* xs;
    const double* ls;
    const double* alpha;
    const double* W;
    int dp;
};

inline GradModel grad_model(const MpoGpModel& m) {
    return GradModel{m.amp, m.y_mean, m.y_std, m.xs, m.ls, m.alpha, m.W, m.dp};
}

// Posterior and its gradient at the point x [d] under one model, by the whole workgroup of
// NW waves: the objective of skopt's L-BFGS-B polish of the best n_restarts_optimizer
// candidates per acquisition (skopt optimizer.py _tell -> fmin_l_bfgs_b(
// gaussian_acquisition_1D, ..., maxiter=20); GaussianProcessRegressor.predict(
// return_mean_grad, return_std_grad)).  All polishes of one ask step run in lockstep, so one
// launch carries one point per live L-BFGS-B run: one workgroup per point, the posterior as
// in the scoring kernel but with the explicit derivative of k* (skopt gpr.py):
//   dk_i/dx_j  = c_i (x_j - X_ij) / ls_j^2,  c_i = -(5/3) amp (1 + t_i) e^-t_i
//   dmu/dx     = y_std dk^T alpha
//   dsd/dx     = -y_std dk^T (W^T W k*) / sd_n,  W = L^-1
// sm (dynamic LDS): k*, c (n each), v = W k* (n), one per-wave partial of W^T v per wave
// (NW n).  NW = 16 waves per point while (3 + NW) n doubles fit the LDS (n <= ~1000; the
// 4-wave form past it, grad_plan below): the two triangular mat-vecs are the serial work,
// 16 waves cut them 4x.  xp [32], red [NW * 64], ga / gu [NW * 2][32]: the
// caller's static LDS.  Every sum runs in a fixed order given (NW, n, d).
// Threads j < d leave with mu, sd and their component of grad mu, grad sd.  Ends behind a
// barrier: the LDS is free for the next model.
// TAIL_UNROLL > 0 bounds the unroll of the last sum over the NW * 2 groups (the same additions in
// the same order): a caller that runs this routine inside a loop of runtime length
// (gp_committee.hip) has less register room than straight-line code; 0 leaves the loop to the
// compiler, as the callers that name no value get it.
template <int NW, int TAIL_UNROLL = 0>
__device__ __forceinline__ void posterior_grad(const GradModel& gm, int n, int d, const double* __restrict__ x,
                                               double* sm, double* xp, double* red, double (*ga)[32],
                                               double (*gu)[32], double& mu, double& sd, double& mu_g, double& sd_g) {
    constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;
    double* kk = sm;              // [n]
    double* cc = kk + n;          // [n]
    double* vv = cc + n;          // [n]
    double* up = vv + n;          // [NW][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double amp = gm.amp;
    const double* __restrict__ xs = gm.xs;
    const double* __restrict__ alpha = gm.alpha;
    const double* __restrict__ W = gm.W;
    const int dp = gm.dp;
    if (tid < 32) xp[tid] = tid < d ? x[tid] / gm.ls[tid] : 0.0;   // x / ls
    __syncthreads();

    // k*, c and mu_n partials
    double mu_part = 0.0;
    for (int i = tid; i < n; i += kGradThreads) {
        double r2 = 0.0;
        for (int j = 0; j < d; ++j) {
            const double t = xp[j] - xs[(size_t)i * dp + j];
            r2 = fma(t, t, r2);
        }
        const double t = kSqrt5 * sqrt(r2);
        const double e = exp(-t);
        const double k = amp * ((1.0 + t + t * t * (1.0 / 3.0)) * e);
        kk[i] = k;
        cc[i] = (-5.0 / 3.0) * amp * (1.0 + t) * e;
        mu_part = fma(k, alpha[i], mu_part);
    }
    for (int i = tid; i < NW * n; i += kGradThreads) up[i] = 0.0;
    __syncthreads();

    // v = W k* (rows per wave, lanes across the row), q = ||v||^2
    double q_part = 0.0;
    for (int r = wave; r < n; r += NW) {
        double s = 0.0;
        for (int c = lane; c <= r; c += 64) s = fma(W[(size_t)r * n + c], kk[c], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) vv[r] = s;
        q_part = fma(s, s, q_part);     // identical in every lane: count lane 0 only
    }
    if (lane != 0) q_part = 0.0;
    __syncthreads();

    // u = W^T v: wave w accumulates rows r = w (mod NW) into its own partial
    double* uw = up + (size_t)wave * n;
    for (int r = wave; r < n; r += NW) {
        const double vr = vv[r];
        for (int c = lane; c <= r; c += 64) uw[c] = fma(W[(size_t)r * n + c], vr, uw[c]);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kGradThreads) {
        double u = up[i];
#pragma unroll
        for (int w = 1; w < NW; ++w) u += up[(size_t)w * n + i];
        up[i] = u;
    }

    // block sums of mu_n and q
    red[tid] = mu_part;
    __syncthreads();
    for (int s = kGradThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double mu_n = red[0];
    __syncthreads();
    red[tid] = q_part;
    __syncthreads();
    for (int s = kGradThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double q = red[0];

    // dk^T alpha and dk^T u per dimension: thread (grp, j) sums observations grp (mod kGroups)
    {
        const int j = tid & 31, grp = tid >> 5;
        double sa = 0.0, su = 0.0;
        if (j < d) {
            for (int i = grp; i < n; i += kGroups) {
                const double t = cc[i] * (xp[j] - xs[(size_t)i * dp + j]);
                sa = fma(t, alpha[i], sa);
                su = fma(t, up[i], su);
            }
        }
        ga[grp][j] = sa;
        gu[grp][j] = su;
    }
    __syncthreads();

    if (tid < d) {
        const int j = tid;
        double sa = 0.0, su = 0.0;
        if constexpr (TAIL_UNROLL > 0) {
#pragma unroll TAIL_UNROLL
            for (int grp = 0; grp < kGroups; ++grp) {
                sa += ga[grp][j];
                su += gu[grp][j];
            }
        } else {
            for (int grp = 0; grp < kGroups; ++grp) {
                sa += ga[grp][j];
                su += gu[grp][j];
            }
        }
        const double inv_ls = 1.0 / gm.ls[j];
        double var = amp - q;
        if (var < 0.0) var = 0.0;
        const double sd_n = sqrt(var);
        mu = gm.y_std * mu_n + gm.y_mean;
        sd = sd_n * gm.y_std;
        mu_g = gm.y_std * sa * inv_ls;
        sd_g = sd_n > 0.0 ? -gm.y_std * su * inv_ls / sd_n : 0.0;
    }
    __syncthreads();
}

// The minimised value fv and one gradient component gv of acquisition a (MPO_ACQ_LCB,
// MPO_ACQ_PI, anything else: EI) from the posterior (mu, sd) and its gradient component
// (mu_g, sd_g): skopt's gaussian_lcb / gaussian_pi / gaussian_ei(return_grad=True).
__device__ __forceinline__ void acq_value_grad(int a, double mu, double sd, double mu_g, double sd_g, double y_opt,
                                               double xi, double kappa, double& fv, double& gv) {
    if (a == (int)MPO_ACQ_LCB) {
        fv = mu - kappa * sd;
        gv = mu_g - kappa * sd_g;
    } else if (sd <= 0.0) {
        fv = 0.0;
        gv = 0.0;
    } else {
        const double improve = y_opt - xi - mu;
        const double z = improve / sd;
        const double cdf = ndtr(z), pdf = norm_pdf(z);
        const double improve_g = (-mu_g * sd - sd_g * improve) / (sd * sd);
        if (a == (int)MPO_ACQ_PI) {
            fv = -cdf;
            gv = -(improve_g * pdf);
        } else {
            const double cdf_g = improve_g * pdf;
            const double pdf_g = -improve * cdf_g;
            fv = -(improve * cdf + sd * pdf);
            gv = -((-mu_g * cdf - pdf_g) + (sd_g * pdf + pdf_g));
        }
    }
}

// The form of a polish kernel pair for n observations: *waves = 16 per point while its LDS
// fits, 4 past it, and *lds the dynamic LDS bytes (19 n or 7 n doubles).  st16 / st4:
// the two kernels' static LDS (reduction rows, gradient tiles), read from their
// code objects.  `who` (may be NULL: no message) names the entry point in a refusal.  The
// one place the choice is made: the launches and the *_grad_path queries all ask here.
inline int grad_plan(const char* who, int n, size_t st16, size_t st4, int* waves, size_t* lds) {
    const size_t lds16 = (size_t)19 * n * sizeof(double), lds4 = (size_t)7 * n * sizeof(double);
    const bool wide = lds16 + st16 <= kMaxLds;
    if (!wide && lds4 + st4 > kMaxLds) {
        if (who) set_error("%s: n=%d too large", who, n);
        return MPO_ENOTSUP;
    }
    *waves = wide ? 16 : 4;
    *lds = wide ? lds16 : lds4;
    return MPO_OK;
}

}  // namespace mpo
