// gp_committee.hip -- a committee of exact GPs as one surrogate, for gfx950 (MI355X): the
// robust Bayesian committee machine (rBCM; Deisenroth & Ng, "Distributed Gaussian
// Processes", ICML 2015).  NOT the reference's semantics: skopt fits one GP to all told
// points (Coordinator.fit, coordinator.py:63-79); this serves the opt-in
// Optimizer(surrogate="committee") past the single GP's 2048 observations.
// E prepared models ("experts") over disjoint parts of the observations share amp, the
// length scales and ONE target normalisation (y_mean, y_std).  At a point x, in normalised
// units, expert e gives the mean m_e and the variance v_e = amp - q_e; with
//   r_e  = v_e / amp, clamped to [2^-52, 1]     (a clamped r_e has zero derivative; r_e = 1
//                                                 contributes nothing)
//   b_e  = -ln(r_e) / 2
//   S    = sum_e b_e (1 / r_e - 1)               P = 1 + S >= 1
//   M    = sum_e b_e m_e / r_e
// the committee's posterior is mu = y_mean + y_std M / P, sd = y_std sqrt(amp / P), and
// EI / PI / LCB are gp_acq_math.h's on (mu, sd).  Both sums run over e = 0 .. E-1 in that
// order from 0, one term after the other: the same bits whatever m, the grid or the batch.
//
// Kernels
//   committee_fold_kernel<false>  S, M += expert e's terms from its (mu, sd) rows: 16 B read,
//                                 16 B read and written per candidate
//   committee_fold_kernel<true>   the last expert's fold and the finish in one pass: mu, sd,
//                                 the acquisition rows and per-wave top-k lists
//   committee_grad_kernel         value + gradient at a few points (the polish objective):
//                                 mpo::posterior_grad expert after expert on the same LDS,
//                                 one workgroup per point

#include "gp_grad.h"
#include "gp_topk.h"

#include <algorithm>
#include <vector>

namespace {

using mpo::acq_value_grad;
using mpo::GradModel;
using mpo::posterior_grad;
using mpo::WaveTopk;

constexpr double kRMin = 0x1p-52;

// Memory-bound passes: 256 threads per workgroup, one candidate per lane and step, at most
// 4 workgroups for each of the 256 CUs (gp_ps.hip's finish pass).
constexpr int kFoldThreads = 256;
constexpr int kFoldGridCap = 1024;

// Expert e's terms of S and M from its posterior (mu, sd) in the units of y.  One place: the
// fold over candidates and the polish objective alike.  r: the clamped ratio; live: false
// where the clamp holds it (its derivative is then zero).
struct Term {
    double r, beta, ir, m;
    bool live;
};
__device__ __forceinline__ Term committee_term(double mu, double sd, double amp, double y_mean, double y_std) {
    Term t;
    t.m = (mu - y_mean) / y_std;
    const double sn = sd / y_std;
    double r = sn * sn / amp;
    t.live = r > kRMin && r < 1.0;
    if (!(r > kRMin)) r = kRMin;
    if (r > 1.0) r = 1.0;
    t.r = r;
    t.beta = -0.5 * log(r);
    t.ir = 1.0 / r;
    return t;
}

// first: S and M start from 0 (not read).  LAST: this expert closes the sums and the pass
// writes the committee's outputs: mu, sd [m], vals [3][m] (rows EI, PI, LCB; rows of unset
// flags untouched), each optional, and part_idx / part_val [waves][3][k], the layout
// mpo::topk_merge reads.  A candidate's outputs depend on its own inputs only.
template <bool LAST>
__global__ __launch_bounds__(kFoldThreads) void committee_fold_kernel(
        const double* __restrict__ mu_e, const double* __restrict__ sd_e, long long m, int first, double amp,
        double y_mean, double y_std, double* __restrict__ S, double* __restrict__ M, double y_opt, double xi,
        double kappa, unsigned flags, double* __restrict__ mu, double* __restrict__ sd, double* __restrict__ vals,
        int k, long long* __restrict__ part_idx, double* __restrict__ part_val) {
    const long long stride = (long long)gridDim.x * kFoldThreads;
    if constexpr (!LAST) {
        for (long long i = (long long)blockIdx.x * kFoldThreads + threadIdx.x; i < m; i += stride) {
            const Term t = committee_term(mu_e[i], sd_e[i], amp, y_mean, y_std);
            const double s0 = first ? 0.0 : S[i], m0 = first ? 0.0 : M[i];
            S[i] = s0 + t.beta * (t.ir - 1.0);
            M[i] = m0 + t.beta * t.ir * t.m;
        }
    } else {
        const bool ei = flags & MPO_ACQ_EI, pi = flags & MPO_ACQ_PI, lcb = flags & MPO_ACQ_LCB;
        WaveTopk te, tp, tl;
        te.init();
        tp.init();
        tl.init();
        // whole steps for every lane of the wave: offer() shuffles across all 64
        const long long start = (long long)blockIdx.x * kFoldThreads + (threadIdx.x & ~63);
        for (long long base = start; base < m; base += stride) {
            const long long i = base + (threadIdx.x & 63);
            const bool live = i < m;
            double ve = __builtin_huge_val(), vp = __builtin_huge_val(), vl = __builtin_huge_val();
            if (live) {
                const Term t = committee_term(mu_e[i], sd_e[i], amp, y_mean, y_std);
                const double s0 = first ? 0.0 : S[i], m0 = first ? 0.0 : M[i];
                const double P = 1.0 + (s0 + t.beta * (t.ir - 1.0));
                const double Mh = (m0 + t.beta * t.ir * t.m) / P;
                const double cmu = y_mean + y_std * Mh;
                const double csd = y_std * sqrt(amp / P);
                if (mu) mu[i] = cmu;
                if (sd) sd[i] = csd;
                double gv;
                if (ei) {
                    acq_value_grad((int)MPO_ACQ_EI, cmu, csd, 0.0, 0.0, y_opt, xi, kappa, ve, gv);
                    if (vals) vals[i] = ve;
                }
                if (pi) {
                    acq_value_grad((int)MPO_ACQ_PI, cmu, csd, 0.0, 0.0, y_opt, xi, kappa, vp, gv);
                    if (vals) vals[m + i] = vp;
                }
                if (lcb) {
                    acq_value_grad((int)MPO_ACQ_LCB, cmu, csd, 0.0, 0.0, y_opt, xi, kappa, vl, gv);
                    if (vals) vals[2 * m + i] = vl;
                }
            }
            if (k > 0) {
                const long long ci = live ? i : 0x7fffffffffffffffLL;
                if (ei) te.offer(ve, ci, k);
                if (pi) tp.offer(vp, ci, k);
                if (lcb) tl.offer(vl, ci, k);
            }
        }
        if (k > 0 && (threadIdx.x & 63) == 0) {
            const size_t part = (size_t)blockIdx.x * (kFoldThreads / 64) + (threadIdx.x >> 6);
            if (ei) te.store(part_idx, part_val, (part * 3 + 0) * k, k);
            if (pi) tp.store(part_idx, part_val, (part * 3 + 1) * k, k);
            if (lcb) tl.store(part_idx, part_val, (part * 3 + 2) * k, k);
        }
    }
}

// What committee_grad_kernel reads of the committee: one kernel argument.
struct CommitteeGrad {
    const double* xs[MPO_COMMITTEE_MAX];
    const double* alpha[MPO_COMMITTEE_MAX];
    const double* W[MPO_COMMITTEE_MAX];
    const double* ls[MPO_COMMITTEE_MAX];   // equal values (mpo_gp_committee_check); each expert reads its own
    int n[MPO_COMMITTEE_MAX];
    double amp, y_mean, y_std;
    int dp, E;
};

// One workgroup per point b: f[b] and g[b][d] of acquisition acq[b] (MPO_ACQ_LCB, MPO_ACQ_PI,
// anything else: EI) under the committee's posterior.  LDS as acq_grad_kernel, (3 + NW) n_max
// doubles, used by one expert after the other.  With m_e, r_e and their gradient components
// (m_e', r_e' = 2 sn_e sn_e' / amp, zero where r_e is clamped):
//   b_e' = -r_e' / (2 r_e)
//   S'   = sum_e b_e' (1 / r_e - 1) - b_e r_e' / r_e^2
//   M'   = sum_e (b_e' m_e + b_e m_e') / r_e - b_e m_e r_e' / r_e^2
//   mu'  = y_std (M' - (M / P) S') / P            sd' = -sd S' / (2 P)
template <int NW>
__global__ __launch_bounds__(NW * 64) void committee_grad_kernel(
        int d, CommitteeGrad cm, const double* __restrict__ x, const int32_t* __restrict__ acq, double y_opt,
        double xi, double kappa, double* __restrict__ f, double* __restrict__ g) {
    extern __shared__ double sm[];
    __shared__ double xp[32];
    constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;
    __shared__ double red[kGradThreads];
    __shared__ double ga[kGroups][32], gu[kGroups][32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* xb = x + (size_t)b * d;
    const double amp = cm.amp, y_mean = cm.y_mean, y_std = cm.y_std;

    double S = 0.0, M = 0.0, S_g = 0.0, M_g = 0.0;
#pragma unroll 1    // E is a runtime count: one copy of posterior_grad, its last sum unrolled by 4
    for (int e = 0; e < cm.E; ++e) {
        double mu = 0.0, sd = 0.0, mu_g = 0.0, sd_g = 0.0;
        const GradModel gm{amp, y_mean, y_std, cm.xs[e], cm.ls[e], cm.alpha[e], cm.W[e], cm.dp};
        posterior_grad<NW, 4>(gm, cm.n[e], d, xb, sm, xp, red, ga, gu, mu, sd, mu_g, sd_g);
        if (tid < d) {
            const Term t = committee_term(mu, sd, amp, y_mean, y_std);
            const double m_g = mu_g / y_std;
            const double r_g = t.live ? 2.0 * (sd / y_std) * (sd_g / y_std) / amp : 0.0;
            const double beta_g = -0.5 * r_g * t.ir;
            const double w = t.beta * t.ir;          // b_e / r_e
            S += t.beta * (t.ir - 1.0);
            M += w * t.m;
            S_g += beta_g * (t.ir - 1.0) - w * t.ir * r_g;
            M_g += (beta_g * t.m + t.beta * m_g) * t.ir - w * t.m * t.ir * r_g;
        }
    }
    if (tid < d) {
        const double P = 1.0 + S;
        const double Mh = M / P;
        const double cmu = y_mean + y_std * Mh;
        const double csd = y_std * sqrt(amp / P);
        const double cmu_g = y_std * (M_g - Mh * S_g) / P;
        const double csd_g = -0.5 * csd * S_g / P;
        double fv, gv;
        acq_value_grad(acq[b], cmu, csd, cmu_g, csd_g, y_opt, xi, kappa, fv, gv);
        g[(size_t)b * d + tid] = gv;
        if (tid == 0) f[b] = fv;
    }
}

// ---------------------------------------------------------------------------
// The host-side refusals of every entry point: MPO_OK, or the code with the message set
// under `who` (null: a silent query).  Length scales are device data: mpo_gp_committee_check
// compares them.
#define COMMITTEE_REFUSE(rc, ...)                      \
    do {                                               \
        if (who) {                                     \
            char msg_[256];                            \
            snprintf(msg_, sizeof msg_, __VA_ARGS__);  \
            mpo::set_error("%s: %s", who, msg_);       \
        }                                              \
        return rc;                                     \
    } while (0)

int committee_ok(const char* who, const MpoGpModel* models, int E) {
    if (E < 1 || E > MPO_COMMITTEE_MAX)
        COMMITTEE_REFUSE(MPO_EINVAL, "E=%d outside [1, %d]", E, MPO_COMMITTEE_MAX);
    if (!models) COMMITTEE_REFUSE(MPO_EINVAL, "null models");
    for (int e = 0; e < E; ++e) {
        const MpoGpModel& m = models[e];
        if (m.n > mpo::kMaxObs)
            COMMITTEE_REFUSE(MPO_ENOTSUP, "expert %d: n=%d exceeds the supported maximum of %d observations", e, m.n,
                          mpo::kMaxObs);
        if (!(m.n > 0 && m.d > 0 && m.d <= 32 && m.dp >= m.d && m.np16 >= m.n && m.np16 - m.n < 16 &&
              (m.np16 & 15) == 0 && m.xs && m.ls && m.alpha && m.W && m.amp > 0.0 && m.y_std > 0.0))
            COMMITTEE_REFUSE(MPO_EINVAL, "expert %d: null or unprepared model", e);
        const MpoGpModel& m0 = models[0];
        if (m.d != m0.d || m.dp != m0.dp)
            COMMITTEE_REFUSE(MPO_EINVAL, "expert %d differs in shape (d %d / %d, dp %d / %d)", e, m.d, m0.d, m.dp, m0.dp);
        if (m.amp != m0.amp) COMMITTEE_REFUSE(MPO_EINVAL, "expert %d differs in amp (%.17g / %.17g)", e, m.amp, m0.amp);
        if (m.y_mean != m0.y_mean || m.y_std != m0.y_std)
            COMMITTEE_REFUSE(MPO_EINVAL, "expert %d differs in the target normalisation (y_mean %.17g / %.17g, "
                          "y_std %.17g / %.17g)", e, m.y_mean, m0.y_mean, m.y_std, m0.y_std);
    }
    return MPO_OK;
}

inline int fold_grid(int64_t m) {
    return (int)std::min<int64_t>((m + kFoldThreads - 1) / kFoldThreads, kFoldGridCap);
}

// The workspace of mpo_gp_committee_score: the experts' scoring passes run one after the
// other and share `score`; four rows of m doubles and the top-k lists, whatever E.
struct CommitteeWs {
    void* score;
    size_t score_bytes;
    double* S;        // [m]
    double* M;        // [m]
    double* mu;       // [m] one expert's
    double* sd;       // [m]
    long long* part_idx;
    double* part_val;
    long long* mid_idx;
    double* mid_val;
    size_t used;
};

// ws = null: the size query.  False when an expert's scoring pass refuses the shape.
bool carve_committee_ws(void* ws, const MpoGpModel* models, int E, int64_t m, int k, CommitteeWs* w) {
    size_t score = 0;
    for (int e = 0; e < E; ++e) {
        const size_t se = mpo_gp_score_ws_bytes(&models[e], m, 0);
        if (se == 0) return false;
        score = std::max(score, se);
    }
    const size_t nparts = (size_t)fold_grid(m) * (kFoldThreads / 64);
    const int kk = std::max(k, 1);
    mpo::WsCarver c(ws);
    w->score_bytes = score;
    w->score = c.take<char>(score);
    w->S = c.take<double>((size_t)m);
    w->M = c.take<double>((size_t)m);
    w->mu = c.take<double>((size_t)m);
    w->sd = c.take<double>((size_t)m);
    w->part_idx = c.take<long long>(nparts * 3 * kk);
    w->part_val = c.take<double>(nparts * 3 * kk);
    w->mid_idx = c.take<long long>((size_t)mpo::kTopkMergeGroups * 3 * kk);
    w->mid_val = c.take<double>((size_t)mpo::kTopkMergeGroups * 3 * kk);
    w->used = c.used;
    return true;
}

// The form of committee_grad_kernel for the largest expert (mpo::grad_plan, with this
// kernel's own static LDS).
int committee_grad_plan(const char* who, const MpoGpModel* models, int E, int* waves, size_t* lds) {
    static const size_t st16 = mpo::static_lds_bytes(reinterpret_cast<const void*>(committee_grad_kernel<16>));
    static const size_t st4 = mpo::static_lds_bytes(reinterpret_cast<const void*>(committee_grad_kernel<4>));
    int nmax = 0;
    for (int e = 0; e < E; ++e) nmax = std::max(nmax, (int)models[e].n);
    return mpo::grad_plan(who, nmax, st16, st4, waves, lds);
}

}  // namespace

int mpo::committee_models_ok(const char* who, const MpoGpModel* models, int E) { return committee_ok(who, models, E); }

// ===========================================================================
extern "C" {

size_t mpo_gp_committee_ws_bytes(const MpoGpModel* models, int E, int64_t m, int k) {
    if (committee_ok(nullptr, models, E) || m <= 0 || k < 0 || k > MPO_TOPK_MAX) return 0;
    CommitteeWs w;
    if (!carve_committee_ws(nullptr, models, E, m, k, &w)) return 0;
    return w.used + 256;
}

int mpo_gp_committee_check(const MpoGpModel* models, int E, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_committee_check";
    if (const int rc = committee_ok(who, models, E)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int d = models[0].d;
    std::vector<double> ls((size_t)E * d);
    for (int e = 0; e < E; ++e)
        MPO_HIP(hipMemcpyAsync(ls.data() + (size_t)e * d, models[e].ls, sizeof(double) * d, hipMemcpyDeviceToHost, s));
    MPO_HIP(hipStreamSynchronize(s));
    for (int e = 1; e < E; ++e)
        for (int j = 0; j < d; ++j)
            MPO_CHECK_ARG(ls[(size_t)e * d + j] == ls[j], "%s: expert %d differs in length scale %d (%.17g / %.17g)", who,
                          e, j, ls[(size_t)e * d + j], ls[j]);
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_committee_score(const MpoGpModel* models, int E, const double* cand, int64_t m, double y_opt, double xi,
                           double kappa, unsigned flags, double* mu, double* sd, double* vals, int k,
                           int64_t* topk_idx, double* topk_val, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_committee_score";
    if (const int rc = committee_ok(who, models, E)) return rc;
    MPO_CHECK_ARG(cand, "%s: null candidates", who);
    MPO_CHECK_ARG(m > 0, "%s: m must be > 0", who);
    MPO_CHECK_ARG((flags & ~7u) == 0 && flags != 0, "%s: bad flags %u", who, flags);
    MPO_CHECK_ARG(k >= 0 && k <= MPO_TOPK_MAX, "%s: k=%d outside [0,%d]", who, k, MPO_TOPK_MAX);
    MPO_CHECK_ARG(k == 0 || (topk_idx && topk_val), "%s: topk outputs required for k>0", who);
    MPO_CHECK_ARG(k > 0 || mu || sd || vals, "%s: nothing to compute", who);
    CommitteeWs w;
    MPO_CHECK_ARG(carve_committee_ws(nullptr, models, E, m, k, &w), "%s: mpo_gp_acq_score refuses one of the experts",
                  who);
    MPO_CHECK_ARG(ws && ws_bytes >= w.used + 256, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.used + 256);
    carve_committee_ws(ws, models, E, m, k, &w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MpoGpModel& m0 = models[0];
    const int grid = fold_grid(m);

    // every expert's own scoring path (resident or streamed) into the (mu, sd) rows, one after
    // the other on `stream`, each folded into S and M before the next overwrites the rows
    for (int e = 0; e < E; ++e) {
        if (const int rc = mpo_gp_acq_score(&models[e], cand, m, 0.0, 0.0, 0.0, MPO_ACQ_EI, w.mu, w.sd, nullptr, 0,
                                            nullptr, nullptr, w.score, w.score_bytes, stream))
            return rc;
        if (e + 1 < E)
            hipLaunchKernelGGL(committee_fold_kernel<false>, dim3(grid), dim3(kFoldThreads), 0, s, w.mu, w.sd,
                               (long long)m, (int)(e == 0), m0.amp, m0.y_mean, m0.y_std, w.S, w.M, y_opt, xi, kappa,
                               flags, mu, sd, vals, k, w.part_idx, w.part_val);
        else
            hipLaunchKernelGGL(committee_fold_kernel<true>, dim3(grid), dim3(kFoldThreads), 0, s, w.mu, w.sd,
                               (long long)m, (int)(e == 0), m0.amp, m0.y_mean, m0.y_std, w.S, w.M, y_opt, xi, kappa,
                               flags, mu, sd, vals, k, w.part_idx, w.part_val);
        MPO_LAUNCH_CHECK();
    }
    if (k > 0)
        MPO_HIP(mpo::topk_merge(w.part_idx, w.part_val, grid * (kFoldThreads / 64), k, flags, w.mid_idx, w.mid_val,
                                reinterpret_cast<long long*>(topk_idx), topk_val, s));
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_committee_grad_path(const MpoGpModel* models, int E) {
    if (const int rc = committee_ok(nullptr, models, E)) return -rc;
    int waves = 0;
    size_t lds = 0;
    const int rc = committee_grad_plan(nullptr, models, E, &waves, &lds);
    return rc ? -rc : waves;
}

int mpo_gp_committee_grad(const MpoGpModel* models, int E, const double* x, int batch, const int32_t* acq,
                          double y_opt, double xi, double kappa, double* f, double* g, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_committee_grad";
    if (const int rc = committee_ok(who, models, E)) return rc;
    MPO_CHECK_ARG(x && acq && f && g, "%s: null pointer", who);
    MPO_CHECK_ARG(batch > 0 && batch <= 65535, "%s: batch=%d outside [1, 65535]", who, batch);
    int waves = 0;
    size_t lds = 0;
    if (const int rc = committee_grad_plan(who, models, E, &waves, &lds)) return rc;
    CommitteeGrad cm{};
    cm.E = E;
    cm.amp = models[0].amp;
    cm.y_mean = models[0].y_mean;
    cm.y_std = models[0].y_std;
    cm.dp = models[0].dp;
    for (int e = 0; e < E; ++e) {
        cm.xs[e] = models[e].xs;
        cm.ls[e] = models[e].ls;
        cm.alpha[e] = models[e].alpha;
        cm.W[e] = models[e].W;
        cm.n[e] = models[e].n;
    }
    const bool wide = waves == 16;
    auto kern = wide ? committee_grad_kernel<16> : committee_grad_kernel<4>;
    MPO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(kern, dim3(batch), dim3(wide ? 1024 : 256), lds, static_cast<hipStream_t>(stream), models[0].d,
                       cm, x, acq, y_opt, xi, kappa, f, g);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_committee_grad_host(const MpoGpModel* models, int E, const double* x_host, int batch,
                               const int32_t* acq_host, double y_opt, double xi, double kappa, double* f_host,
                               double* g_host, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_committee_grad_host";
    if (const int rc = committee_ok(who, models, E)) return rc;
    MPO_CHECK_ARG(x_host && acq_host && f_host && g_host, "%s: null pointer", who);
    MPO_CHECK_ARG(batch > 0 && batch <= 65535, "%s: batch=%d outside [1, 65535]", who, batch);
    return mpo::pinned_round(who, stream, x_host, acq_host, f_host, g_host, nullptr,
                             [&](const double* x, const int32_t* acq, double* f, double* g, double*) -> int {
        return mpo_gp_committee_grad(models, E, x, batch, acq, y_opt, xi, kappa, f, g, stream);
    });
    MPO_GUARD_END
}

}  // extern "C"
