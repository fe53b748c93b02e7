// gp_ps.hip -- cost-aware acquisitions EIps / PIps for gfx950 (MI355X): skopt's "expected
// improvement per second" (skopt acquisition.py gaussian_acquisition_1D / _gaussian_acquisition
// with acq_func = "EIps" / "PIps"), reached from Coordinator.ask
// (coordinator.py:46-50) once the optimizer is told (value, time) pairs.
// Two GPs on the same observations: f on the objective, tau on log t.  With
//   a(x)     = -EI_f(x) or -PI_f(x)             (mpo_gp_acq_score's / mpo_gp_acq_grad's value)
//   (mu, s)  = tau's posterior mean / std at x  (original units of log t)
//   inv_t(x) = exp(-mu + s^2 / 2)               (E[1/t] under a log-normal t)
// the minimised value is v = a inv_t and grad v = grad a inv_t + v (-grad mu + s grad s).
//
// Kernels
//   ps_finish_kernel    the elementwise product over m candidates after the two models'
//                       own scoring passes, and per-wave top-k lists
//   acq_ps_grad_kernel  value + gradient at a few points (the polish objective): both
//                       posteriors and their gradients (mpo::posterior_grad, gp_grad.h) in
//                       one launch, one workgroup per point

#include "gp_grad.h"
#include "gp_topk.h"

#include <algorithm>

namespace {

using mpo::acq_value_grad;
using mpo::grad_model;
using mpo::GradModel;
using mpo::lex_less;
using mpo::posterior_grad;
using mpo::WaveTopk;

constexpr unsigned kPsFlags = MPO_ACQ_EI | MPO_ACQ_PI;

// E[1/t] of a log-normal t with log t ~ N(mu, s^2).  One place: the scoring finish and the
// polish objective round alike.
__device__ __forceinline__ double inv_time(double mu, double s) { return exp(fma(0.5 * s, s, -mu)); }

// The finish pass is memory-bound (32 B read, 24 B written per candidate): 256 threads per
// workgroup, one candidate per lane and step, at most 4 workgroups for each of the 256 CUs.
constexpr int kFinThreads = 256;
constexpr int kFinGridCap = 1024;

// a [2][m] (rows EI, PI of fmodel's scoring pass; rows of unset flags are not read), mu / sd
// [m] of tmodel's.  vals [2][m], inv_t [m]: optional.  part_idx / part_val: [waves][3][k],
// the layout mpo::topk_merge reads.  A candidate's outputs depend on its own inputs only.
__global__ __launch_bounds__(kFinThreads) void ps_finish_kernel(
        const double* __restrict__ a, const double* __restrict__ mu, const double* __restrict__ sd, long long m,
        unsigned flags, double* __restrict__ vals, double* __restrict__ inv_t, int k,
        long long* __restrict__ part_idx, double* __restrict__ part_val) {
    const bool ei = flags & MPO_ACQ_EI, pi = flags & MPO_ACQ_PI;
    WaveTopk te, tp;
    te.init();
    tp.init();
    const long long stride = (long long)gridDim.x * kFinThreads;
    // whole steps for every lane of the wave: offer() shuffles across all 64
    const long long first = (long long)blockIdx.x * kFinThreads + (threadIdx.x & ~63);
    for (long long base = first; base < m; base += stride) {
        const long long i = base + (threadIdx.x & 63);
        const bool live = i < m;
        double ve = __builtin_huge_val(), vp = __builtin_huge_val();
        if (live) {
            const double it = inv_time(mu[i], sd[i]);
            if (inv_t) inv_t[i] = it;
            if (ei) {
                ve = a[i] * it;
                if (vals) vals[i] = ve;
            }
            if (pi) {
                vp = a[m + i] * it;
                if (vals) vals[m + i] = vp;
            }
        }
        if (k > 0) {
            const long long ci = live ? i : 0x7fffffffffffffffLL;
            if (ei) te.offer(ve, ci, k);
            if (pi) tp.offer(vp, ci, k);
        }
    }
    if (k > 0 && (threadIdx.x & 63) == 0) {
        const size_t part = (size_t)blockIdx.x * (kFinThreads / 64) + (threadIdx.x >> 6);
        if (ei) te.store(part_idx, part_val, (part * 3 + 0) * k, k);
        if (pi) tp.store(part_idx, part_val, (part * 3 + 1) * k, k);
    }
}

// ---------------------------------------------------------------------------
// One workgroup per point b: f[b] = v, g[b][d] = grad v of acquisition acq[b] (MPO_ACQ_EI or
// MPO_ACQ_PI; anything else gives NaN), parts[b] = (a, inv_t, mu_t, s_t) when parts is set.
// LDS as acq_grad_kernel: (3 + NW) n doubles, used by one model after the other.
template <int NW>
__global__ __launch_bounds__(NW * 64) void acq_ps_grad_kernel(
        int n, int d, GradModel fm, GradModel tm, const double* __restrict__ x, const int32_t* __restrict__ acq,
        double y_opt, double xi, double* __restrict__ f, double* __restrict__ g, double* __restrict__ parts) {
    extern __shared__ double sm[];
    __shared__ double xp[32];
    constexpr int kGradThreads = NW * 64, kGroups = kGradThreads / 32;
    __shared__ double red[kGradThreads];
    __shared__ double ga[kGroups][32], gu[kGroups][32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* xb = x + (size_t)b * d;

    double mu = 0.0, sd = 0.0, mu_g = 0.0, sd_g = 0.0;
    posterior_grad<NW>(fm, n, d, xb, sm, xp, red, ga, gu, mu, sd, mu_g, sd_g);
    double mt = 0.0, st = 0.0, mt_g = 0.0, st_g = 0.0;
    posterior_grad<NW>(tm, n, d, xb, sm, xp, red, ga, gu, mt, st, mt_g, st_g);

    if (tid < d) {
        const int a = acq[b];
        double av, ag;     // the plain acquisition, as mpo_gp_acq_grad computes it
        acq_value_grad(a, mu, sd, mu_g, sd_g, y_opt, xi, 0.0, av, ag);
        if (a != (int)MPO_ACQ_EI && a != (int)MPO_ACQ_PI) av = ag = __builtin_nan("");
        const double it = inv_time(mt, st);
        const double v = av * it;
        g[(size_t)b * d + tid] = fma(ag, it, v * fma(st, st_g, -mt_g));
        if (tid == 0) {
            f[b] = v;
            if (parts) {
                parts[(size_t)b * 4 + 0] = av;
                parts[(size_t)b * 4 + 1] = it;
                parts[(size_t)b * 4 + 2] = mt;
                parts[(size_t)b * 4 + 3] = st;
            }
        }
    }
}

// ---------------------------------------------------------------------------
bool model_ok(const MpoGpModel* m) {
    return m && m->n > 0 && m->n <= mpo::kMaxObs && m->d > 0 && m->d <= 32 && m->dp >= m->d && m->xs && m->ls &&
           m->alpha && m->W;
}

bool pair_ok(const char* who, const MpoGpModel* fm, const MpoGpModel* tm) {
    if (!model_ok(fm) || !model_ok(tm)) {
        if (who) mpo::set_error("%s: null or unprepared model", who);
        return false;
    }
    if (fm->n != tm->n || fm->d != tm->d) {
        if (who) mpo::set_error("%s: the two models differ in shape (n %d / %d, d %d / %d)", who, fm->n, tm->n, fm->d,
                                tm->d);
        return false;
    }
    return true;
}

inline int fin_grid(int64_t m) { return (int)std::min<int64_t>((m + kFinThreads - 1) / kFinThreads, kFinGridCap); }

// The workspace of mpo_gp_acq_ps_score: the two scoring passes run one after the other and
// share `score`; the rows and the top-k lists are the finish pass's.
struct PsWs {
    void* score;
    size_t score_bytes;
    double* a;        // [2][m]
    double* mu;       // [m]
    double* sd;       // [m]
    long long* part_idx;
    double* part_val;
    long long* mid_idx;
    double* mid_val;
    size_t used;
};

// ws = null: the size query.  False when either model's scoring pass refuses the shape.
bool carve_ps_ws(void* ws, const MpoGpModel* fm, const MpoGpModel* tm, int64_t m, int k, PsWs* w) {
    const size_t sf = mpo_gp_score_ws_bytes(fm, m, 0), st = mpo_gp_score_ws_bytes(tm, m, 0);
    if (sf == 0 || st == 0) return false;
    const size_t nparts = (size_t)fin_grid(m) * (kFinThreads / 64);
    const int kk = std::max(k, 1);
    mpo::WsCarver c(ws);
    w->score_bytes = std::max(sf, st);
    w->score = c.take<char>(w->score_bytes);
    w->a = c.take<double>((size_t)2 * m);
    w->mu = c.take<double>((size_t)m);
    w->sd = c.take<double>((size_t)m);
    w->part_idx = c.take<long long>(nparts * 3 * kk);
    w->part_val = c.take<double>(nparts * 3 * kk);
    w->mid_idx = c.take<long long>((size_t)mpo::kTopkMergeGroups * 3 * kk);
    w->mid_val = c.take<double>((size_t)mpo::kTopkMergeGroups * 3 * kk);
    w->used = c.used;
    return true;
}

// The form of acq_ps_grad_kernel for n observations (mpo::grad_plan, with this kernel's own
// static LDS).
int ps_grad_plan(const char* who, int n, int* waves, size_t* lds) {
    static const size_t st16 = mpo::static_lds_bytes(reinterpret_cast<const void*>(acq_ps_grad_kernel<16>));
    static const size_t st4 = mpo::static_lds_bytes(reinterpret_cast<const void*>(acq_ps_grad_kernel<4>));
    return mpo::grad_plan(who, n, st16, st4, waves, lds);
}

}  // namespace

// ===========================================================================
extern "C" {

size_t mpo_gp_acq_ps_ws_bytes(const MpoGpModel* fmodel, const MpoGpModel* tmodel, int64_t m, int k) {
    if (!pair_ok(nullptr, fmodel, tmodel) || m <= 0 || k < 0 || k > MPO_TOPK_MAX) return 0;
    PsWs w;
    if (!carve_ps_ws(nullptr, fmodel, tmodel, m, k, &w)) return 0;
    return w.used + 256;
}

int mpo_gp_acq_ps_score(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* cand, int64_t m,
                        double y_opt, double xi, unsigned flags, double* vals, double* inv_t, int k,
                        int64_t* topk_idx, double* topk_val, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_acq_ps_score";
    if (!pair_ok(who, fmodel, tmodel)) return MPO_EINVAL;
    MPO_CHECK_ARG(cand, "%s: null candidates", who);
    MPO_CHECK_ARG(m > 0, "%s: m must be > 0", who);
    MPO_CHECK_ARG((flags & ~kPsFlags) == 0 && flags != 0, "%s: bad flags %u (EI | PI)", who, flags);
    MPO_CHECK_ARG(k >= 0 && k <= MPO_TOPK_MAX, "%s: k=%d outside [0,%d]", who, k, MPO_TOPK_MAX);
    MPO_CHECK_ARG(k == 0 || (topk_idx && topk_val), "%s: topk outputs required for k>0", who);
    MPO_CHECK_ARG(k > 0 || vals || inv_t, "%s: nothing to compute", who);
    PsWs w;
    MPO_CHECK_ARG(carve_ps_ws(nullptr, fmodel, tmodel, m, k, &w), "%s: mpo_gp_acq_score refuses one of the models",
                  who);
    MPO_CHECK_ARG(ws && ws_bytes >= w.used + 256, "%s: workspace too small", who);
    carve_ps_ws(ws, fmodel, tmodel, m, k, &w);
    hipStream_t s = static_cast<hipStream_t>(stream);

    // the two models' own scoring paths (resident or streamed), one after the other on `stream`
    if (const int rc = mpo_gp_acq_score(fmodel, cand, m, y_opt, xi, 0.0, flags, nullptr, nullptr, w.a, 0, nullptr,
                                        nullptr, w.score, w.score_bytes, stream))
        return rc;
    if (const int rc = mpo_gp_acq_score(tmodel, cand, m, 0.0, 0.0, 0.0, MPO_ACQ_EI, w.mu, w.sd, nullptr, 0, nullptr,
                                        nullptr, w.score, w.score_bytes, stream))
        return rc;
    const int grid = fin_grid(m);
    hipLaunchKernelGGL(ps_finish_kernel, dim3(grid), dim3(kFinThreads), 0, s, w.a, w.mu, w.sd, (long long)m, flags,
                       vals, inv_t, k, w.part_idx, w.part_val);
    MPO_LAUNCH_CHECK();
    if (k > 0)
        MPO_HIP(mpo::topk_merge(w.part_idx, w.part_val, grid * (kFinThreads / 64), k, flags, w.mid_idx, w.mid_val,
                                reinterpret_cast<long long*>(topk_idx), topk_val, s));
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_acq_ps_grad_path(const MpoGpModel* fmodel, const MpoGpModel* tmodel) {
    if (!pair_ok(nullptr, fmodel, tmodel)) return -MPO_EINVAL;
    int waves = 0;
    size_t lds = 0;
    const int rc = ps_grad_plan(nullptr, fmodel->n, &waves, &lds);
    return rc ? -rc : waves;
}

int mpo_gp_acq_ps_grad(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* x, int batch,
                       const int32_t* acq, double y_opt, double xi, double* f, double* g, double* parts,
                       void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_acq_ps_grad";
    if (!pair_ok(who, fmodel, tmodel)) return MPO_EINVAL;
    MPO_CHECK_ARG(x && acq && f && g, "%s: null pointer", who);
    MPO_CHECK_ARG(batch > 0 && batch <= 65535, "%s: batch=%d outside [1, 65535]", who, batch);
    int waves = 0;
    size_t lds = 0;
    if (const int rc = ps_grad_plan(who, fmodel->n, &waves, &lds)) return rc;
    const bool wide = waves == 16;
    auto kern = wide ? acq_ps_grad_kernel<16> : acq_ps_grad_kernel<4>;
    MPO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    hipLaunchKernelGGL(kern, dim3(batch), dim3(wide ? 1024 : 256), lds, static_cast<hipStream_t>(stream), fmodel->n,
                       fmodel->d, grad_model(*fmodel), grad_model(*tmodel), x, acq, y_opt, xi, f, g, parts);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_acq_ps_grad_host(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* x_host, int batch,
                            const int32_t* acq_host, double y_opt, double xi, double* f_host, double* g_host,
                            double* parts_host, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_acq_ps_grad_host";
    if (!pair_ok(who, fmodel, tmodel)) return MPO_EINVAL;
    MPO_CHECK_ARG(x_host && acq_host && f_host && g_host, "%s: null pointer", who);
    MPO_CHECK_ARG(batch > 0 && batch <= 65535, "%s: batch=%d outside [1, 65535]", who, batch);
    return mpo::pinned_round(who, stream, x_host, acq_host, f_host, g_host, parts_host,
                             [&](const double* x, const int32_t* acq, double* f, double* g, double* parts) -> int {
        for (int b = 0; b < batch; ++b)
            MPO_CHECK_ARG(acq_host[b] == (int32_t)MPO_ACQ_EI || acq_host[b] == (int32_t)MPO_ACQ_PI,
                          "%s: acq[%d]=%d is neither MPO_ACQ_EI nor MPO_ACQ_PI", who, b, acq_host[b]);
        return mpo_gp_acq_ps_grad(fmodel, tmodel, x, batch, acq, y_opt, xi, f, g, parts, stream);
    });
    MPO_GUARD_END
}

}  // extern "C"
