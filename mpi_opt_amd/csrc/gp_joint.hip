// gp_joint.hip -- the joint posterior of a prepared GP over m <= MPO_JOINT_MAX query
// points (gfx950, fp64 v_mfma_f64_16x16x4): covariance, correlated samples and the
// per-sample argmin (mpo_gp_posterior_cov, mpo_gp_sample).
//
// With c the query points / length_scale, K* = amp Matern52(|c - xs|) [m][n] and
// W = L^-1 of the model:
//   joint_v_kernel      V = K* W^T [mp][np] and mu_n = K* alpha          (workspace)
//   joint_cov_kernel    Sigma_n = amp Matern52(|c_I - c_J|) - V V^T, lower 16 x 16 tiles
//                       and their mirrors; cov = y_std^2 Sigma_n (no noise term: skopt
//                       zeroes the WhiteKernel after the fit)
//   mpo::blocked_chol   Lc Lc^T = Sigma_n + jitter amp I on the matrix padded to 32 with
//                       identity (the bc_* steps of mpo_gp_prepare, gp.hip)
//   joint_sample_kernel S[r][i] = mu[i] + y_std sum_{j<=i} Lc[i][j] Z[j][r] and the
//                       per-workgroup (min, index) of every draw
//   mpo::argmin_fold    the workgroups' partials of a draw folded in order (gp_paths.hip)
// mp = m rounded up to 32, np = the model's np16.  Only the plain W of the model is
// read, never wfrag: the same kernels serve a resident, a streamed, an appended and a
// from_factor model.  Every sum runs in a fixed order given (m, n, s): the launch
// geometry is a function of those alone, so two runs give the same bits.
//
// f64 16x16x4 operands: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 q.
#include "mpo_internal.h"
#include "gp_acq_math.h"

#include <algorithm>
#include <cmath>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

using mpo::lex_less;   // gp_acq_math.h
using mpo::matern52;  // the Matern of bc_kmat_kernel (mpo_internal.h)

constexpr int kPanel = 256;           // observations per K* panel / columns of V per workgroup
constexpr int kKsLd = kPanel + 2;     // LDS row stride of the panel: 16 rows on 16 distinct bank pairs
constexpr int kCsLd = 33;             // LDS row stride of the scaled query tile (dp <= 32)

// Workgroup (ct, J): the 16 query points of tile ct, columns j in [256 J, 256 J + 256) of V.
// It walks the K* panels p = 0 .. J (direct differences, Matern per pair, into the LDS) and
// multiplies only the lower-triangular k-steps of W: V[c][j] = sum_{i <= j} K*[c][i] W[j][i].
// The workgroups of the last J see every panel and also sum mu_n = K* alpha: 16 threads per
// query point, thread `sub` takes i = sub, sub + 16, .. in order, then a fixed butterfly.
// J == 0 stores the scaled query points (rows >= m repeat row m - 1; nothing reads them
// past the identity padding).
__global__ __launch_bounds__(256) void joint_v_kernel(const double* __restrict__ cand, int m, int d, int dp,
                                                      const double* __restrict__ ls, const double* __restrict__ xs,
                                                      const double* __restrict__ alpha, const double* __restrict__ W,
                                                      int n, int np, double amp, double* __restrict__ V,
                                                      double* __restrict__ mu_n, double* __restrict__ cs_out) {
    __shared__ double ks[16 * kKsLd];
    __shared__ double cs[16 * kCsLd];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = blockIdx.x, J = blockIdx.y;
    const bool with_mu = J == (int)gridDim.y - 1;

    for (int e = tid; e < 16 * dp; e += 256) {
        const int r = e / dp, c = e % dp;
        const int gm = min(ct * 16 + r, m - 1);
        const double v = c < d ? cand[(size_t)gm * d + c] / ls[c] : 0.0;
        cs[r * kCsLd + c] = v;
        if (J == 0) cs_out[(size_t)(ct * 16 + r) * dp + c] = v;
    }
    __syncthreads();

    f64x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = {0.0, 0.0, 0.0, 0.0};
    double mu_acc = 0.0;

    for (int p = 0; p <= J; ++p) {
        const int i0 = p * kPanel;
        {   // K* panel: thread = (query point r, observation slot), 16 observations each
            const int r = tid & 15;
            for (int u = 0; u < 16; ++u) {
                const int il = (tid >> 4) + 16 * u;
                const int obs = i0 + il;
                double v = 0.0;
                if (obs < n) {
                    double r2 = 0.0;
                    for (int c = 0; c < dp; ++c) {
                        const double t = cs[r * kCsLd + c] - xs[(size_t)obs * dp + c];
                        r2 += t * t;
                    }
                    v = matern52(sqrt(r2), amp);
                }
                ks[r * kKsLd + il] = v;
            }
        }
        __syncthreads();
        if (with_mu) {
            const int r = tid >> 4, sub = tid & 15;
            for (int u = 0; u < 16; ++u) {
                const int il = sub + 16 * u;
                if (i0 + il < n) mu_acc = fma(ks[r * kKsLd + il], alpha[i0 + il], mu_acc);
            }
        }
        // wave w: the column tiles j0 = 256 J + 16 (4 w + q); k-steps of this panel up to
        // the tile's last column
        int lim[4], kmax = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j0 = J * kPanel + 16 * (4 * wave + q);
            lim[q] = j0 < np ? min(kPanel, j0 + 16 - i0) / 4 : 0;
            kmax = max(kmax, lim[q]);
        }
        for (int k4 = 0; k4 < kmax; ++k4) {
            const int kk = 4 * k4 + (lane >> 4);
            const double av = ks[(lane & 15) * kKsLd + kk];
            const int i = i0 + kk;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (k4 < lim[q]) {
                    const int j = J * kPanel + 16 * (4 * wave + q) + (lane & 15);
                    const double bv = (j < n && i <= j) ? W[(size_t)j * n + i] : 0.0;
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j0 = J * kPanel + 16 * (4 * wave + q);
        if (j0 >= np) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            V[(size_t)(ct * 16 + (lane >> 4) + 4 * e) * np + j0 + (lane & 15)] = acc[q][e];
    }
    if (with_mu) {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) mu_acc += __shfl_xor(mu_acc, off);
        if ((tid & 15) == 0) mu_n[ct * 16 + (tid >> 4)] = mu_acc;
    }
}

// One wave per lower 16 x 16 tile (I >= J) of
//   out = scale (amp Matern52(|c_I - c_J|) - V_I V_J^T + diag_add I),   K run = np,
// written with its mirror.  Rows / columns in [m, rows) are identity padding (rows = m: the
// public covariance; rows = mp: the matrix the factorisation takes).  The diagonal tiles
// also write mu = y_mean + y_std mu_n when asked.
__global__ __launch_bounds__(256) void joint_cov_kernel(const double* __restrict__ V, const double* __restrict__ cs,
                                                        const double* __restrict__ mu_n, int m, int rows, int dp,
                                                        int np, double amp, double scale, double diag_add,
                                                        double y_mean, double y_std, double* __restrict__ out,
                                                        int ld, double* __restrict__ mu_out) {
    const int lane = threadIdx.x & 63;
    const int T = (rows + 15) / 16;
    const int ntl = T * (T + 1) / 2;
    const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nw = gridDim.x * 4;
    for (int t = gw; t < ntl; t += nw) {
        int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (I * (I + 1) / 2 > t) --I;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int J = t - I * (I + 1) / 2;
        const double* va = V + (size_t)(16 * I + (lane & 15)) * np + (lane >> 4);
        const double* vb = V + (size_t)(16 * J + (lane & 15)) * np + (lane >> 4);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < np; k += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va[k], vb[k], acc, 0, 0, 0);
        const int gj = 16 * J + (lane & 15);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = 16 * I + (lane >> 4) + 4 * q;
            if (gi >= rows || gj >= rows) continue;
            double v;
            if (gi < m && gj < m) {
                double r2 = 0.0;
                for (int c = 0; c < dp; ++c) {
                    const double u = cs[(size_t)gi * dp + c] - cs[(size_t)gj * dp + c];
                    r2 += u * u;
                }
                v = matern52(sqrt(r2), amp) - acc[q];
                if (gi == gj) v += diag_add;
                v *= scale;
            } else {
                v = gi == gj ? 1.0 : 0.0;
            }
            out[(size_t)gi * ld + gj] = v;
            if (I != J) out[(size_t)gj * ld + gi] = v;
        }
        if (I == J && mu_out && lane < 16 && 16 * I + lane < m)
            mu_out[16 * I + lane] = y_mean + y_std * mu_n[16 * I + lane];
    }
}

// Workgroup (bx, by): rows i in [64 bx, 64 bx + 64) (one 16-row tile per wave), draws
// r in [16 by, 16 by + 16).  S[r][i] = mu[i] + y_std sum_{j <= i} Lc[i][j] Z[j][r]: the
// lower-triangular k-steps only (the upper triangle of Lc's diagonal blocks still holds
// the covariance and is masked).  Then (min, lowest index) of every draw over the
// workgroup's rows: in-lane over q, a fixed butterfly over lane >> 4, the four waves in
// order through the LDS.  No atomics.
__global__ __launch_bounds__(256) void joint_sample_kernel(const double* __restrict__ Lc, int mp, int m,
                                                           const double* __restrict__ Z, int s,
                                                           const double* __restrict__ mu_n, double y_mean,
                                                           double y_std, double* __restrict__ samples,
                                                           double* __restrict__ part_val,
                                                           long long* __restrict__ part_idx) {
    __shared__ double rv[4][16];
    __shared__ long long ri[4][16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i0 = 16 * (4 * blockIdx.x + wave);
    const int r = 16 * blockIdx.y + (lane & 15);
    double bv = INFINITY;
    long long bi = 0x7fffffffffffffffLL;
    if (i0 < mp) {
        const int irow = i0 + (lane & 15);
        const double* lrow = Lc + (size_t)irow * mp;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < i0 + 16; k += 4) {
            const int j = k + (lane >> 4);
            const double a = j <= irow ? lrow[j] : 0.0;
            const double b = (j < m && r < s) ? Z[(size_t)j * s + r] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + (lane >> 4) + 4 * q;
            if (i < m && r < s) {
                const double v = (y_mean + y_std * mu_n[i]) + y_std * acc[q];
                if (samples) samples[(size_t)r * m + i] = v;
                if (lex_less(v, i, bv, bi)) { bv = v; bi = i; }
            }
        }
    }
    if (!part_val) return;
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const double ov = __shfl_xor(bv, off);
        const long long oi = __shfl_xor(bi, off);
        if (lex_less(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane < 16) { rv[wave][lane] = bv; ri[wave][lane] = bi; }
    __syncthreads();
    if (threadIdx.x < 16 && r < s) {
        for (int w = 1; w < 4; ++w)
            if (lex_less(rv[w][lane], ri[w][lane], bv, bi)) { bv = rv[w][lane]; bi = ri[w][lane]; }
        part_val[(size_t)r * gridDim.x + blockIdx.x] = bv;
        part_idx[(size_t)r * gridDim.x + blockIdx.x] = bi;
    }
}

struct JointWs {
    double* V;        // [mp][np]
    double* mu_n;     // [mp]
    double* cs;       // [mp][dp]
    double* A;        // [mp][mp]   (s > 0)
    double* Dinv;     // [mp][32]
    double* part_val; // [s][nb]
    long long* part_idx;
    size_t used;
};

inline int joint_mp(int m) { return (m + 31) / 32 * 32; }
inline int joint_nb(int m) { return (joint_mp(m) + 63) / 64; }

JointWs carve_joint_ws(void* ws, int np, int dp, int m, int s) {
    mpo::WsCarver c(ws);
    const size_t mp = joint_mp(m);
    JointWs w{};
    w.V = c.take<double>(mp * np);
    w.mu_n = c.take<double>(mp);
    w.cs = c.take<double>(mp * dp);
    if (s > 0) {
        w.A = c.take<double>(mp * mp);
        w.Dinv = c.take<double>(mp * 32);
        w.part_val = c.take<double>((size_t)s * joint_nb(m));
        w.part_idx = c.take<long long>((size_t)s * joint_nb(m));
    }
    w.used = c.used;
    return w;
}

// the shape fields (all the workspace query reads), and the pointers the kernels follow
bool shape_ok(const MpoGpModel* md) {
    return md->n > 0 && md->d > 0 && md->d <= md->dp && md->dp <= 32 && md->dp % 4 == 0 &&
           md->np16 == (md->n + 15) / 16 * 16;
}
bool model_ok(const MpoGpModel* md) { return shape_ok(md) && md->xs && md->ls && md->alpha && md->W; }

// Host checks shared by the two entry points: MPO_OK, or the status with the message set.
int joint_check(const char* who, const MpoGpModel* model, const void* cand, int m) {
    MPO_CHECK_ARG(model && cand, "%s: null model/candidates", who);
    MPO_CHECK_ARG(m >= 1, "%s: m=%d must be >= 1", who, m);
    MPO_CHECK_ARG(model_ok(model), "%s: malformed model n=%d d=%d dp=%d np16=%d", who, model->n, model->d, model->dp,
                  model->np16);
    if (model->n > mpo::kMaxObs || m > MPO_JOINT_MAX) {
        mpo::set_error("%s: n=%d m=%d outside the supported n <= %d, m <= %d", who, model->n, m, mpo::kMaxObs,
                       MPO_JOINT_MAX);
        return MPO_ENOTSUP;
    }
    return MPO_OK;
}

int launch_v(const MpoGpModel* md, const double* cand, int m, const JointWs& w, hipStream_t s) {
    const int mp = joint_mp(m), np = md->np16;
    hipLaunchKernelGGL(joint_v_kernel, dim3(mp / 16, (np + kPanel - 1) / kPanel), dim3(256), 0, s, cand, m, md->d,
                       md->dp, md->ls, md->xs, md->alpha, md->W, md->n, np, md->amp, w.V, w.mu_n, w.cs);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

int launch_cov(const MpoGpModel* md, int m, int rows, const JointWs& w, double scale, double diag_add, double* out,
               int ld, double* mu_out, hipStream_t s) {
    const int T = (rows + 15) / 16, ntl = T * (T + 1) / 2;
    hipLaunchKernelGGL(joint_cov_kernel, dim3(std::max(1, std::min(2048, (ntl + 3) / 4))), dim3(256), 0, s, w.V, w.cs,
                       w.mu_n, m, rows, md->dp, md->np16, md->amp, scale, diag_add, md->y_mean, md->y_std, out, ld,
                       mu_out);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

}  // namespace

extern "C" {

size_t mpo_gp_joint_ws_bytes(const MpoGpModel* model, int m, int s) {
    if (!model || m < 1 || m > MPO_JOINT_MAX || s < 0 || s > MPO_JOINT_SMAX || !shape_ok(model) ||
        model->n > mpo::kMaxObs)
        return 0;
    return carve_joint_ws(nullptr, model->np16, model->dp, m, s).used + 256;
}

int mpo_gp_posterior_cov(const MpoGpModel* model, const double* cand, int m, double* mu, double* cov, int ldc,
                         void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_posterior_cov";
    if (const int rc = joint_check(who, model, cand, m)) return rc;
    MPO_CHECK_ARG(cov && ws, "%s: null cov/workspace", who);
    MPO_CHECK_ARG(ldc >= m, "%s: ldc=%d < m=%d", who, ldc, m);
    const size_t need = mpo_gp_joint_ws_bytes(model, m, 0);
    MPO_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const JointWs w = carve_joint_ws(ws, model->np16, model->dp, m, 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = launch_v(model, cand, m, w, st)) return rc;
    return launch_cov(model, m, m, w, model->y_std * model->y_std, 0.0, cov, ldc, mu, st);
    MPO_GUARD_END
}

int mpo_gp_sample(const MpoGpModel* model, const double* cand, int m, const double* z, int s, double jitter,
                  double* samples, int64_t* argmin, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_sample";
    if (const int rc = joint_check(who, model, cand, m)) return rc;
    MPO_CHECK_ARG(z && info && ws, "%s: null z/info/workspace", who);
    MPO_CHECK_ARG(s >= 1, "%s: s=%d must be >= 1", who, s);
    if (s > MPO_JOINT_SMAX) {   // joint_sample_kernel's grid y is ceil(s / 16) <= 65535
        mpo::set_error("%s: s=%d outside the supported s <= %d", who, s, MPO_JOINT_SMAX);
        return MPO_ENOTSUP;
    }
    MPO_CHECK_ARG(jitter >= 0.0 && std::isfinite(jitter), "%s: jitter must be finite and >= 0", who);
    const size_t need = mpo_gp_joint_ws_bytes(model, m, s);
    MPO_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const JointWs w = carve_joint_ws(ws, model->np16, model->dp, m, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int mp = joint_mp(m), nb = joint_nb(m);
    if (const int rc = launch_v(model, cand, m, w, st)) return rc;
    if (const int rc = launch_cov(model, m, mp, w, 1.0, jitter * model->amp, w.A, mp, nullptr, st)) return rc;
    MPO_HIP(mpo::blocked_chol(w.A, mp, w.Dinv, info, st));
    if (!samples && !argmin) return MPO_OK;
    hipLaunchKernelGGL(joint_sample_kernel, dim3(nb, (s + 15) / 16), dim3(256), 0, st, w.A, mp, m, z, s, w.mu_n,
                       model->y_mean, model->y_std, samples, argmin ? w.part_val : nullptr, w.part_idx);
    MPO_LAUNCH_CHECK();
    if (argmin)
        MPO_HIP(mpo::argmin_fold(w.part_val, w.part_idx, s, nb, reinterpret_cast<long long*>(argmin), nullptr, st));
    return MPO_OK;
    MPO_GUARD_END
}

}  // extern "C"
