// gp_paths.hip -- pathwise posterior samples of a prepared GP (gfx950, fp64
// v_mfma_f64_16x16x4): Matheron's rule with a random-Fourier-feature prior (Wilson et al.
// 2020, "Efficiently sampling functions from Gaussian process posteriors").  A draw is a
// function; s draws at m points are one GEMM [m x (Fp + np16)] . [(Fp + np16) x s] whose A
// operand is computed on the fly (mpo_gp_paths_prepare, mpo_gp_paths_eval).
// No m x m matrix, no factorisation, no jitter, no cap on m.
//
// With c = x / ls, phi_j(x) = cos(omega_j . c + phase_j), scale = sqrt(2 amp / F):
//   paths_pack_kernel    omega [Fp][dp], phase [Fp] zero-padded
//   paths_phi_kernel     Phi(X) [n][F] from the model's xs
//   paths_resid_kernel   resid = scale Phi w + sqrt(noise + 1e-10) eps           [n][s]
//   paths_wt_kernel      t = W resid (lower triangle)                            [n][s]
//   paths_coef_kernel    coef = [scale w ; 0 ; alpha - W^T t ; 0]                [Kp][sp]
//   paths_eval_kernel    f_r(x) = y_mean + y_std (A(x) coef[:, r]),  A = [phi | amp Matern52(|c - xs|)],
//                        the optional sample rows and the per-workgroup (min, index) of every draw
//   argmin_fold_kernel   the workgroups' partials of a draw folded in order (mpo::argmin_fold)
//   paths_grad_kernel    f_r(x) and its gradient at one point per workgroup (mpo_gp_paths_grad: the
//                        objective of a continuous minimisation of a draw; no MFMA, latency-bound)
// Fp = F rounded up to 16, Kp = Fp + np16 rounded up to 64 (the K panel), sp = s rounded up
// to 16, plus 16 (a draw tile that starts at any first_draw stays inside the row).  Only the
// plain W, xs, alpha and ls of the model are read, never wfrag: the same kernels serve a
// resident, a streamed, an appended and a from_factor model.  Every sum runs in a fixed
// order that depends on (F, n) alone: the value of a candidate under a draw is the same
// bits whatever m, the grid, the rows around it or the draw range of the call.
//
// f64 16x16x4 operands: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 q.
#include "mpo_internal.h"
#include "gp_acq_math.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

using mpo::lex_less;   // gp_acq_math.h
using mpo::matern52;   // the Matern of bc_kmat_kernel (mpo_internal.h)

constexpr int kTileM = 64;            // candidates per tile: four 16-row MFMA tiles
constexpr int kPanelK = 64;           // columns of A per LDS panel: 16 k-steps
constexpr int kChunkS = 256;          // draws per workgroup: 16 draw tiles, wave w owns w, w + 4, ..
constexpr int kStLd = 65;             // LDS row stride of a wave's 16 draws x 64 rows staging area
constexpr int kCsLd = 33;            // LDS row stride of the scaled candidate tile (dp <= 32)
constexpr int kGridCap = 512;         // resident workgroups: 256 CUs x 2 (launch bounds)

inline int round_up(int x, int a) { return (x + a - 1) / a * a; }
inline int paths_fp(int F) { return round_up(F, 16); }
inline int paths_kp(int F, int np16) { return round_up(paths_fp(F) + np16, kPanelK); }
inline int paths_sp(int s) { return round_up(s, 16) + 16; }

// ---- prepare ---------------------------------------------------------------------------

__global__ void paths_pack_kernel(const double* __restrict__ omega, const double* __restrict__ phase, int F, int Fp,
                                  int d, int dp, double* __restrict__ om_p, double* __restrict__ ph_p) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Fp * dp) return;
    const int j = e / dp, c = e % dp;
    om_p[e] = (j < F && c < d) ? omega[(size_t)j * d + c] : 0.0;
    if (c == 0) ph_p[j] = j < F ? phase[j] : 0.0;
}

// Phi[i][j] = cos(omega_j . xs_i + phase_j): the argument summed over the dimensions in order
__global__ void paths_phi_kernel(const double* __restrict__ xs, const double* __restrict__ om_p,
                                 const double* __restrict__ ph_p, int n, int F, int dp, double* __restrict__ Phi) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= F || i >= n) return;
    double a = ph_p[j];
    for (int c = 0; c < dp; ++c) a = fma(om_p[(size_t)j * dp + c], xs[(size_t)i * dp + c], a);
    Phi[(size_t)i * F + j] = cos(a);
}

// resid[i][r] = scale sum_j Phi[i][j] w[j][r] + sig eps[i][r], j in order
__global__ void paths_resid_kernel(const double* __restrict__ Phi, const double* __restrict__ w,
                                   const double* __restrict__ eps, int n, int F, int s, double scale, double sig,
                                   double* __restrict__ resid) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (r >= s || i >= n) return;
    const double* p = Phi + (size_t)i * F;
    double acc = 0.0;
    for (int j = 0; j < F; ++j) acc = fma(p[j], w[(size_t)j * s + r], acc);
    resid[(size_t)i * s + r] = fma(scale, acc, sig * eps[(size_t)i * s + r]);
}

// t[i][r] = sum_{k <= i} W[i][k] resid[k][r], k in order
__global__ void paths_wt_kernel(const double* __restrict__ W, const double* __restrict__ resid, int n, int s,
                                double* __restrict__ t) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (r >= s || i >= n) return;
    const double* wr = W + (size_t)i * n;
    double acc = 0.0;
    for (int k = 0; k <= i; ++k) acc = fma(wr[k], resid[(size_t)k * s + r], acc);
    t[(size_t)i * s + r] = acc;
}

// coef rows [0, F): scale w; rows [Fp, Fp + n): alpha[i] - sum_{k >= i} W[k][i] t[k][r], k in
// order.  The padding rows and columns were zeroed before (hipMemsetAsync).
__global__ void paths_coef_kernel(const double* __restrict__ W, const double* __restrict__ alpha,
                                  const double* __restrict__ t, const double* __restrict__ w, int n, int F, int Fp,
                                  int s, int sp, double scale, double* __restrict__ coef) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (r >= s) return;
    if (row < F) {
        coef[(size_t)row * sp + r] = scale * w[(size_t)row * s + r];
        return;
    }
    const int i = row - F;
    if (i >= n) return;
    double acc = 0.0;
    for (int k = i; k < n; ++k) acc = fma(W[(size_t)k * n + i], t[(size_t)k * s + r], acc);
    coef[(size_t)(Fp + i) * sp + r] = alpha[i] - acc;
}

// ---- eval --------------------------------------------------------------------------------

// Workgroup (bx, by): the candidate tiles bx, bx + gridDim.x, .. of 64 rows, the draws
// first + 256 by .. of the call (16-draw tiles; wave w owns tiles w, w + 4, w + 8, w + 12 and
// all 64 rows of each).  Per candidate tile the A operand is built ONCE, panel by panel
// (64 columns) into the LDS in A-fragment order -- thread (row = tid & 63, wave): the 16
// columns 16 wave .. of the panel, all features (cosines) or all observations (Matern by
// direct differences), since Fp is a multiple of 16 -- and multiplied into every draw tile
// of the workgroup; the coefficients stream from L2.  Then y_mean + y_std (.), the optional
// sample rows staged through the LDS so that a store runs along m, and the running
// (min, lowest index) of every draw: in-lane over the rows and tiles, a fixed butterfly over
// lane >> 4 at the end.  A wave owns all rows of its draws, so no fold across waves.
// Rows >= m of the last tile repeat row m - 1 and are neither stored nor folded.
__global__ __launch_bounds__(256, 2) void paths_eval_kernel(
    const double* __restrict__ cand, long long m, int d, int dp, const double* __restrict__ ls,
    const double* __restrict__ xs, int n, double amp, const double* __restrict__ om_p, const double* __restrict__ ph_p,
    int Fp, int Kp, const double* __restrict__ coef, int sp, int first, int n_draws, double y_mean, double y_std,
    double* __restrict__ samples, double* __restrict__ part_val, long long* __restrict__ part_idx, long long n_tiles) {
    __shared__ double as[4 * 16 * kStLd];     // A panel in fragment order (4096); the sample staging area
    __shared__ double cs[kTileM * kCsLd];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int d0 = kChunkS * blockIdx.y;                       // first draw of the workgroup, in the call
    const int ndt = (min(n_draws - d0, kChunkS) + 15) / 16;    // its draw tiles
    const double* bbase = coef + first + d0 + (lane & 15);

    double bv[4];
    long long bi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { bv[q] = INFINITY; bi[q] = 0x7fffffffffffffffLL; }

    for (long long ct = blockIdx.x; ct < n_tiles; ct += gridDim.x) {
        const long long row0 = ct * kTileM;
        __syncthreads();   // the previous tile's readers of cs / as are done
        for (int e = tid; e < kTileM * dp; e += 256) {
            const int r = e / dp, c = e % dp;
            const long long gm = min(row0 + r, m - 1);
            cs[r * kCsLd + c] = c < d ? cand[(size_t)gm * d + c] / ls[c] : 0.0;
        }
        __syncthreads();

        f64x4 acc[4][4];   // [row tile][draw tile slot]
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = {0.0, 0.0, 0.0, 0.0};

        for (int k0 = 0; k0 < Kp; k0 += kPanelK) {
            {   // the panel: row = lane, columns k0 + 16 wave + u
                const double* crow = cs + lane * kCsLd;
                const int cbase = k0 + 16 * wave;
                double* dst = as + ((lane >> 4) * 16 + 4 * wave) * 64 + (lane & 15);
                if (cbase < Fp) {
                    for (int u = 0; u < 16; ++u) {
                        const int j = cbase + u;
                        double a = ph_p[j];
                        for (int c = 0; c < dp; ++c) a = fma(om_p[(size_t)j * dp + c], crow[c], a);
                        dst[(u >> 2) * 64 + (u & 3) * 16] = cos(a);
                    }
                } else {
                    for (int u = 0; u < 16; ++u) {
                        const int obs = cbase - Fp + u;
                        double v = 0.0;
                        if (obs < n) {
                            double r2 = 0.0;
                            for (int c = 0; c < dp; ++c) {
                                const double tt = crow[c] - xs[(size_t)obs * dp + c];
                                r2 += tt * tt;
                            }
                            v = matern52(sqrt(r2), amp);
                        }
                        dst[(u >> 2) * 64 + (u & 3) * 16] = v;
                    }
                }
            }
            __syncthreads();
            for (int j = 0; j < kPanelK / 4; ++j) {
                const double* brow = bbase + (size_t)(k0 + 4 * j + (lane >> 4)) * sp;
                double b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = (wave + 4 * q < ndt) ? brow[16 * (wave + 4 * q)] : 0.0;
                double a[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] = as[(t * 16 + j) * 64 + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (wave + 4 * q < ndt) {
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[q], acc[t][q], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }

        // finish, fold, and store: draw r = first + d0 + 16 (wave + 4 q) + (lane & 15), out row
        // r - first; candidate row0 + 16 t + (lane >> 4) + 4 e
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int dr = d0 + 16 * (wave + 4 * q) + (lane & 15);   // draw within the call
            const bool live = wave + 4 * q < ndt && dr < n_draws;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double v = y_mean + y_std * acc[t][q][e];
                    acc[t][q][e] = v;
                    const long long i = row0 + 16 * t + (lane >> 4) + 4 * e;
                    if (live && i < m && lex_less(v, i, bv[q], bi[q])) { bv[q] = v; bi[q] = i; }
                }
        }
        if (samples) {
            // wave-private 16 draws x 64 rows staging area; every wave walks the four slots, so
            // the barriers are uniform
            double* st = as + wave * 16 * kStLd;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __syncthreads();
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) st[(lane & 15) * kStLd + 16 * t + (lane >> 4) + 4 * e] = acc[t][q][e];
                __syncthreads();
                if (wave + 4 * q < ndt) {
                    const long long i = row0 + lane;
                    for (int c = 0; c < 16; ++c) {
                        const int dr = d0 + 16 * (wave + 4 * q) + c;
                        if (dr < n_draws && i < m) samples[(size_t)dr * m + i] = st[c * kStLd + lane];
                    }
                }
            }
        }
    }

    if (!part_val) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const double ov = __shfl_xor(bv[q], off);
            const long long oi = __shfl_xor(bi[q], off);
            if (lex_less(ov, oi, bv[q], bi[q])) { bv[q] = ov; bi[q] = oi; }
        }
        const int dr = d0 + 16 * (wave + 4 * q) + lane;
        if (lane < 16 && wave + 4 * q < ndt && dr < n_draws) {
            part_val[(size_t)dr * gridDim.x + blockIdx.x] = bv[q];
            part_idx[(size_t)dr * gridDim.x + blockIdx.x] = bi[q];
        }
    }
}

// argmin[r] / minval[r]: the draw's nb workgroup partials folded in order (ties to the lowest index)
__global__ void argmin_fold_kernel(const double* __restrict__ part_val, const long long* __restrict__ part_idx,
                                    int n_draws, int nb, long long* __restrict__ argmin, double* __restrict__ minval) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_draws) return;
    double bv = part_val[(size_t)r * nb];
    long long bi = part_idx[(size_t)r * nb];
    for (int b = 1; b < nb; ++b) {
        const double v = part_val[(size_t)r * nb + b];
        const long long i = part_idx[(size_t)r * nb + b];
        if (lex_less(v, i, bv, bi)) { bv = v; bi = i; }
    }
    if (argmin) argmin[r] = bi;
    if (minval) minval[r] = bv;
}

// ---- value and gradient at a point ---------------------------------------------------------

// Workgroup b: f and g of draw[b] at x[b].  The Fp + n terms (features, then observations)
// go to thread tid, tid + 256, ..; a thread adds its terms' shares of f and of the gradient
// IN THE SCALED SPACE (d / dc) into registers, DP a template parameter so that no private
// array is indexed at run time.  The partials fold through a fixed butterfly in the wave,
// then the four waves in order through the LDS; y_std and 1 / ls come once, at the end.
// The order depends on (Fp, n) alone: a run's f and g are the same bits in any batch.
//   feature j      a = omega_j . c + phase_j (the sum of paths_phi_kernel):
//                  f += cos(a) coef_j,  dc += -sin(a) coef_j omega_j
//   observation i  D = c - xs_i, k = sqrt(5) |D|:
//                  f += amp (1 + k + k^2/3) e^-k coef_i,  dc += -amp (5/3)(1 + k) e^-k coef_i D
// (dMatern/dr) / r has no division by r: an observation at the point itself adds exactly 0.
// A draw outside [0, s) gives NaN and reads nothing.
template <int DP>
__global__ __launch_bounds__(256) void paths_grad_kernel(
    const double* __restrict__ x, const int32_t* __restrict__ draw, int d, const double* __restrict__ ls,
    const double* __restrict__ xs, int n, double amp, const double* __restrict__ om_p, const double* __restrict__ ph_p,
    int Fp, const double* __restrict__ coef, int sp, int s, double y_mean, double y_std, double* __restrict__ f,
    double* __restrict__ g) {
    __shared__ double cs[DP];
    __shared__ double part[4][DP + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int r = draw[b];
    if (r < 0 || r >= s) {   // uniform over the workgroup
        if (tid == 0) f[b] = NAN;
        if (tid < d) g[(size_t)b * d + tid] = NAN;
        return;
    }
    if (tid < DP) cs[tid] = tid < d ? x[(size_t)b * d + tid] / ls[tid] : 0.0;
    __syncthreads();

    double af = 0.0, ag[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) ag[c] = 0.0;
    const double* cf = coef + r;
    const int terms = Fp + n;
    for (int t = tid; t < terms; t += 256) {
        if (t < Fp) {
            const double* om = om_p + (size_t)t * DP;
            double w[DP];
            double a = ph_p[t];
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                w[c] = om[c];
                a = fma(w[c], cs[c], a);
            }
            const double cj = cf[(size_t)t * sp];
            af = fma(cos(a), cj, af);
            const double sj = -sin(a) * cj;
#pragma unroll
            for (int c = 0; c < DP; ++c) ag[c] = fma(sj, w[c], ag[c]);
        } else {
            const double* xo = xs + (size_t)(t - Fp) * DP;
            double dl[DP];
            double r2 = 0.0;
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                dl[c] = cs[c] - xo[c];
                r2 += dl[c] * dl[c];
            }
            const double rr = sqrt(r2);
            const double ci = cf[(size_t)t * sp];
            af = fma(matern52(rr, amp), ci, af);
            const double k = rr * mpo::kSqrt5;
            const double gi = -(amp * ((5.0 / 3.0) * (1.0 + k) * exp(-k))) * ci;
#pragma unroll
            for (int c = 0; c < DP; ++c) ag[c] = fma(gi, dl[c], ag[c]);
        }
    }

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        af += __shfl_xor(af, off);
#pragma unroll
        for (int c = 0; c < DP; ++c) ag[c] += __shfl_xor(ag[c], off);
    }
    if (lane == 0) {
        part[wave][DP] = af;
#pragma unroll
        for (int c = 0; c < DP; ++c) part[wave][c] = ag[c];
    }
    __syncthreads();
    if (tid <= DP) {
        const double v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        if (tid == DP) f[b] = y_mean + y_std * v;
        else if (tid < d) g[(size_t)b * d + tid] = y_std * v / ls[tid];
    }
}

// ---- host ----------------------------------------------------------------------------------

struct PathsWs {
    double* om_p;    // [Fp][dp]
    double* ph_p;    // [Fp]
    double* coef;    // [Kp][sp]
    double* Phi;     // [n][F]     (prepare only)
    double* resid;   // [n][s]
    double* t;       // [n][s]
    size_t used;
};

PathsWs carve_paths_ws(void* ws, int n, int np16, int dp, int F, int s) {
    mpo::WsCarver c(ws);
    const size_t Fp = paths_fp(F), Kp = paths_kp(F, np16), sp = paths_sp(s);
    PathsWs w{};
    w.om_p = c.take<double>(Fp * dp);
    w.ph_p = c.take<double>(Fp);
    w.coef = c.take<double>(Kp * sp);
    w.Phi = c.take<double>((size_t)n * F);
    w.resid = c.take<double>((size_t)n * s);
    w.t = c.take<double>((size_t)n * s);
    w.used = c.used;
    return w;
}

// the shape fields (all the workspace queries read), and the pointers the kernels follow
bool shape_ok(const MpoGpModel* md) {
    return md->n > 0 && md->d > 0 && md->d <= md->dp && md->dp <= 32 && md->dp % 4 == 0 &&
           md->np16 == (md->n + 15) / 16 * 16;
}
bool model_ok(const MpoGpModel* md) { return shape_ok(md) && md->xs && md->ls && md->alpha && md->W; }

bool paths_shape_ok(const MpoGpPaths* p) {
    return p->F >= 1 && p->F <= MPO_PATHS_FMAX && p->s >= 1 && p->s <= MPO_PATHS_SMAX && p->n >= 1 &&
           p->n <= mpo::kMaxObs && p->Fp == paths_fp(p->F) && p->Kp == paths_kp(p->F, (p->n + 15) / 16 * 16) &&
           p->sp == paths_sp(p->s);
}
bool paths_ok(const MpoGpPaths* p, const MpoGpModel* md) {
    return paths_shape_ok(p) && p->n == md->n && p->dp == md->dp && p->omega && p->phase && p->coef;
}

// the candidate tiles of m rows and the workgroups that walk them (MPO_PATHS_GRID lowers the
// cap: a test knob, as MPO_GP_PANEL is for the streamed scoring kernel)
inline long long eval_tiles(int64_t m) { return (m + kTileM - 1) / kTileM; }
inline int eval_chunks(int n_draws) { return (n_draws + kChunkS - 1) / kChunkS; }
int eval_grid_x(int64_t m, int n_draws) {
    int cap = std::max(1, kGridCap / eval_chunks(n_draws));
    if (const char* e = std::getenv("MPO_PATHS_GRID")) {
        const int v = std::atoi(e);
        if (v >= 1 && v < cap) cap = v;
    }
    return (int)std::min<long long>(eval_tiles(m), cap);
}
// sized for the uncapped grid, whatever the knob says
inline size_t eval_parts(int64_t m, int n_draws) {
    return (size_t)n_draws * (size_t)std::min<long long>(eval_tiles(m), kGridCap);
}

// the instance of a model's padded width (the widths of the scoring kernels); null otherwise
using GradKernel = decltype(&paths_grad_kernel<4>);
GradKernel pick_grad_kernel(int dp) {
    switch (dp) {
        case 4: return paths_grad_kernel<4>;
        case 8: return paths_grad_kernel<8>;
        case 12: return paths_grad_kernel<12>;
        case 16: return paths_grad_kernel<16>;
        case 32: return paths_grad_kernel<32>;
        default: return nullptr;
    }
}

}  // namespace

hipError_t mpo::argmin_fold(const double* part_val, const long long* part_idx, int n_draws, int nb, long long* argmin,
                            double* minval, hipStream_t s) {
    hipLaunchKernelGGL(argmin_fold_kernel, dim3((n_draws + 255) / 256), dim3(256), 0, s, part_val, part_idx, n_draws, nb,
                       argmin, minval);
    return hipGetLastError();
}

extern "C" {

size_t mpo_gp_paths_ws_bytes(const MpoGpModel* model, int F, int s) {
    if (!model || !shape_ok(model) || model->n > mpo::kMaxObs || F < 1 || F > MPO_PATHS_FMAX || s < 1 ||
        s > MPO_PATHS_SMAX)
        return 0;
    return carve_paths_ws(nullptr, model->n, model->np16, model->dp, F, s).used + 256;
}

int mpo_gp_paths_prepare(const MpoGpModel* model, double noise, const double* omega, const double* phase,
                         const double* w, const double* eps, int F, int s, MpoGpPaths* paths, void* ws,
                         size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_paths_prepare";
    MPO_CHECK_ARG(model && omega && phase && w && eps && paths && ws, "%s: null argument", who);
    MPO_CHECK_ARG(F >= 1 && s >= 1, "%s: F=%d s=%d must be >= 1", who, F, s);
    MPO_CHECK_ARG(model_ok(model), "%s: malformed model n=%d d=%d dp=%d np16=%d", who, model->n, model->d, model->dp,
                  model->np16);
    MPO_CHECK_ARG(noise >= 0.0 && std::isfinite(noise), "%s: noise must be finite and >= 0", who);
    if (model->n > mpo::kMaxObs || F > MPO_PATHS_FMAX || s > MPO_PATHS_SMAX) {
        mpo::set_error("%s: n=%d F=%d s=%d outside the supported n <= %d, F <= %d, s <= %d", who, model->n, F, s,
                       mpo::kMaxObs, MPO_PATHS_FMAX, MPO_PATHS_SMAX);
        return MPO_ENOTSUP;
    }
    const size_t need = mpo_gp_paths_ws_bytes(model, F, s);
    MPO_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    const int n = model->n, dp = model->dp, Fp = paths_fp(F), Kp = paths_kp(F, model->np16), sp = paths_sp(s);
    const PathsWs pw = carve_paths_ws(ws, n, model->np16, dp, F, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double scale = std::sqrt(2.0 * model->amp / F), sig = std::sqrt(noise + 1e-10);

    MPO_HIP(hipMemsetAsync(pw.coef, 0, (size_t)Kp * sp * sizeof(double), st));
    hipLaunchKernelGGL(paths_pack_kernel, dim3((Fp * dp + 255) / 256), dim3(256), 0, st, omega, phase, F, Fp,
                       model->d, dp, pw.om_p, pw.ph_p);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_phi_kernel, dim3((F + 255) / 256, n), dim3(256), 0, st, model->xs, pw.om_p, pw.ph_p, n, F,
                       dp, pw.Phi);
    MPO_LAUNCH_CHECK();
    const dim3 gs((s + 63) / 64, n);
    hipLaunchKernelGGL(paths_resid_kernel, gs, dim3(64), 0, st, pw.Phi, w, eps, n, F, s, scale, sig, pw.resid);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_wt_kernel, gs, dim3(64), 0, st, model->W, pw.resid, n, s, pw.t);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(paths_coef_kernel, dim3((s + 63) / 64, F + n), dim3(64), 0, st, model->W, model->alpha, pw.t, w,
                       n, F, Fp, s, sp, scale, pw.coef);
    MPO_LAUNCH_CHECK();

    paths->F = F;
    paths->s = s;
    paths->n = n;
    paths->dp = dp;
    paths->Fp = Fp;
    paths->Kp = Kp;
    paths->sp = sp;
    paths->reserved = 0;
    paths->omega = pw.om_p;
    paths->phase = pw.ph_p;
    paths->coef = pw.coef;
    return MPO_OK;
    MPO_GUARD_END
}

size_t mpo_gp_paths_eval_ws_bytes(const MpoGpModel* model, const MpoGpPaths* paths, int64_t m, int n_draws) {
    if (!model || !paths || !shape_ok(model) || model->n > mpo::kMaxObs || !paths_shape_ok(paths) ||
        paths->n != model->n || paths->dp != model->dp || m < 1 || n_draws < 1 || n_draws > paths->s)
        return 0;
    mpo::WsCarver c(nullptr);
    c.take<double>(eval_parts(m, n_draws));
    c.take<long long>(eval_parts(m, n_draws));
    return c.used + 256;
}

int mpo_gp_paths_eval(const MpoGpModel* model, const MpoGpPaths* paths, const double* cand, int64_t m, int first_draw,
                      int n_draws, double* samples, int64_t* argmin, double* minval, void* ws, size_t ws_bytes,
                      void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_paths_eval";
    MPO_CHECK_ARG(model && paths && cand && ws, "%s: null model/paths/candidates/workspace", who);
    MPO_CHECK_ARG(m >= 1, "%s: m=%lld must be >= 1", who, (long long)m);
    MPO_CHECK_ARG(model_ok(model), "%s: malformed model n=%d d=%d dp=%d np16=%d", who, model->n, model->d, model->dp,
                  model->np16);
    if (model->n > mpo::kMaxObs || paths->F > MPO_PATHS_FMAX || paths->s > MPO_PATHS_SMAX) {
        mpo::set_error("%s: n=%d F=%d s=%d outside the supported n <= %d, F <= %d, s <= %d", who, model->n, paths->F,
                       paths->s, mpo::kMaxObs, MPO_PATHS_FMAX, MPO_PATHS_SMAX);
        return MPO_ENOTSUP;
    }
    MPO_CHECK_ARG(paths_ok(paths, model), "%s: malformed paths F=%d s=%d n=%d dp=%d Fp=%d Kp=%d sp=%d", who, paths->F,
                  paths->s, paths->n, paths->dp, paths->Fp, paths->Kp, paths->sp);
    MPO_CHECK_ARG(first_draw >= 0 && n_draws >= 1 && n_draws <= paths->s && first_draw <= paths->s - n_draws,
                  "%s: draws [%d, %d + %d) outside [0, %d)", who, first_draw, first_draw, n_draws, paths->s);
    const size_t need = mpo_gp_paths_eval_ws_bytes(model, paths, m, n_draws);
    MPO_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%zu < %zu)", who, ws_bytes, need);
    if (!samples && !argmin && !minval) return MPO_OK;
    mpo::WsCarver c(ws);
    double* part_val = c.take<double>(eval_parts(m, n_draws));
    long long* part_idx = c.take<long long>(eval_parts(m, n_draws));
    const bool fold = argmin || minval;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gx = eval_grid_x(m, n_draws);
    hipLaunchKernelGGL(paths_eval_kernel, dim3(gx, eval_chunks(n_draws)), dim3(256), 0, st, cand, (long long)m,
                       model->d, model->dp, model->ls, model->xs, model->n, model->amp, paths->omega, paths->phase,
                       paths->Fp, paths->Kp, paths->coef, paths->sp, first_draw, n_draws, model->y_mean, model->y_std,
                       samples, fold ? part_val : nullptr, part_idx, eval_tiles(m));
    MPO_LAUNCH_CHECK();
    if (fold) MPO_HIP(mpo::argmin_fold(part_val, part_idx, n_draws, gx, reinterpret_cast<long long*>(argmin), minval, st));
    return MPO_OK;
    MPO_GUARD_END
}

// the checks of mpo_gp_paths_grad and its _host form, all on the host
static int paths_grad_check(const char* who, const MpoGpModel* model, const MpoGpPaths* paths, const void* x,
                            const void* draw, int batch, const void* f, const void* g) {
    MPO_CHECK_ARG(model && paths && x && draw && f && g, "%s: null pointer", who);
    MPO_CHECK_ARG(batch >= 1 && batch <= MPO_PATHS_GRAD_BMAX, "%s: batch=%d outside [1, %d]", who, batch,
                  MPO_PATHS_GRAD_BMAX);
    MPO_CHECK_ARG(model_ok(model) && model->n <= mpo::kMaxObs && pick_grad_kernel(model->dp),
                  "%s: malformed model n=%d d=%d dp=%d np16=%d", who, model->n, model->d, model->dp, model->np16);
    MPO_CHECK_ARG(paths_ok(paths, model), "%s: malformed paths F=%d s=%d n=%d dp=%d Fp=%d Kp=%d sp=%d", who, paths->F,
                  paths->s, paths->n, paths->dp, paths->Fp, paths->Kp, paths->sp);
    return MPO_OK;
}

int mpo_gp_paths_grad(const MpoGpModel* model, const MpoGpPaths* paths, const double* x, const int32_t* draw, int batch,
                      double* f, double* g, void* stream) {
    MPO_GUARD_BEGIN
    if (const int rc = paths_grad_check("mpo_gp_paths_grad", model, paths, x, draw, batch, f, g)) return rc;
    hipLaunchKernelGGL(pick_grad_kernel(model->dp), dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       draw, model->d, model->ls, model->xs, model->n, model->amp, paths->omega, paths->phase,
                       paths->Fp, paths->coef, paths->sp, paths->s, model->y_mean, model->y_std, f, g);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_gp_paths_grad_host(const MpoGpModel* model, const MpoGpPaths* paths, const double* x_host,
                           const int32_t* draw_host, int batch, double* f_host, double* g_host, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_paths_grad_host";
    if (const int rc = paths_grad_check(who, model, paths, x_host, draw_host, batch, f_host, g_host)) return rc;
    return mpo::pinned_round(who, stream, x_host, draw_host, f_host, g_host, nullptr,
                             [&](const double* x, const int32_t* draw, double* f, double* g, double*) -> int {
        for (int b = 0; b < batch; ++b)
            MPO_CHECK_ARG(draw_host[b] >= 0 && draw_host[b] < paths->s, "%s: draw[%d]=%d outside [0, %d)", who, b,
                          draw_host[b], paths->s);
        return mpo_gp_paths_grad(model, paths, x, draw, batch, f, g, stream);
    });
    MPO_GUARD_END
}

}  // extern "C"
