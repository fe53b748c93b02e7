// topclass.hip -- population training of the strided test_cnn ("topclass") on gfx950 (MI355X).
//
// The third population engine: the reference's first example (mpiLAPI.py:178-195, built by
// hyperparameter_search_option3.py:108-114 and base_model.py:21-55), channels-last:
//
//   Conv2D(32, k, strides 3, valid, relu) -> Conv2D(32, k, strides 3, valid, relu)
//   -> MaxPool 2x2 -> Dropout(dropout / 2) -> Flatten -> Dense(128, relu) -> Dropout(dropout)
//   -> Dense(classes, softmax)
//
// Every member is one (trial, fold) pair with its own kernel_size (1..9), dropout, lr, seed
// and loss / optimizer bits; the input shape (H, W, C) and the class count belong to the
// population.  One launch per op covers every member through a host-built item list.
//
// Every contraction of a step is one implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32):
// tc_gemm_kernel<OP> computes a 64 x 32 output tile per workgroup (a wave per 16 rows, two
// accumulators), its A and B fragments gathered straight from global memory by the op's own
// index map -- the strided windows of x / a1 for the forward convolutions and their weight
// gradients, a residue class of a1 pixels for conv2's input gradient -- and zero where the
// map leaves the tensor.  Nothing is staged in LDS and nothing is shared between members:
// an item belongs to one member, every output element has one K order that depends on that
// member's geometry and the batch alone, so a member's bits do not depend on the population
// around it.  What that costs is measured in DESIGN.md (x is re-read by every member).
//
//   conv1 / conv2 forward     M = B Ho Wo pixels, N = 32, K = k k Cin
//   pool_fwd                  a2 -> pd = dropout_0(maxpool), argmax (first maximum, row-major)
//   dense 1 / 2 forward       h = relu(pd w3 + b3), hd = dropout_1(h); z3 = hd w4 + b4
//   loss                      softmax, Keras binary / categorical cross-entropy, dz3
//   dense weight gradients    M = fan_in + 1 (a row of ones gives the bias gradient), K = B
//   dense input gradients     dh = dz3 w4^T mask_1 (h > 0);  dp = dh w3^T mask_0
//   pool_bwd                  dz2 = unpool(dp) (a2 > 0), zero on the rows / columns the pool drops
//   conv2 input gradient      per residue class (iy mod 3, ix mod 3) of a1 pixels: K runs over the
//                             ceil(k/3)^2 taps that can reach the class, so every a1 pixel --
//                             covered by 0, 1 or several windows -- is written on every step
//   conv weight gradients     M = k k Cin + 1, K = B Ho Wo split in chunks of 2048 pixels into
//                             partial slabs, summed in slab order by tc_reduce_kernel
//   adam                      Keras Adam / SGD with the member's lr

#include "mpo_internal.h"
#include "pop_common.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace {

using namespace mpo::pop;   // dropout hash, loss row + fold, update_range, the size / offset queries

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kF = 32;          // filters of both convolutions (mpiLAPI.py:184-185)
constexpr int kD = 128;         // dense units (mpiLAPI.py:190)
constexpr int kMaxClasses = 16;
constexpr int kStride = 3;
constexpr int kWgChunk = 2048;  // pixels per weight-gradient slab (a multiple of 4)
constexpr int kAdamChunk = 4096;
constexpr int kTileM = 64, kTileN = 32;

struct TcMember {
    int k, H1, W1, H2, W2, Hp, Wp, K1;
    float lr, inv0, inv1;       // 1 / (1 - rate) of dropout layer 0 (dropout / 2) and 1 (dropout)
    unsigned thr0, thr1;        // keep iff (hash >> 8) >= thr
    int drop0, drop1;           // 0 < rate < 1 (any other rate is the identity, as Keras 2)
    int loss, opt;
    unsigned seed;
    int s1, s2;                 // weight-gradient slabs of conv1 / conv2
    long long w1, b1, w2, b2, w3, b3, w4, b4, pend;
    long long a1, a2, pd, am, h, hd, z3, dz3, dh, dp, dz2, dz1, slab1, slab2;
};

struct TcItem { int member, m0, n0, aux; };

struct TcArgs {
    const TcMember* mem;
    float* params;
    float* grads;
    float* act;
    const float* x;          // [n_samples][H][W][C]
    const int* labels;
    const int* order;
    long long order_stride, row0;
    int B, H, W, C, classes;
    int step, train;
    float* loss_out;
    float* loss_sum;
    int* correct;
};

enum TcOp { CONV1_FWD = 0, CONV2_FWD, D1_FWD, D2_FWD, D2_WGRAD, D2_DGRAD, D1_WGRAD, D1_DGRAD, CONV2_DGRAD,
            CONV2_WGRAD, CONV1_WGRAD, kNumOps };

// multiplier of dropout `layer` on flat element `elem` of the member's [B, features] tensor
__device__ __forceinline__ float tc_mask(const TcArgs& a, const TcMember& mb, int layer, unsigned elem) {
    if (!a.train || !(layer ? mb.drop1 : mb.drop0)) return 1.f;
    const unsigned base = drop_base(mb.seed, a.step, layer);
    return drop_keep(base, elem, layer ? mb.thr1 : mb.thr0) ? (layer ? mb.inv1 : mb.inv0) : 0.f;
}

// ============================================================================
// One op's index maps: A(m, kk), B(kk, n) and the store of C(m, n).
// ============================================================================
template <int OP>
struct TcGemm {
    const TcArgs& a;
    const TcMember& mb;
    const int member, aux;
    int M, N, K, kbeg, kend;
    int ry, rx, nyc, nxc, J;   // CONV2_DGRAD: the residue class and its pixel grid, taps per axis

    __device__ TcGemm(const TcArgs& a_, const TcMember& mb_, const TcItem& it)
        : a(a_), mb(mb_), member(it.member), aux(it.aux) {
        const int k = mb.k, B = a.B;
        ry = rx = nyc = nxc = J = 0;
        kbeg = 0;
        if constexpr (OP == CONV1_FWD) { M = B * mb.H1 * mb.W1; N = kF; K = k * k * a.C; }
        if constexpr (OP == CONV2_FWD) { M = B * mb.H2 * mb.W2; N = kF; K = k * k * kF; }
        if constexpr (OP == D1_FWD) { M = B; N = kD; K = mb.K1; }
        if constexpr (OP == D2_FWD) { M = B; N = a.classes; K = kD; }
        if constexpr (OP == D2_WGRAD) { M = kD + 1; N = a.classes; K = B; }
        if constexpr (OP == D2_DGRAD) { M = B; N = kD; K = a.classes; }
        if constexpr (OP == D1_WGRAD) { M = mb.K1 + 1; N = kD; K = B; }
        if constexpr (OP == D1_DGRAD) { M = B; N = mb.K1; K = kD; }
        if constexpr (OP == CONV2_DGRAD) {
            ry = aux / kStride; rx = aux % kStride;
            nyc = (mb.H1 - ry + kStride - 1) / kStride;
            nxc = (mb.W1 - rx + kStride - 1) / kStride;
            J = (k + kStride - 1) / kStride;
            M = B * nyc * nxc; N = kF; K = J * J * kF;
        }
        if constexpr (OP == CONV2_WGRAD) { M = k * k * kF + 1; N = kF; K = B * mb.H2 * mb.W2; kbeg = aux * kWgChunk; }
        if constexpr (OP == CONV1_WGRAD) { M = k * k * a.C + 1; N = kF; K = B * mb.H1 * mb.W1; kbeg = aux * kWgChunk; }
        kend = K;
        if constexpr (OP == CONV2_WGRAD || OP == CONV1_WGRAD) kend = min(K, kbeg + kWgChunk);
    }

    __device__ __forceinline__ long long sample(int b) const {
        return a.order[(long long)member * a.order_stride + a.row0 + b];
    }

    // what of A(m, .) does not depend on kk: a base pointer and up to three ints
    struct Row { const float* p; int i0, i1, i2; bool ok; };

    __device__ Row row(int m) const {
        Row r{nullptr, 0, 0, 0, m < M};
        if (!r.ok) return r;
        if constexpr (OP == CONV1_FWD) {
            const int hw = mb.H1 * mb.W1, b = m / hw, rem = m - b * hw, oy = rem / mb.W1, ox = rem - oy * mb.W1;
            r.p = a.x + sample(b) * ((long long)a.H * a.W * a.C) + ((long long)oy * kStride * a.W + ox * kStride) * a.C;
        }
        if constexpr (OP == CONV2_FWD) {
            const int hw = mb.H2 * mb.W2, b = m / hw, rem = m - b * hw, oy = rem / mb.W2, ox = rem - oy * mb.W2;
            r.p = a.act + mb.a1 + (((long long)b * mb.H1 + oy * kStride) * mb.W1 + ox * kStride) * kF;
        }
        if constexpr (OP == D1_FWD) r.p = a.act + mb.pd + (long long)m * mb.K1;
        if constexpr (OP == D2_FWD) r.p = a.act + mb.hd + (long long)m * kD;
        if constexpr (OP == D2_WGRAD) { r.p = a.act + mb.hd + m; r.i0 = m == kD; }
        if constexpr (OP == D1_WGRAD) { r.p = a.act + mb.pd + m; r.i0 = m == mb.K1; }
        if constexpr (OP == D2_DGRAD) r.p = a.act + mb.dz3 + (long long)m * a.classes;
        if constexpr (OP == D1_DGRAD) r.p = a.act + mb.dh + (long long)m * kD;
        if constexpr (OP == CONV2_DGRAD) {
            const int hw = nyc * nxc, b = m / hw, rem = m - b * hw;
            r.i0 = b; r.i1 = rem / nxc; r.i2 = rem - r.i1 * nxc;
            r.p = a.act + mb.dz2;
        }
        if constexpr (OP == CONV2_WGRAD) {
            const int tap = m / kF, c = m - tap * kF, ky = tap / mb.k, kx = tap - ky * mb.k;
            r.i0 = m == mb.k * mb.k * kF;
            r.p = a.act + mb.a1 + ((long long)ky * mb.W1 + kx) * kF + c;
        }
        if constexpr (OP == CONV1_WGRAD) {
            const int tap = m / a.C, c = m - tap * a.C, ky = tap / mb.k, kx = tap - ky * mb.k;
            r.i0 = m == mb.k * mb.k * a.C;
            r.i1 = (ky * a.W + kx) * a.C + c;
            r.p = a.x;
        }
        return r;
    }

    __device__ __forceinline__ float A(const Row& r, int kk) const {
        if (!r.ok || kk >= kend) return 0.f;
        if constexpr (OP == CONV1_FWD) {
            const int tap = kk / a.C, c = kk - tap * a.C, ky = tap / mb.k, kx = tap - ky * mb.k;
            return r.p[(ky * a.W + kx) * a.C + c];
        }
        if constexpr (OP == CONV2_FWD) {
            const int tap = kk / kF, c = kk - tap * kF, ky = tap / mb.k, kx = tap - ky * mb.k;
            return r.p[(ky * mb.W1 + kx) * kF + c];
        }
        if constexpr (OP == D1_FWD || OP == D2_FWD || OP == D2_DGRAD || OP == D1_DGRAD) return r.p[kk];
        if constexpr (OP == D2_WGRAD) return r.i0 ? 1.f : r.p[(long long)kk * kD];
        if constexpr (OP == D1_WGRAD) return r.i0 ? 1.f : r.p[(long long)kk * mb.K1];
        if constexpr (OP == CONV2_DGRAD) {
            const int j = kk / kF, f = kk - j * kF, jy = j / J, jx = j - jy * J;
            const int ky = ry + kStride * jy, kx = rx + kStride * jx, oy = r.i1 - jy, ox = r.i2 - jx;
            if (ky >= mb.k || kx >= mb.k || oy < 0 || ox < 0 || oy >= mb.H2 || ox >= mb.W2) return 0.f;
            return r.p[(((long long)r.i0 * mb.H2 + oy) * mb.W2 + ox) * kF + f];
        }
        if constexpr (OP == CONV2_WGRAD) {
            if (r.i0) return 1.f;
            const int hw = mb.H2 * mb.W2, b = kk / hw, rem = kk - b * hw, oy = rem / mb.W2, ox = rem - oy * mb.W2;
            return r.p[(((long long)b * mb.H1 + oy * kStride) * mb.W1 + ox * kStride) * kF];
        }
        if constexpr (OP == CONV1_WGRAD) {
            if (r.i0) return 1.f;
            const int hw = mb.H1 * mb.W1, b = kk / hw, rem = kk - b * hw, oy = rem / mb.W1, ox = rem - oy * mb.W1;
            return r.p[sample(b) * ((long long)a.H * a.W * a.C) + ((long long)oy * kStride * a.W + ox * kStride) * a.C + r.i1];
        }
        return 0.f;
    }

    __device__ __forceinline__ float Bv(int kk, int n) const {
        if (n >= N || kk >= kend) return 0.f;
        const float* P = a.params;
        if constexpr (OP == CONV1_FWD) return P[mb.w1 + (long long)kk * kF + n];
        if constexpr (OP == CONV2_FWD) return P[mb.w2 + (long long)kk * kF + n];
        if constexpr (OP == D1_FWD) return P[mb.w3 + (long long)kk * kD + n];
        if constexpr (OP == D2_FWD) return P[mb.w4 + (long long)kk * a.classes + n];
        if constexpr (OP == D2_WGRAD) return a.act[mb.dz3 + (long long)kk * a.classes + n];
        if constexpr (OP == D2_DGRAD) return P[mb.w4 + (long long)n * a.classes + kk];
        if constexpr (OP == D1_WGRAD) return a.act[mb.dh + (long long)kk * kD + n];
        if constexpr (OP == D1_DGRAD) return P[mb.w3 + (long long)n * kD + kk];
        if constexpr (OP == CONV2_DGRAD) {
            const int j = kk / kF, f = kk - j * kF, jy = j / J, jx = j - jy * J;
            const int ky = ry + kStride * jy, kx = rx + kStride * jx;
            if (ky >= mb.k || kx >= mb.k) return 0.f;
            return P[mb.w2 + ((long long)(ky * mb.k + kx) * kF + n) * kF + f];
        }
        if constexpr (OP == CONV2_WGRAD) return a.act[mb.dz2 + (long long)kk * kF + n];
        if constexpr (OP == CONV1_WGRAD) return a.act[mb.dz1 + (long long)kk * kF + n];
        return 0.f;
    }

    __device__ __forceinline__ void store(int m, int n, float v) const {
        if (m >= M || n >= N) return;
        float* act = a.act;
        if constexpr (OP == CONV1_FWD) act[mb.a1 + (long long)m * kF + n] = fmaxf(v + a.params[mb.b1 + n], 0.f);
        if constexpr (OP == CONV2_FWD) act[mb.a2 + (long long)m * kF + n] = fmaxf(v + a.params[mb.b2 + n], 0.f);
        if constexpr (OP == D1_FWD) {
            const float hv = fmaxf(v + a.params[mb.b3 + n], 0.f);
            const long long o = (long long)m * kD + n;
            act[mb.h + o] = hv;
            act[mb.hd + o] = hv * tc_mask(a, mb, 1, (unsigned)o);
        }
        if constexpr (OP == D2_FWD) act[mb.z3 + (long long)m * a.classes + n] = v + a.params[mb.b4 + n];
        if constexpr (OP == D2_WGRAD) a.grads[m == kD ? mb.b4 + n : mb.w4 + (long long)m * a.classes + n] = v;
        if constexpr (OP == D1_WGRAD) a.grads[m == mb.K1 ? mb.b3 + n : mb.w3 + (long long)m * kD + n] = v;
        if constexpr (OP == D2_DGRAD) {
            const long long o = (long long)m * kD + n;
            act[mb.dh + o] = act[mb.h + o] > 0.f ? v * tc_mask(a, mb, 1, (unsigned)o) : 0.f;
        }
        if constexpr (OP == D1_DGRAD) {
            const long long o = (long long)m * mb.K1 + n;
            act[mb.dp + o] = v * tc_mask(a, mb, 0, (unsigned)o);
        }
        if constexpr (OP == CONV2_DGRAD) {
            const int hw = nyc * nxc, b = m / hw, rem = m - b * hw, cy = rem / nxc, cx = rem - cy * nxc;
            const long long o = (((long long)b * mb.H1 + ry + kStride * cy) * mb.W1 + rx + kStride * cx) * kF + n;
            act[mb.dz1 + o] = act[mb.a1 + o] > 0.f ? v : 0.f;
        }
        if constexpr (OP == CONV2_WGRAD) act[mb.slab2 + ((long long)aux * M + m) * kF + n] = v;
        if constexpr (OP == CONV1_WGRAD) act[mb.slab1 + ((long long)aux * M + m) * kF + n] = v;
    }
};

// One 64 x 32 tile of one member's op: wave w owns rows [16 w, 16 w + 16), two 16-column
// accumulators; lane l feeds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] of each
// k-step of 4 and receives C[row 4 (l >> 4) + i][col l & 15].  K ascends in steps of 4.
template <int OP>
__global__ __launch_bounds__(256) void tc_gemm_kernel(TcArgs a, const TcItem* __restrict__ items) {
    const TcItem it = items[blockIdx.x];
    const TcMember& mb = a.mem[it.member];
    const TcGemm<OP> g(a, mb, it);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int mrow = it.m0 + wave * 16;
    if (mrow >= g.M) return;
    const typename TcGemm<OP>::Row row = g.row(mrow + r);
    const int n0 = it.n0 + r, n1 = n0 + 16;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // four k-steps' gathers in flight before their MFMAs (a step past kend reads zeros)
    for (int kb = g.kbeg; kb < g.kend; kb += 16) {
        float av[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = kb + 4 * u + q;
            av[u] = g.A(row, kk);
            b0[u] = g.Bv(kk, n0);
            b1[u] = g.Bv(kk, n1);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b0[u], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b1[u], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        g.store(mrow + q * 4 + i, n0, acc0[i]);
        g.store(mrow + q * 4 + i, n1, acc1[i]);
    }
}

// ============================================================================
// VALU kernels: grid (element chunks, members)
// ============================================================================
// max-pool 2x2 stride 2 (floor), first maximum in row-major window order; dropout layer 0
__global__ __launch_bounds__(256) void tc_pool_fwd_kernel(TcArgs a) {
    const TcMember& mb = a.mem[blockIdx.y];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.B * mb.K1) return;
    const int j = (int)(idx % mb.K1), b = (int)(idx / mb.K1);
    const int f = j % kF, px = (j / kF) % mb.Wp, py = j / kF / mb.Wp;
    const float* src = a.act + mb.a2 + (((long long)b * mb.H2 + 2 * py) * mb.W2 + 2 * px) * kF + f;
    float best = src[0];
    int arg = 0;
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float v = src[((long long)(w >> 1) * mb.W2 + (w & 1)) * kF];
        if (v > best) { best = v; arg = w; }
    }
    a.act[mb.pd + idx] = best * tc_mask(a, mb, 0, (unsigned)idx);
    reinterpret_cast<int*>(a.act + mb.am)[idx] = arg;
}

// dz2 over every a2 element: the pooled gradient at the window's argmax, gated by a2 > 0;
// zero elsewhere, the rows / columns the floor-mode pool drops included
__global__ __launch_bounds__(256) void tc_pool_bwd_kernel(TcArgs a) {
    const TcMember& mb = a.mem[blockIdx.y];
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.B * mb.H2 * mb.W2 * kF) return;
    const int f = (int)(idx % kF);
    long long p = idx / kF;
    const int x = (int)(p % mb.W2);
    p /= mb.W2;
    const int y = (int)(p % mb.H2), b = (int)(p / mb.H2);
    const int py = y >> 1, px = x >> 1;
    float v = 0.f;
    if (py < mb.Hp && px < mb.Wp) {
        const long long o = (long long)b * mb.K1 + ((long long)py * mb.Wp + px) * kF + f;
        if (reinterpret_cast<const int*>(a.act + mb.am)[o] == ((y & 1) << 1 | (x & 1)) && a.act[mb.a2 + idx] > 0.f)
            v = a.act[mb.dp + o];
    }
    a.act[mb.dz2 + idx] = v;
}

// softmax + Keras binary / categorical cross-entropy (oracle/cnn.py bce_loss_and_grad /
// cce_loss_and_grad with the class count in place of 10).  A workgroup per member, a thread
// per sample row.
__global__ __launch_bounds__(256) void tc_loss_kernel(TcArgs a) {
    const int member = blockIdx.x, B = a.B, nc = a.classes;
    const TcMember& mb = a.mem[member];
    float lsum = 0.f;
    int corr = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int y = a.labels[a.order[(long long)member * a.order_stride + a.row0 + b]];
        softmax_loss_row<kMaxClasses>(a.act + mb.z3 + (long long)b * nc, nc, y, mb.loss, B, a.train,
                                      a.act + mb.dz3 + (long long)b * nc, lsum, corr);
    }
    loss_finish(lsum, corr, B, a.train, a.loss_out + member, a.loss_sum + member, a.correct + member);
}

// weight-gradient slabs -> dw, db (slab order).  conv: 0 = conv1, 1 = conv2
__global__ __launch_bounds__(256) void tc_reduce_kernel(TcArgs a, int conv) {
    const TcMember& mb = a.mem[blockIdx.y];
    const int rows = mb.k * mb.k * (conv ? kF : a.C);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (rows + 1) * kF) return;
    const float* slab = a.act + (conv ? mb.slab2 : mb.slab1);
    const int S = conv ? mb.s2 : mb.s1;
    const long long stride = (long long)(rows + 1) * kF;
    float s = 0.f;
    for (int j = 0; j < S; ++j) s += slab[j * stride + i];
    const long long w = conv ? mb.w2 : mb.w1, bo = conv ? mb.b2 : mb.b1;
    a.grads[i < rows * kF ? w + i : bo + (i - rows * kF)] = s;
}

// Adam (Keras form): lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p -= lr_t m / (sqrt(v) + eps)
__global__ __launch_bounds__(256) void tc_adam_kernel(TcArgs a, float* __restrict__ mo, float* __restrict__ vo, int t) {
    const TcMember& mb = a.mem[blockIdx.y];
    const long long begin = mb.w1 + (long long)blockIdx.x * kAdamChunk;
    const long long end = min(mb.pend, begin + kAdamChunk);
    if (begin >= end) return;
    update_range(a.params, a.grads, mo, vo, begin, end, mb.lr, mb.opt, t, 0.9f, 0.999f, 1e-8f);
}

// ============================================================================
// Host-side plan
// ============================================================================
struct TcPlan {
    int n = 0, B = 0, H = 0, W = 0, C = 0, classes = 0;
    std::vector<TcMember> mem;
    std::vector<TcItem> lists[kNumOps];
    size_t off_mem = 0, off[kNumOps] = {};
    std::vector<char> host_tables;
    long long n_params = 0, act_floats = 0;
    size_t table_bytes = 0;
    long long max_pool = 0, max_a2 = 0, max_red1 = 0, max_red2 = 0, max_params = 0;
    float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *act = nullptr;
    char* table_base = nullptr;
    bool bound = false;
};

int tc_build_plan(TcPlan& P, const MpoTcSpec* specs, int n, int B, int H, int W, int C, int classes) {
    if (C < 1 || C > 8 || H < 1 || H > 256 || W < 1 || W > 256) {
        mpo::set_error("mpo_tc_create: input shape %d x %d x %d outside H, W 1..256, C 1..8", H, W, C);
        return MPO_ENOTSUP;
    }
    if (classes < 2 || classes > kMaxClasses) {
        mpo::set_error("mpo_tc_create: %d classes outside 2..%d", classes, kMaxClasses);
        return MPO_ENOTSUP;
    }
    P.n = n; P.B = B; P.H = H; P.W = W; P.C = C; P.classes = classes;
    P.mem.resize(n);
    long long po = 0, ao = 0;
    auto palloc = [&](long long cnt) { long long o = po; po += (cnt + 63) / 64 * 64; return o; };
    auto aalloc = [&](long long cnt) { long long o = ao; ao += (cnt + 63) / 64 * 64; return o; };
    for (int i = 0; i < n; ++i) {
        const MpoTcSpec& s = specs[i];
        TcMember& m = P.mem[i];
        std::memset(&m, 0, sizeof(m));
        const int k = s.kernel_size;
        if (k < 1 || k > 9) {
            mpo::set_error("mpo_tc_create: member %d has kernel_size %d outside 1..9", i, k);
            return MPO_ENOTSUP;
        }
        if (!(s.lr > 0.f) || !std::isfinite(s.lr) || !std::isfinite(s.dropout)) {
            mpo::set_error("mpo_tc_create: member %d has lr %g / dropout %g (lr > 0, both finite)", i, s.lr, s.dropout);
            return MPO_ENOTSUP;
        }
        const int loss = s.options & MPO_LOSS_MASK, opt = s.options & MPO_OPT_MASK;
        if ((s.options & ~(MPO_LOSS_MASK | MPO_OPT_MASK)) || (loss != MPO_LOSS_BCE && loss != MPO_LOSS_CCE) ||
            (opt != MPO_OPT_ADAM && opt != MPO_OPT_SGD)) {
            mpo::set_error("mpo_tc_create: member %d has unsupported options 0x%x", i, (unsigned)s.options);
            return MPO_ENOTSUP;
        }
        m.k = k;
        m.H1 = H >= k ? (H - k) / kStride + 1 : 0;
        m.W1 = W >= k ? (W - k) / kStride + 1 : 0;
        m.H2 = m.H1 >= k ? (m.H1 - k) / kStride + 1 : 0;
        m.W2 = m.W1 >= k ? (m.W1 - k) / kStride + 1 : 0;
        if (m.H2 < 2 || m.W2 < 2) {
            mpo::set_error("mpo_tc_create: member %d (kernel_size %d on %d x %d) has a conv2 output of %d x %d, below "
                           "the 2 x 2 the max-pool needs", i, k, H, W, m.H2, m.W2);
            return MPO_ENOTSUP;
        }
        m.Hp = m.H2 / 2; m.Wp = m.W2 / 2;
        m.K1 = m.Hp * m.Wp * kF;
        m.lr = s.lr; m.seed = s.seed; m.loss = loss; m.opt = opt;
        const float r0 = s.dropout / 2.f, r1 = s.dropout;
        m.drop0 = r0 > 0.f && r0 < 1.f;
        m.drop1 = r1 > 0.f && r1 < 1.f;
        m.inv0 = m.drop0 ? 1.f / (1.f - r0) : 1.f;
        m.inv1 = m.drop1 ? 1.f / (1.f - r1) : 1.f;
        m.thr0 = m.drop0 ? (unsigned)std::ceil((double)r0 * 16777216.0) : 0u;
        m.thr1 = m.drop1 ? (unsigned)std::ceil((double)r1 * 16777216.0) : 0u;
        m.w1 = palloc((long long)k * k * C * kF); m.b1 = palloc(kF);
        m.w2 = palloc((long long)k * k * kF * kF); m.b2 = palloc(kF);
        m.w3 = palloc((long long)m.K1 * kD); m.b3 = palloc(kD);
        m.w4 = palloc((long long)kD * classes); m.b4 = palloc(classes);
        m.pend = po;
        const long long p1 = (long long)B * m.H1 * m.W1, p2 = (long long)B * m.H2 * m.W2;
        // slabs: a function of the member's geometry and the batch alone (member isolation)
        m.s1 = (int)((p1 + kWgChunk - 1) / kWgChunk);
        m.s2 = (int)((p2 + kWgChunk - 1) / kWgChunk);
        m.a1 = aalloc(p1 * kF); m.a2 = aalloc(p2 * kF);
        m.pd = aalloc((long long)B * m.K1); m.am = aalloc((long long)B * m.K1);
        m.h = aalloc((long long)B * kD); m.hd = aalloc((long long)B * kD);
        m.z3 = aalloc((long long)B * classes); m.dz3 = aalloc((long long)B * classes);
        m.dh = aalloc((long long)B * kD); m.dp = aalloc((long long)B * m.K1);
        m.dz2 = aalloc(p2 * kF); m.dz1 = aalloc(p1 * kF);
        const int r1w = k * k * C + 1, r2w = k * k * kF + 1;
        m.slab1 = aalloc((long long)m.s1 * r1w * kF);
        m.slab2 = aalloc((long long)m.s2 * r2w * kF);

        auto tiles = [&](int op, long long M, int N, int aux) {
            for (long long m0 = 0; m0 < M; m0 += kTileM)
                for (int n0 = 0; n0 < N; n0 += kTileN) P.lists[op].push_back({i, (int)m0, n0, aux});
        };
        tiles(CONV1_FWD, p1, kF, 0);
        tiles(CONV2_FWD, p2, kF, 0);
        tiles(D1_FWD, B, kD, 0);
        tiles(D2_FWD, B, classes, 0);
        tiles(D2_WGRAD, kD + 1, classes, 0);
        tiles(D2_DGRAD, B, kD, 0);
        tiles(D1_WGRAD, m.K1 + 1, kD, 0);
        tiles(D1_DGRAD, B, m.K1, 0);
        for (int cls = 0; cls < kStride * kStride; ++cls) {
            const int ry = cls / kStride, rx = cls % kStride;
            const long long nyc = (m.H1 - ry + kStride - 1) / kStride, nxc = (m.W1 - rx + kStride - 1) / kStride;
            tiles(CONV2_DGRAD, (long long)B * nyc * nxc, kF, cls);
        }
        for (int sl = 0; sl < m.s2; ++sl) tiles(CONV2_WGRAD, r2w, kF, sl);
        for (int sl = 0; sl < m.s1; ++sl) tiles(CONV1_WGRAD, r1w, kF, sl);
        P.max_pool = std::max(P.max_pool, (long long)B * m.K1);
        P.max_a2 = std::max(P.max_a2, p2 * kF);
        P.max_red1 = std::max(P.max_red1, (long long)r1w * kF);
        P.max_red2 = std::max(P.max_red2, (long long)r2w * kF);
        P.max_params = std::max(P.max_params, m.pend - m.w1);
    }
    P.n_params = po;
    P.act_floats = ao;
    size_t off = 0;
    auto put = [&](size_t& slot, const void* src, size_t bytes) {
        slot = off;
        off = mpo::align_up(off + bytes, 256);
        P.host_tables.resize(off);
        if (bytes) std::memcpy(P.host_tables.data() + slot, src, bytes);
    };
    put(P.off_mem, P.mem.data(), P.mem.size() * sizeof(TcMember));
    for (int op = 0; op < kNumOps; ++op) put(P.off[op], P.lists[op].data(), P.lists[op].size() * sizeof(TcItem));
    P.table_bytes = off;
    return MPO_OK;
}

TcArgs tc_args(const TcPlan& P, const float* x, const int* labels, const int* order, long long order_stride,
               long long row0, int step, int train) {
    TcArgs a{};
    a.mem = reinterpret_cast<const TcMember*>(P.table_base + P.off_mem);
    a.params = P.params; a.grads = P.grads; a.act = P.act;
    a.x = x; a.labels = labels; a.order = order; a.order_stride = order_stride; a.row0 = row0;
    a.B = P.B; a.H = P.H; a.W = P.W; a.C = P.C; a.classes = P.classes;
    a.step = step; a.train = train;
    return a;
}

template <int OP>
int tc_launch(const TcPlan& P, const TcArgs& a, hipStream_t s) {
    const size_t cnt = P.lists[OP].size();
    if (!cnt) return MPO_OK;
    hipLaunchKernelGGL(tc_gemm_kernel<OP>, dim3((unsigned)cnt), dim3(256), 0, s, a,
                       reinterpret_cast<const TcItem*>(P.table_base + P.off[OP]));
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

inline unsigned tc_blocks(long long elems, int per) { return (unsigned)((elems + per - 1) / per); }

#define TC_RUN(call)            \
    do {                        \
        const int rc_ = (call); \
        if (rc_) return rc_;    \
    } while (0)

int tc_forward(const TcPlan& P, const TcArgs& a, hipStream_t s) {
    TC_RUN(tc_launch<CONV1_FWD>(P, a, s));
    TC_RUN(tc_launch<CONV2_FWD>(P, a, s));
    hipLaunchKernelGGL(tc_pool_fwd_kernel, dim3(tc_blocks(P.max_pool, 256), (unsigned)P.n), dim3(256), 0, s, a);
    MPO_LAUNCH_CHECK();
    TC_RUN(tc_launch<D1_FWD>(P, a, s));
    TC_RUN(tc_launch<D2_FWD>(P, a, s));
    hipLaunchKernelGGL(tc_loss_kernel, dim3((unsigned)P.n), dim3(256), 0, s, a);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

int tc_train(const TcPlan& P, const TcArgs& a, hipStream_t s) {
    TC_RUN(tc_forward(P, a, s));
    TC_RUN(tc_launch<D2_WGRAD>(P, a, s));
    TC_RUN(tc_launch<D2_DGRAD>(P, a, s));
    TC_RUN(tc_launch<D1_WGRAD>(P, a, s));
    TC_RUN(tc_launch<D1_DGRAD>(P, a, s));
    const unsigned nm = (unsigned)P.n;
    hipLaunchKernelGGL(tc_pool_bwd_kernel, dim3(tc_blocks(P.max_a2, 256), nm), dim3(256), 0, s, a);
    MPO_LAUNCH_CHECK();
    TC_RUN(tc_launch<CONV2_WGRAD>(P, a, s));
    TC_RUN(tc_launch<CONV2_DGRAD>(P, a, s));
    TC_RUN(tc_launch<CONV1_WGRAD>(P, a, s));
    hipLaunchKernelGGL(tc_reduce_kernel, dim3(tc_blocks(P.max_red2, 256), nm), dim3(256), 0, s, a, 1);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(tc_reduce_kernel, dim3(tc_blocks(P.max_red1, 256), nm), dim3(256), 0, s, a, 0);
    MPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(tc_adam_kernel, dim3(tc_blocks(P.max_params, kAdamChunk), nm), dim3(256), 0, s, a, P.m, P.v,
                       a.step + 1);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
}

}  // namespace

extern "C" {

int mpo_tc_create(const MpoTcSpec* specs, int n_members, int batch, int H, int W, int C, int classes, void** handle) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(specs && handle, "mpo_tc_create: null pointer");
    MPO_CHECK_ARG(n_members > 0 && batch > 0 && batch <= 256, "mpo_tc_create: n_members=%d batch=%d (1..256)", n_members,
                  batch);
    auto P = std::make_unique<TcPlan>();
    const int rc = tc_build_plan(*P, specs, n_members, batch, H, W, C, classes);
    if (rc) return rc;
    *handle = P.release();
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_tc_destroy(void* handle) {
    delete static_cast<TcPlan*>(handle);
    return MPO_OK;
}

int mpo_tc_sizes(const void* handle, MpoPopSizes* out) {
    MPO_CHECK_ARG(handle && out, "mpo_tc_sizes: null pointer");
    const TcPlan& P = *static_cast<const TcPlan*>(handle);
    fill_sizes(P, out);
    return MPO_OK;
}

int mpo_tc_param_layout(const void* handle, int member, int64_t* offsets) {
    MPO_CHECK_ARG(handle && offsets, "mpo_tc_param_layout: null pointer");
    const TcPlan& P = *static_cast<const TcPlan*>(handle);
    MPO_CHECK_ARG(member >= 0 && member < P.n, "mpo_tc_param_layout: member %d out of range", member);
    const TcMember& m = P.mem[member];
    const long long o[9] = {m.w1, m.b1, m.w2, m.b2, m.w3, m.b3, m.w4, m.b4, m.pend};
    copy_offsets(o, offsets);
    return MPO_OK;
}

int mpo_tc_act_layout(const void* handle, int member, int64_t* offsets) {
    MPO_CHECK_ARG(handle && offsets, "mpo_tc_act_layout: null pointer");
    const TcPlan& P = *static_cast<const TcPlan*>(handle);
    MPO_CHECK_ARG(member >= 0 && member < P.n, "mpo_tc_act_layout: member %d out of range", member);
    const TcMember& m = P.mem[member];
    const long long o[12] = {m.a1, m.a2, m.pd, m.am, m.h, m.hd, m.z3, m.dz3, m.dh, m.dp, m.dz2, m.dz1};
    copy_offsets(o, offsets);
    return MPO_OK;
}

int mpo_tc_bind(void* handle, float* params, float* grads, float* adam_m, float* adam_v, float* act, void* tables,
                void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(handle && params && grads && adam_m && adam_v && act && tables, "mpo_tc_bind: null pointer");
    TcPlan& P = *static_cast<TcPlan*>(handle);
    P.params = params; P.grads = grads; P.m = adam_m; P.v = adam_v; P.act = act;
    P.table_base = static_cast<char*>(tables);
    MPO_HIP(hipMemcpyAsync(tables, P.host_tables.data(), P.table_bytes, hipMemcpyHostToDevice,
                           static_cast<hipStream_t>(stream)));
    MPO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    P.bound = true;
    return MPO_OK;
    MPO_GUARD_END
}

int mpo_tc_train_step(void* handle, const float* x, const int32_t* labels, const int32_t* order, int64_t order_stride,
                      int64_t row0, int32_t step, float* loss_out, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(handle && x && labels && order && loss_out, "mpo_tc_train_step: null pointer");
    TcPlan& P = *static_cast<TcPlan*>(handle);
    MPO_CHECK_ARG(P.bound, "mpo_tc_train_step: call mpo_tc_bind first");
    MPO_CHECK_ARG(step >= 0 && row0 >= 0, "mpo_tc_train_step: step and row0 must be >= 0");
    TcArgs a = tc_args(P, x, labels, order, order_stride, row0, step, 1);
    a.loss_out = loss_out;
    return tc_train(P, a, static_cast<hipStream_t>(stream));
    MPO_GUARD_END
}

int mpo_tc_eval_step(void* handle, const float* x, const int32_t* labels, const int32_t* order, int64_t order_stride,
                     int64_t row0, float* loss_sum, int32_t* correct, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(handle && x && labels && order && loss_sum && correct, "mpo_tc_eval_step: null pointer");
    TcPlan& P = *static_cast<TcPlan*>(handle);
    MPO_CHECK_ARG(P.bound, "mpo_tc_eval_step: call mpo_tc_bind first");
    MPO_CHECK_ARG(row0 >= 0, "mpo_tc_eval_step: row0 must be >= 0");
    TcArgs a = tc_args(P, x, labels, order, order_stride, row0, 0, 0);
    a.loss_sum = loss_sum;
    a.correct = correct;
    return tc_forward(P, a, static_cast<hipStream_t>(stream));
    MPO_GUARD_END
}

}  // extern "C"
