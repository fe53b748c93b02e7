// What the MNIST (cnn.hip) and topclass (topclass.hip) population engines compute alike: the
// dropout counter hash, the softmax + Keras cross-entropy of one sample row with its fold over
// the batch, the Keras Adam / SGD update of a parameter range, and the two host queries that
// copy a plan's sizes and a member's offsets out.  One copy, pinned to oracle/cnn.py once.
//
// densenet.hip shares none of the device routines, on purpose: its head computes the
// categorical cross-entropy on one thread per sample with double sums, and its Adam folds the
// l2 gradient in.  Those are other computations, not copies of these.
#pragma once

#include "mpo_internal.h"

namespace mpo {
namespace pop {

// Keras clips probabilities to [1e-7, 1 - 1e-7] before the logarithm
constexpr float kClipEps = 1e-7f;

// ---- dropout counter hash (identical in oracle/cnn.py) ---------------------
__device__ __forceinline__ unsigned lowbias32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ unsigned drop_base(unsigned seed, int step, int layer) {
    unsigned b = lowbias32(seed ^ (unsigned)(layer * 0x9E3779B9u));
    return lowbias32(b ^ (unsigned)step);
}

__device__ __forceinline__ bool drop_keep(unsigned base, unsigned elem, unsigned thr) {
    return (lowbias32(elem ^ base) >> 8) >= thr;
}

// softmax + Keras binary / categorical cross-entropy (oracle/cnn.py bce_loss_and_grad /
// cce_loss_and_grad) of one sample: logits z [nc], label y, batch B.  Adds the sample's loss
// to lsum and its hit to corr; in training writes d loss / d logits to dz [nc].  Arrays hold
// MAXC lanes; lanes c >= nc contribute exact zeros.
template <int MAXC>
__device__ __forceinline__ void softmax_loss_row(const float* z, int nc, int y, int loss, int B, int train, float* dz,
                                                 float& lsum, int& corr) {
    float zm = z[0];
    int am = 0;
    for (int c = 1; c < nc; ++c) if (z[c] > zm) { zm = z[c]; am = c; }
    float e[MAXC], s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) { e[c] = c < nc ? expf(z[c] - zm) : 0.f; s += e[c]; }
    corr += (am == y);
    if (loss == MPO_LOSS_CCE) {
        // Keras categorical_crossentropy: q = p / sum p, clipped target probability;
        // d loss / d logits = live (q - onehot) / B (the DenseNet head's form)
        float q[MAXC], S2 = 0.f, qt = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { q[c] = e[c] / s; S2 += q[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) { q[c] /= S2; if (c == y) qt = q[c]; }
        lsum += -logf(fminf(fmaxf(qt, kClipEps), 1.f - kClipEps));
        if (train) {
            const float live = (qt >= kClipEps && qt <= 1.f - kClipEps) ? 1.f / (float)B : 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) if (c < nc) dz[c] = live * (q[c] - (c == y ? 1.f : 0.f));
        }
        return;
    }
    float l = 0.f, gdot = 0.f, gp[MAXC], pr[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        gp[c] = pr[c] = 0.f;
        if (c >= nc) continue;
        const float p = e[c] / s;
        pr[c] = p;
        const float t = (c == y) ? 1.f : 0.f;
        const float pc = fminf(fmaxf(p, kClipEps), 1.f - kClipEps);
        l += -(t * logf(pc) + (1.f - t) * logf(1.f - pc));
        const bool inside = p > kClipEps && p < 1.f - kClipEps;
        gp[c] = inside ? (pc - t) / (pc * (1.f - pc)) / (float)(nc * B) : 0.f;
        gdot += gp[c] * p;
    }
    lsum += l / (float)nc;
    if (train) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) if (c < nc) dz[c] = pr[c] * (gp[c] - gdot);
    }
}

// Fold of a 256-thread workgroup's (lsum, corr) in a fixed order, then the member's result:
// the mean batch loss in training, the running loss sum and hit count in evaluation.
__device__ __forceinline__ void loss_finish(float lsum, int corr, int B, int train, float* loss_out, float* loss_sum,
                                            int* correct) {
    __shared__ float red[256];
    __shared__ int redc[256];
    const int tid = threadIdx.x;
    red[tid] = lsum;
    redc[tid] = corr;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[tid] += red[tid + s]; redc[tid] += redc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (train) {
            *loss_out = red[0] / (float)B;
        } else {
            *loss_sum += red[0];
            *correct += redc[0];
        }
    }
}

// One workgroup's update of params [begin, end).  MPO_OPT_SGD: Keras SGD, no momentum.
// Otherwise Adam (Keras form): lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); p -= lr_t m / (sqrt(v) + eps)
__device__ __forceinline__ void update_range(float* __restrict__ params, const float* __restrict__ grads,
                                             float* __restrict__ mo, float* __restrict__ vo, long long begin,
                                             long long end, float lr, int opt, int t, float b1, float b2, float eps) {
    if (opt == MPO_OPT_SGD) {
        for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) params[i] -= lr * grads[i];
        return;
    }
    const double corr = sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t));
    const float lr_t = (float)(lr * corr);
    for (long long i = begin + threadIdx.x; i < end; i += blockDim.x) {
        const float g = grads[i];
        const float m = b1 * mo[i] + (1.f - b1) * g;
        const float v = b2 * vo[i] + (1.f - b2) * g * g;
        mo[i] = m;
        vo[i] = v;
        params[i] -= lr_t * m / (sqrtf(v) + eps);
    }
}

// ---- host: the queries both engines answer from their plan -----------------
template <class PlanT>
inline void fill_sizes(const PlanT& P, MpoPopSizes* out) {
    out->n_params = P.n_params;
    out->act_floats = P.act_floats;
    out->table_bytes = (int64_t)P.table_bytes;
    out->n_members = P.n;
    out->batch = P.B;
}

template <int N>
inline void copy_offsets(const long long (&o)[N], int64_t* offsets) {
    for (int i = 0; i < N; ++i) offsets[i] = o[i];
}

}  // namespace pop
}  // namespace mpo
