// One wave's running top-k of (value, index), shared by the elementwise finish passes
// (gp_ps.hip ps_finish_kernel, gp_committee.hip committee_fold_kernel): their per-wave lists
// go out in the [part][3][k] layout that mpo::topk_merge reads.
#pragma once

#include "mpo_internal.h"
#include "gp_acq_math.h"

namespace mpo {

// One wave's running top-k of (value, index), the same list in every lane.
struct WaveTopk {
    double v[MPO_TOPK_MAX];
    long long i[MPO_TOPK_MAX];
    double thr_v;     // entry k - 1: what a candidate has to beat
    long long thr_i;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int r = 0; r < MPO_TOPK_MAX; ++r) { v[r] = __builtin_huge_val(); i[r] = 0x7fffffffffffffffLL; }
        thr_v = v[0];
        thr_i = i[0];
    }
    // the lanes' candidates (cv, ci) of one step; at most k of them enter
    __device__ __forceinline__ void offer(double cv, long long ci, int k) {
        while (__ballot(lex_less(cv, ci, thr_v, thr_i))) {
            double bv = cv;
            long long bi = ci;
            wave_lex_min(bv, bi);
            if (ci == bi) { cv = __builtin_huge_val(); ci = 0x7fffffffffffffffLL; }
#pragma unroll
            for (int s = 0; s < MPO_TOPK_MAX; ++s) {
                if (s < k && lex_less(bv, bi, v[s], i[s])) {
                    const double tv = v[s];
                    const long long ti = i[s];
                    v[s] = bv; i[s] = bi; bv = tv; bi = ti;
                }
            }
#pragma unroll
            for (int s = 0; s < MPO_TOPK_MAX; ++s) {
                if (s == k - 1) { thr_v = v[s]; thr_i = i[s]; }
            }
        }
    }
    __device__ __forceinline__ void store(long long* __restrict__ pi, double* __restrict__ pv, size_t off, int k) const {
#pragma unroll
        for (int r = 0; r < MPO_TOPK_MAX; ++r) {
            if (r < k) { pv[off + r] = v[r]; pi[off + r] = i[r]; }
        }
    }
};

}  // namespace mpo
