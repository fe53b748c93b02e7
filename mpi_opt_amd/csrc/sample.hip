// sample.hip -- acquisition candidates drawn on the device (mpo_space_sample).
//
// Candidate i of a search space is a pure function of (seed, i): one Philox4x32-10
// block per pair of original dimensions, counter (i lo, i hi, pair, 0), key (seed lo,
// seed hi), mapped into the transformed space the GP scores (include/mpo.h has the
// law).  No state, no LDS, no workspace: any slice [first, first + m) of the set can
// be produced on any device and equals the same rows of the whole.
#include "mpo_internal.h"

namespace {

constexpr int kMaxCols = 32;      // the GP's limit on transformed dimensions
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // 8 workgroups for each of 256 CUs; the grid strides past that

// One original dimension: its kind, its first transformed column and its count.
// 32 x 16 B, passed to the kernel by value.
struct Dim {
    int32_t kind;
    int32_t col;
    int64_t count;     // MpoDimDesc.count (0 for a Real)
};
struct DimTable {
    Dim c[kMaxCols];
};

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                              uint32_t c3, uint32_t (&r)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        // 32 x 32 -> 64 bit products: one v_mad_u64_u32 each, not a mul_hi / mul_lo pair
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// 27 + 26 bits: exact in fp64, in [0, 1)
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6)) * 0x1p-53;
}

__device__ __forceinline__ bool one_hot(const Dim& dm) { return dm.kind == MPO_DIM_CATEGORICAL && dm.count > 2; }

// The single column of a dimension that takes one (every kind but a one-hot Categorical).
__device__ __forceinline__ double single_value(const Dim& dm, double u) {
    if (dm.kind == MPO_DIM_REAL) return u;
    const double s = (double)dm.count;
    if (dm.kind == MPO_DIM_INTEGER) return dm.count == 0 ? 0.0 : rint(u * s) / s;
    return (double)min((int)(u * s), (int)dm.count - 1);
}

__device__ __forceinline__ void store_dim(const Dim& dm, double u, double* __restrict__ p) {
    if (!one_hot(dm)) {
        *p = single_value(dm, u);
        return;
    }
    const int c = (int)dm.count;
    const int j = min((int)(u * (double)c), c - 1);
    for (int k = 0; k < c; ++k) p[k] = k == j ? 1.0 : 0.0;
}

// One work item is (candidate row, pair b of original dimensions): one Philox block,
// whose two draws fill the columns of dimensions 2b and 2b + 1 -- adjacent in the row.
// Items are numbered row-major (row * n_pairs + b) and thread t of the grid takes items
// t, t + grid, ...: consecutive lanes write consecutive runs of a row-major output, so a
// wave's stores cover contiguous memory, 16 B per lane where both dimensions take one
// column (one 16 B store where that address is 16 B aligned, two 8 B stores otherwise).
// (row, b) advance by the stride's quotient and remainder (sq, sr): no division in the loop.
__global__ __launch_bounds__(kBlock) void space_sample_kernel(const DimTable t, const int n_dims, const int d,
                                                              const uint32_t k0, const uint32_t k1,
                                                              const uint64_t first, const int64_t m,
                                                              const uint32_t sq, const uint32_t sr,
                                                              double* __restrict__ out) {
    const int n_pairs = (n_dims + 1) >> 1;
    const uint32_t gt = blockIdx.x * kBlock + threadIdx.x;
    int64_t row = gt / (uint32_t)n_pairs;
    int b = (int)(gt % (uint32_t)n_pairs);
    for (; row < m; ) {
        const uint64_t i = first + (uint64_t)row;
        uint32_t r[4];
        philox4x32_10(k0, k1, (uint32_t)i, (uint32_t)(i >> 32), (uint32_t)b, 0u, r);
        const Dim d0 = t.c[2 * b];
        const double u0 = u53(r[0], r[1]), u1 = u53(r[2], r[3]);
        double* __restrict__ p = out + row * d + d0.col;
        if (2 * b + 1 < n_dims) {
            const Dim d1 = t.c[2 * b + 1];
            if (!one_hot(d0) && !one_hot(d1)) {
                const double v0 = single_value(d0, u0), v1 = single_value(d1, u1);
                if (((uintptr_t)p & 15) == 0) {
                    *reinterpret_cast<double2*>(p) = make_double2(v0, v1);
                } else {
                    p[0] = v0;
                    p[1] = v1;
                }
            } else {
                store_dim(d0, u0, p);
                store_dim(d1, u1, out + row * d + d1.col);
            }
        } else {
            store_dim(d0, u0, p);
        }
        b += (int)sr;
        row += sq;
        if (b >= n_pairs) {
            b -= n_pairs;
            ++row;
        }
    }
}

}  // namespace

extern "C" int mpo_space_sample(const MpoDimDesc* dims, int n_dims, int d, uint64_t seed, int64_t first, int64_t m,
                                double* out, void* stream) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(dims, "mpo_space_sample: null dimension table");
    MPO_CHECK_ARG(n_dims >= 1 && n_dims <= kMaxCols, "mpo_space_sample: n_dims=%d outside [1, %d]", n_dims, kMaxCols);
    MPO_CHECK_ARG(d >= 1 && d <= kMaxCols, "mpo_space_sample: d=%d outside [1, %d]", d, kMaxCols);
    DimTable t{};
    int width = 0;
    for (int j = 0; j < n_dims; ++j) {
        const int32_t kind = dims[j].kind;
        const int64_t count = dims[j].count;
        int w = 1;
        if (kind == MPO_DIM_INTEGER) {
            MPO_CHECK_ARG(count >= 0 && count < ((int64_t)1 << 52),
                          "mpo_space_sample: dimension %d: Integer span %lld outside [0, 2^52)", j, (long long)count);
        } else if (kind == MPO_DIM_CATEGORICAL) {
            MPO_CHECK_ARG(count >= 1, "mpo_space_sample: dimension %d: Categorical with %lld categories", j,
                          (long long)count);
            if (count > 2) w = count > kMaxCols ? kMaxCols + 1 : (int)count;
        } else {
            MPO_CHECK_ARG(kind == MPO_DIM_REAL, "mpo_space_sample: dimension %d: unknown kind %d", j, (int)kind);
        }
        t.c[j] = Dim{kind, width, kind == MPO_DIM_REAL ? 0 : count};
        width += w;
        MPO_CHECK_ARG(width <= kMaxCols, "mpo_space_sample: the dimensions take more than %d transformed columns",
                      kMaxCols);
    }
    MPO_CHECK_ARG(width == d, "mpo_space_sample: d=%d but the dimensions take %d transformed columns", d, width);
    MPO_CHECK_ARG(first >= 0 && m >= 0, "mpo_space_sample: negative first=%lld or m=%lld", (long long)first,
                  (long long)m);
    MPO_CHECK_ARG(first <= ((int64_t)1 << 62) && m <= ((int64_t)1 << 62) - first,
                  "mpo_space_sample: first + m = %lld + %lld exceeds 2^62", (long long)first, (long long)m);
    if (m == 0) return MPO_OK;
    MPO_CHECK_ARG(out, "mpo_space_sample: null output");
    MPO_CHECK_ARG(((uintptr_t)out & 7) == 0, "mpo_space_sample: output not 8-byte aligned");
    if (m > INT64_MAX / (8 * kMaxCols)) {
        mpo::set_error("mpo_space_sample: m=%lld rows do not fit an address space", (long long)m);
        return MPO_ENOTSUP;
    }
    const int n_pairs = (n_dims + 1) / 2;
    const int64_t items = m * n_pairs;
    const int64_t want = (items + kBlock - 1) / kBlock;
    const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    const uint32_t stride = blocks * kBlock;
    hipLaunchKernelGGL(space_sample_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), t,
                       n_dims, d, (uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)first, m,
                       stride / (uint32_t)n_pairs, stride % (uint32_t)n_pairs, out);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}
