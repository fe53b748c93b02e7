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

// The host checks the entry points share, in mpo_space_sample's order and words.  The
// dimension table into `t`; with `d` (null where the caller writes no rows) also the
// transformed widths against it.
int check_dims(const char* fn, const MpoDimDesc* dims, int n_dims, const int* d, DimTable& t) {
    MPO_CHECK_ARG(dims, "%s: null dimension table", fn);
    MPO_CHECK_ARG(n_dims >= 1 && n_dims <= kMaxCols, "%s: n_dims=%d outside [1, %d]", fn, n_dims, kMaxCols);
    MPO_CHECK_ARG(!d || (*d >= 1 && *d <= kMaxCols), "%s: d=%d outside [1, %d]", fn, d ? *d : 0, kMaxCols);
    int width = 0;
    for (int j = 0; j < n_dims; ++j) {
        const int32_t kind = dims[j].kind;
        const int64_t count = dims[j].count;
        int w = 1;
        if (kind == MPO_DIM_INTEGER) {
            MPO_CHECK_ARG(count >= 0 && count < ((int64_t)1 << 52),
                          "%s: dimension %d: Integer span %lld outside [0, 2^52)", fn, j, (long long)count);
        } else if (kind == MPO_DIM_CATEGORICAL) {
            MPO_CHECK_ARG(count >= 1, "%s: dimension %d: Categorical with %lld categories", fn, j, (long long)count);
            if (count > 2) w = count > kMaxCols ? kMaxCols + 1 : (int)count;
        } else {
            MPO_CHECK_ARG(kind == MPO_DIM_REAL, "%s: dimension %d: unknown kind %d", fn, j, (int)kind);
        }
        if (!d) continue;
        t.c[j] = Dim{kind, width, kind == MPO_DIM_REAL ? 0 : count};
        width += w;
        MPO_CHECK_ARG(width <= kMaxCols, "%s: the dimensions take more than %d transformed columns", fn, kMaxCols);
    }
    MPO_CHECK_ARG(!d || width == *d, "%s: d=%d but the dimensions take %d transformed columns", fn, d ? *d : 0, width);
    return MPO_OK;
}

// The rows [first, first + m) of a candidate set.
int check_rows(const char* fn, int64_t first, int64_t m) {
    MPO_CHECK_ARG(first >= 0 && m >= 0, "%s: negative first=%lld or m=%lld", fn, (long long)first, (long long)m);
    MPO_CHECK_ARG(first <= ((int64_t)1 << 62) && m <= ((int64_t)1 << 62) - first,
                  "%s: first + m = %lld + %lld exceeds 2^62", fn, (long long)first, (long long)m);
    return MPO_OK;
}

// The output of m > 0 rows.
int check_out(const char* fn, int64_t m, const double* out) {
    MPO_CHECK_ARG(out, "%s: null output", fn);
    MPO_CHECK_ARG(((uintptr_t)out & 7) == 0, "%s: output not 8-byte aligned", fn);
    if (m > INT64_MAX / (8 * kMaxCols)) {
        mpo::set_error("%s: m=%lld rows do not fit an address space", fn, (long long)m);
        return MPO_ENOTSUP;
    }
    return MPO_OK;
}

// Grid of one thread per (row, pair) item, capped at kMaxBlocks workgroups.
unsigned item_blocks(int64_t m, int n_pairs) {
    const int64_t want = (m * n_pairs + kBlock - 1) / kBlock;
    return (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
}

// ---- the lattice of the discrete dimensions (mpo_space_lattice) -------------------------

// Place value of every discrete dimension in the mixed-radix number of a lattice point (the
// last discrete dimension has place 1); unused for a Real.  32 x 8 B, by value.
struct PlaceTable {
    int64_t p[kMaxCols];
};

__host__ __device__ __forceinline__ int64_t radix(int32_t kind, int64_t count) {
    return kind == MPO_DIM_INTEGER ? count + 1 : count;
}

// L and the place values of a checked dimension table; MPO_EINVAL when L exceeds 2^62.
int lattice_places(const char* fn, const MpoDimDesc* dims, int n_dims, PlaceTable* places, int64_t* L) {
    int64_t prod = 1;
    for (int j = n_dims - 1; j >= 0; --j) {
        if (dims[j].kind == MPO_DIM_REAL) continue;
        if (places) places->p[j] = prod;
        const int64_t r = radix(dims[j].kind, dims[j].count);
        MPO_CHECK_ARG(r <= ((int64_t)1 << 62) / prod, "%s: the lattice of the discrete dimensions exceeds 2^62 points",
                      fn);
        prod *= r;
    }
    *L = prod;
    return MPO_OK;
}

// Digit of dimension dm in lattice point l.  W is uint32_t when L < 2^32 (every place and
// radix then fits as well) and uint64_t otherwise: the same integers either way.
template <class W>
__device__ __forceinline__ int64_t digit(const Dim& dm, int64_t place, W l) {
    return (int64_t)((l / (W)place) % (W)radix(dm.kind, dm.count));
}

// One dimension's cell of a lattice row: a Real takes the draw u, a discrete dimension its
// digit k.  `v` is the column of a dimension that takes one, `k` the hot column of a one-hot.
struct Cell {
    double v;
    int k;
};
template <class W>
__device__ __forceinline__ Cell lattice_cell(const Dim& dm, int64_t place, W l, double u) {
    if (dm.kind == MPO_DIM_REAL) return Cell{u, 0};
    const int64_t k = digit<W>(dm, place, l);
    if (dm.kind == MPO_DIM_INTEGER) return Cell{dm.count == 0 ? 0.0 : (double)k / (double)dm.count, 0};
    return Cell{(double)k, (int)k};
}

__device__ __forceinline__ void store_cell(const Dim& dm, const Cell& c, double* __restrict__ p) {
    if (!one_hot(dm)) {
        *p = c.v;
        return;
    }
    const int n = (int)dm.count;
    for (int k = 0; k < n; ++k) p[k] = k == c.k ? 1.0 : 0.0;
}

// space_sample_kernel's items, order and stores; a discrete dimension takes its digit of
// lattice point (first + row) mod L where that kernel maps a draw, and the Philox block of a
// pair is computed only where the pair holds a Real (the same counter, so the same u).
template <class W>
__global__ __launch_bounds__(kBlock) void space_lattice_kernel(const DimTable t, const PlaceTable places,
                                                               const int n_dims, const int d, const uint32_t k0,
                                                               const uint32_t k1, const uint64_t first,
                                                               const int64_t m, const uint64_t L, const uint32_t sq,
                                                               const uint32_t sr, double* __restrict__ out) {
    const int n_pairs = (n_dims + 1) >> 1;
    const uint32_t gt = blockIdx.x * kBlock + threadIdx.x;
    int64_t row = gt / (uint32_t)n_pairs;
    int b = (int)(gt % (uint32_t)n_pairs);
    for (; row < m; ) {
        const uint64_t i = first + (uint64_t)row;
        const W l = (W)(i % L);
        const bool two = 2 * b + 1 < n_dims;
        const Dim d0 = t.c[2 * b];
        const Dim d1 = t.c[two ? 2 * b + 1 : 2 * b];
        double u0 = 0.0, u1 = 0.0;
        if (d0.kind == MPO_DIM_REAL || d1.kind == MPO_DIM_REAL) {
            uint32_t r[4];
            philox4x32_10(k0, k1, (uint32_t)i, (uint32_t)(i >> 32), (uint32_t)b, 0u, r);
            u0 = u53(r[0], r[1]);
            u1 = u53(r[2], r[3]);
        }
        const Cell c0 = lattice_cell<W>(d0, places.p[2 * b], l, u0);
        double* __restrict__ p = out + row * d + d0.col;
        if (two) {
            const Cell c1 = lattice_cell<W>(d1, places.p[2 * b + 1], l, u1);
            if (!one_hot(d0) && !one_hot(d1)) {
                if (((uintptr_t)p & 15) == 0) {
                    *reinterpret_cast<double2*>(p) = make_double2(c0.v, c1.v);
                } else {
                    p[0] = c0.v;
                    p[1] = c1.v;
                }
            } else {
                store_cell(d0, c0, p);
                store_cell(d1, c1, out + row * d + d1.col);
            }
        } else {
            store_cell(d0, c0, p);
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
    DimTable t{};
    if (const int rc = check_dims("mpo_space_sample", dims, n_dims, &d, t)) return rc;
    if (const int rc = check_rows("mpo_space_sample", first, m)) return rc;
    if (m == 0) return MPO_OK;
    if (const int rc = check_out("mpo_space_sample", m, out)) return rc;
    const int n_pairs = (n_dims + 1) / 2;
    const unsigned blocks = item_blocks(m, n_pairs);
    const uint32_t stride = blocks * kBlock;
    hipLaunchKernelGGL(space_sample_kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), t,
                       n_dims, d, (uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)first, m,
                       stride / (uint32_t)n_pairs, stride % (uint32_t)n_pairs, out);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}

extern "C" int mpo_space_lattice_size(const MpoDimDesc* dims, int n_dims, int64_t* L) {
    MPO_GUARD_BEGIN
    MPO_CHECK_ARG(L, "mpo_space_lattice_size: null result");
    DimTable t{};
    if (const int rc = check_dims("mpo_space_lattice_size", dims, n_dims, nullptr, t)) return rc;
    return lattice_places("mpo_space_lattice_size", dims, n_dims, nullptr, L);
    MPO_GUARD_END
}

extern "C" int mpo_space_lattice(const MpoDimDesc* dims, int n_dims, int d, uint64_t seed, int64_t first, int64_t m,
                                 double* out, void* stream) {
    MPO_GUARD_BEGIN
    DimTable t{};
    if (const int rc = check_dims("mpo_space_lattice", dims, n_dims, &d, t)) return rc;
    if (const int rc = check_rows("mpo_space_lattice", first, m)) return rc;
    PlaceTable places{};
    int64_t L = 1;
    if (const int rc = lattice_places("mpo_space_lattice", dims, n_dims, &places, &L)) return rc;
    if (m == 0) return MPO_OK;
    if (const int rc = check_out("mpo_space_lattice", m, out)) return rc;
    const int n_pairs = (n_dims + 1) / 2;
    const unsigned blocks = item_blocks(m, n_pairs);
    const uint32_t stride = blocks * kBlock;
    auto kernel = L < ((int64_t)1 << 32) ? space_lattice_kernel<uint32_t> : space_lattice_kernel<uint64_t>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), t, places, n_dims, d,
                       (uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)first, m, (uint64_t)L,
                       stride / (uint32_t)n_pairs, stride % (uint32_t)n_pairs, out);
    MPO_LAUNCH_CHECK();
    return MPO_OK;
    MPO_GUARD_END
}
