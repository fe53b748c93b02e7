// gp_pd.hip -- partial dependence of a prepared GP's posterior mean (gfx950, fp64 VALU):
// mpo_gp_partial_dependence, mpo_gp_pd_ws_bytes.
//
// For a task with column spans a (and b), grid values ga < a.count (gb < b.count) and the
// S sample rows, cell (ga, gb) is
//   pd = y_mean + y_std (amp / S) sum_i alpha_i sum_s m52( sqrt(rest[s][i] + A[ga][i] + B[gb][i]) )
//   rest[s][i] = sum_{k outside the spans} (samples[s][k] / ls_k - xs[i][k])^2
//   A[ga][i]   = sum_{k in a} (grid_a[ga][k] / ls_k - xs[i][k])^2,   B likewise
// with m52(r) = (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r): the mean over the samples of the
// posterior mean at the sample with the spans' columns overwritten (skopt
// plots.partial_dependence_1D / _2D).  Every part is a sum of squares of direct
// differences; nothing is subtracted.
//
//   pd_scale_kernel  cs[s][k] = samples[s][k] / ls_k                          (workspace)
//   pd_cells_kernel  workgroup (task, tile of 256 cells, sample split, observation split):
//                    one thread per cell; the rest / A / B tiles of 64 samples x 32
//                    observations are built in the LDS and the cell's sum over them goes to
//                    part[task][split][cell]                                   (workspace)
//   pd_fold_kernel   the splits of a cell folded in order, then the affine finish
// The splits are functions of (S, n) alone and a task's partials live in its own range, so
// a task's bits depend on the model, the samples and that task only.  No atomics.
#include "mpo_internal.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int kSc = 64;        // samples per LDS tile
constexpr int kNi = 32;        // observations per LDS tile
constexpr int kCells = 256;    // cells per workgroup: one per thread
constexpr int kMaxSSplit = 8;  // sample splits of a task (each a run of whole tiles)
constexpr int kMaxISplit = 4;  // observation splits
constexpr int kIRun = 256;     // observations a workgroup takes before a second split is made
constexpr int kLaunchTasks = 48;

struct PdDevTask {
    MpoPdTask t;
    int64_t part_off;   // doubles into the partials
};
struct PdBatch {
    PdDevTask task[kLaunchTasks];
};
static_assert(sizeof(PdBatch) <= 3200, "the task batch travels as a kernel argument");

// how many splits, and the tiles each takes: functions of the extent alone
inline int tiles_of(int extent, int tile) { return (extent + tile - 1) / tile; }
inline int s_splits(int S) { return std::min(tiles_of(S, kSc), kMaxSSplit); }
inline int i_splits(int n) { return std::min(tiles_of(n, kIRun), kMaxISplit); }

__device__ __forceinline__ double m52(double r2) {
    const double k = sqrt(r2) * mpo::kSqrt5;
    return (1.0 + k + k * k * (1.0 / 3.0)) * exp(-k);
}

__global__ __launch_bounds__(256) void pd_scale_kernel(const double* __restrict__ samples, int S, int d,
                                                       const double* __restrict__ ls, double* __restrict__ cs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < S * d) cs[e] = samples[e] / ls[e % d];
}

// One axis tile: dst[il][g] = sum_{k in span} (grid[g][k - col] / ls_k - xs[i0 + il][k])^2, zeros for
// an absent axis (count is then taken as 1 by the caller).
__device__ __forceinline__ void axis_tile(const MpoPdAxis& ax, int count, const double* __restrict__ grid,
                                          const double* __restrict__ ls, const double* __restrict__ xs, int dp,
                                          int i0, int ni, double* dst) {
    for (int e = threadIdx.x; e < ni * count; e += 256) {
        const int il = e / count, g = e % count;
        double v = 0.0;
        for (int k = 0; k < ax.width; ++k) {
            const int c = ax.col + k;
            const double t = grid[ax.grid_off + (int64_t)g * ax.width + k] / ls[c] - xs[(size_t)(i0 + il) * dp + c];
            v += t * t;
        }
        dst[il * 64 + g] = v;
    }
}

__global__ __launch_bounds__(256) void pd_cells_kernel(PdBatch batch, const double* __restrict__ cs,
                                                       int S, int d, int dp, int n,
                                                       const double* __restrict__ xs, const double* __restrict__ ls,
                                                       const double* __restrict__ alpha,
                                                       const double* __restrict__ grid, double* __restrict__ part) {
    __shared__ double rest[kNi * kSc];   // [il][sl]
    __shared__ double At[kNi * 64];      // [il][ga]
    __shared__ double Bt[kNi * 64];      // [il][gb]
    const PdDevTask& dt = batch.task[blockIdx.y];
    const MpoPdAxis a = dt.t.a, b = dt.t.b;
    const int gb_n = b.width > 0 ? b.count : 1;
    const int cells = a.count * gb_n;
    const int ns = min((S + kSc - 1) / kSc, kMaxSSplit), ni_s = min((n + kIRun - 1) / kIRun, kMaxISplit);
    const int nsplit = ns * ni_s;
    const int tile = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
    if (tile * kCells >= cells) return;   // uniform: the grid is sized for the batch's largest task
    const int ss = split / ni_s, is = split % ni_s;
    // this workgroup's runs of whole tiles
    const int s_tiles = (S + kSc - 1) / kSc, i_tiles = (n + kNi - 1) / kNi;
    const int st0 = s_tiles * ss / ns, st1 = s_tiles * (ss + 1) / ns;        // <= 64 tiles x 8 splits
    const int it0 = i_tiles * is / ni_s, it1 = i_tiles * (is + 1) / ni_s;    // <= 64 tiles x 4 splits

    const int cell = tile * kCells + threadIdx.x;
    const bool live = cell < cells;
    const int ga = live ? cell / gb_n : 0, gb = live ? cell % gb_n : 0;
    const int a0 = a.col, a1 = a.col + a.width;
    const int b0 = b.width > 0 ? b.col : 0, b1 = b.width > 0 ? b.col + b.width : 0;

    double acc = 0.0;
    for (int it = it0; it < it1; ++it) {
        const int i0 = it * kNi, ni = min(kNi, n - i0);
        for (int st = st0; st < st1; ++st) {
            const int s0 = st * kSc, nsl = min(kSc, S - s0);
            __syncthreads();   // the previous tile's readers are done
            if (st == st0) {
                axis_tile(a, a.count, grid, ls, xs, dp, i0, ni, At);
                if (b.width > 0) axis_tile(b, b.count, grid, ls, xs, dp, i0, ni, Bt);
                else
                    for (int e = threadIdx.x; e < ni; e += 256) Bt[e * 64] = 0.0;
            }
            for (int e = threadIdx.x; e < ni * nsl; e += 256) {
                const int il = e / nsl, sl = e % nsl;
                const double* c = cs + (size_t)(s0 + sl) * d;
                const double* x = xs + (size_t)(i0 + il) * dp;
                double v = 0.0;
                for (int k = 0; k < d; ++k) {
                    if ((k >= a0 && k < a1) || (k >= b0 && k < b1)) continue;
                    const double t = c[k] - x[k];
                    v += t * t;
                }
                rest[il * kSc + sl] = v;
            }
            __syncthreads();
            if (live) {
                for (int il = 0; il < ni; ++il) {
                    const double ab = At[il * 64 + ga] + Bt[il * 64 + gb];
                    const double* r = rest + il * kSc;
                    double ksum = 0.0;
#pragma unroll 4
                    for (int sl = 0; sl < nsl; ++sl) ksum += m52(r[sl] + ab);
                    acc = fma(alpha[i0 + il], ksum, acc);
                }
            }
        }
    }
    if (live) part[dt.part_off + (int64_t)split * cells + cell] = acc;
}

__global__ __launch_bounds__(256) void pd_fold_kernel(PdBatch batch, int S, int n, double amp, double y_mean,
                                                      double y_std, const double* __restrict__ part,
                                                      double* __restrict__ out) {
    const PdDevTask& dt = batch.task[blockIdx.y];
    const int cells = dt.t.a.count * (dt.t.b.width > 0 ? dt.t.b.count : 1);
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const int nsplit = min((S + kSc - 1) / kSc, kMaxSSplit) * min((n + kIRun - 1) / kIRun, kMaxISplit);
    double sum = 0.0;
    for (int p = 0; p < nsplit; ++p) sum += part[dt.part_off + (int64_t)p * cells + cell];
    out[dt.t.out_off + cell] = y_mean + y_std * (amp * sum / (double)S);
}

inline int64_t task_cells(const MpoPdTask& t) { return (int64_t)t.a.count * (t.b.width > 0 ? t.b.count : 1); }

bool shape_ok(const MpoGpModel* md) {
    return md->n > 0 && md->d > 0 && md->d <= md->dp && md->dp <= 32 && md->dp % 4 == 0;
}

bool axis_ok(const char* who, int t, const char* name, const MpoPdAxis& ax, int d) {
    if (ax.width < 0 || ax.col < 0 || ax.col >= d || ax.width > d - ax.col) {
        if (who) mpo::set_error("%s: task %d axis %s: span [%d, %d + %d) outside [0, %d)", who, t, name, ax.col,
                                ax.col, ax.width, d);
        return false;
    }
    if (ax.count < 1 || ax.count > MPO_PD_GMAX) {
        if (who) mpo::set_error("%s: task %d axis %s: count=%d outside [1, %d]", who, t, name, ax.count, MPO_PD_GMAX);
        return false;
    }
    if (ax.grid_off < 0) {
        if (who) mpo::set_error("%s: task %d axis %s: negative grid offset", who, t, name);
        return false;
    }
    return true;
}

// Everything but the buffers and the workspace size: MPO_OK, or the status (message set when `who`).
int pd_check(const char* who, const MpoGpModel* model, int S, const MpoPdTask* tasks, int T) {
    auto bad = [&](const char* what) {
        if (who) mpo::set_error("%s: %s", who, what);
        return MPO_EINVAL;
    };
    if (!model || !tasks) return bad("null model/tasks");
    if (!shape_ok(model)) return bad("malformed model");
    if (!model->xs || !model->ls || !model->alpha) return bad("model not prepared");
    if (model->n > mpo::kMaxObs) {
        if (who) mpo::set_error("%s: n=%d outside the supported n <= %d", who, model->n, mpo::kMaxObs);
        return MPO_ENOTSUP;
    }
    if (S < 1 || S > MPO_PD_SMAX) return bad("S outside [1, MPO_PD_SMAX]");
    if (T < 1 || T > MPO_PD_TMAX) return bad("T outside [1, MPO_PD_TMAX]");
    const int d = model->d;
    std::vector<std::pair<int64_t, int64_t>> ranges;
    ranges.reserve(T);
    for (int t = 0; t < T; ++t) {
        const MpoPdTask& k = tasks[t];
        if (k.a.width == 0) {
            if (who) mpo::set_error("%s: task %d: the first axis is absent", who, t);
            return MPO_EINVAL;
        }
        if (!axis_ok(who, t, "a", k.a, d)) return MPO_EINVAL;
        if (k.b.width != 0) {
            if (!axis_ok(who, t, "b", k.b, d)) return MPO_EINVAL;
            if (k.a.col < k.b.col + k.b.width && k.b.col < k.a.col + k.a.width) {
                if (who) mpo::set_error("%s: task %d: spans a and b overlap", who, t);
                return MPO_EINVAL;
            }
        }
        if (k.out_off < 0) {
            if (who) mpo::set_error("%s: task %d: negative output offset", who, t);
            return MPO_EINVAL;
        }
        ranges.emplace_back(k.out_off, k.out_off + task_cells(k));
    }
    std::sort(ranges.begin(), ranges.end());
    for (int t = 1; t < T; ++t)
        if (ranges[t].first < ranges[t - 1].second) return bad("the output ranges of two tasks overlap");
    return MPO_OK;
}

struct PdWs {
    double* cs;     // [S][d]
    double* part;   // per task [splits][cells]
    size_t used;
};

PdWs carve_pd_ws(void* ws, const MpoGpModel* md, int S, const MpoPdTask* tasks, int T) {
    mpo::WsCarver c(ws);
    PdWs w{};
    w.cs = c.take<double>((size_t)S * md->d);
    const size_t nsplit = (size_t)s_splits(S) * i_splits(md->n);
    size_t cells = 0;
    for (int t = 0; t < T; ++t) cells += (size_t)task_cells(tasks[t]);
    w.part = c.take<double>(nsplit * cells);
    w.used = mpo::align_up(c.used, 256);
    return w;
}

}  // namespace

extern "C" {

size_t mpo_gp_pd_ws_bytes(const MpoGpModel* model, int S, const MpoPdTask* tasks_host, int T) {
    try {
        if (pd_check(nullptr, model, S, tasks_host, T) != MPO_OK) return 0;
        return carve_pd_ws(nullptr, model, S, tasks_host, T).used;
    } catch (...) {
        return 0;
    }
}

int mpo_gp_partial_dependence(const MpoGpModel* model, const double* samples, int S, const MpoPdTask* tasks_host,
                              int T, const double* grid, double* out, void* ws, size_t ws_bytes, void* stream) {
    MPO_GUARD_BEGIN
    const char* who = "mpo_gp_partial_dependence";
    if (const int rc = pd_check(who, model, S, tasks_host, T)) return rc;
    MPO_CHECK_ARG(samples && grid && out && ws, "%s: null samples/grid/out/workspace", who);
    const PdWs w = carve_pd_ws(ws, model, S, tasks_host, T);
    MPO_CHECK_ARG(ws_bytes >= w.used, "%s: workspace too small (%zu < %zu)", who, ws_bytes, w.used);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = model->n, d = model->d;
    const int nsplit = s_splits(S) * i_splits(n);
    hipLaunchKernelGGL(pd_scale_kernel, dim3((S * d + 255) / 256), dim3(256), 0, st, samples, S, d, model->ls, w.cs);
    MPO_LAUNCH_CHECK();
    int64_t part_off = 0;
    for (int t0 = 0; t0 < T; t0 += kLaunchTasks) {
        const int nt = std::min(kLaunchTasks, T - t0);
        PdBatch batch{};
        int64_t max_cells = 0;
        for (int j = 0; j < nt; ++j) {
            batch.task[j].t = tasks_host[t0 + j];
            batch.task[j].part_off = part_off;
            const int64_t cells = task_cells(tasks_host[t0 + j]);
            part_off += cells * nsplit;
            max_cells = std::max(max_cells, cells);
        }
        const int tiles = (int)((max_cells + kCells - 1) / kCells);
        hipLaunchKernelGGL(pd_cells_kernel, dim3(tiles * nsplit, nt), dim3(256), 0, st, batch, w.cs, S, d,
                           model->dp, n, model->xs, model->ls, model->alpha, grid, w.part);
        MPO_LAUNCH_CHECK();
        hipLaunchKernelGGL(pd_fold_kernel, dim3(tiles, nt), dim3(256), 0, st, batch, S, n, model->amp, model->y_mean,
                           model->y_std, w.part, out);
        MPO_LAUNCH_CHECK();
    }
    return MPO_OK;
    MPO_GUARD_END
}

}  // extern "C"
