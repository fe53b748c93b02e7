// Internal helpers shared by the libmpo.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <utility>

#include "../../include/mpo.h"

namespace mpo {

// Thread-local message of the last failure (returned by mpo_last_error()).
void set_error(const char* fmt, ...);
void clear_error();

// The most observations a GP may hold: the refit (gp_fit.hip) and the posterior /
// scoring entry points (gp.hip) refuse more with MPO_ENOTSUP.
constexpr int kMaxObs = 2048;

constexpr double kSqrt5 = 2.236067977499789696409173668731276235;

// LDS a workgroup may use (gfx950: 160 KiB per CU)
constexpr size_t kMaxLds = 160 * 1024;

// sklearn kernels.py:1715-1724 (nu = 2.5) times ConstantKernel: the factorisation's and the
// joint posterior's Matern (gp.hip, gp_joint.hip).
__device__ __forceinline__ double matern52(double r, double amp) {
    // k^2 / 3 as a multiply by the rounded 1/3: within 1 ulp of sklearn's division,
    // and an fp64 divide costs ~10 VALU ops per candidate-observation pair
    const double k = r * kSqrt5;
    return amp * ((1.0 + k + k * k * (1.0 / 3.0)) * exp(-k));
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Carve consecutive 256-B aligned regions out of a caller workspace.
struct WsCarver {
    char* base;
    size_t used = 0;
    explicit WsCarver(void* p) : base(static_cast<char*>(p)) {}
    template <class T>
    T* take(size_t count) {
        used = align_up(used, 256);
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += count * sizeof(T);
        return p;
    }
};

// Makes the device a stream belongs to current for the scope of an entry point
// and restores the caller's afterwards: entry points that query or configure the
// device (hipFuncSetAttribute, attributes, pinned-pointer lookups) then target the
// stream's GPU whatever device the calling thread has current.
struct StreamDeviceScope {
    int prev = -1, dev = -1;
    explicit StreamDeviceScope(hipStream_t s) {
        if (s == nullptr || hipGetDevice(&prev) != hipSuccess || hipStreamGetDevice(s, &dev) != hipSuccess) {
            (void)hipGetLastError();
            prev = dev = -1;
            return;
        }
        if (dev != prev && hipSetDevice(dev) != hipSuccess) {
            (void)hipGetLastError();
            prev = dev = -1;
        }
    }
    ~StreamDeviceScope() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
    StreamDeviceScope(const StreamDeviceScope&) = delete;
    StreamDeviceScope& operator=(const StreamDeviceScope&) = delete;
};

// A second stream for independent launches of one step, on the caller's stream's
// device, forked from / joined into that stream with events (created on first use,
// re-created if the caller moves to another device).  get() returns nullptr when
// disabled or when the stream / events cannot be created (the step then runs
// serially on the caller's stream).
// The side streams themselves come from one process-wide pool per (device, caller
// stream, slot): every population engine stepped from the same caller stream shares
// them, so a process that holds several engines (a search: one per population,
// DenseNet and MNIST) keeps the same few streams -- with one pair of streams per
// engine, a 40-member engine stepped 15% slower while a second, idle engine was alive
// (6.53 vs 5.69 ms; 5.69 with pooled streams: profiles/r05/shard_ratio_probe.log).
// Engines stepped from DISTINCT caller streams get distinct side streams (r06), so a
// join never waits for another caller's work: the ABI's "thread-safe across streams"
// contract holds for them (tests/test_train_gpu.py::
// test_engines_on_two_threads_and_streams_keep_their_bits).  Engines sharing a caller
// stream are serialised by that stream anyway.  The fork / join events stay per engine.
inline hipStream_t pooled_side_stream(int dev, hipStream_t caller, int slot) {
    static std::mutex mu;
    static std::map<std::tuple<int, hipStream_t, int>, hipStream_t> pool;
    std::lock_guard<std::mutex> lk(mu);
    auto it = pool.find({dev, caller, slot});
    if (it != pool.end()) return it->second;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(dev);
    hipStream_t st = nullptr;
    const bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    (void)hipSetDevice(cur);
    if (!ok) { (void)hipGetLastError(); return nullptr; }
    pool[{dev, caller, slot}] = st;   // lives for the process
    return st;
}

struct SideStream {
    bool enabled = true;
    int slot = 0;   // which pooled stream (0: the side stream, 1: a third stream)
    hipStream_t side = nullptr;
    hipStream_t caller = nullptr;   // the caller stream `side` was pooled for
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int device = -1;
    SideStream() = default;
    explicit SideStream(int slot_) : slot(slot_) {}
    SideStream(const SideStream&) = delete;
    SideStream& operator=(const SideStream&) = delete;
    ~SideStream() { release(); }
    void release() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        side = nullptr;   // pooled: not destroyed
        caller = nullptr;
        ev_fork = ev_join = nullptr;
        device = -1;
    }
    hipStream_t get(hipStream_t s) {
        if (!enabled) return nullptr;
        int dev = 0;
        if (hipStreamGetDevice(s, &dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (side && dev == device) {
            if (s == caller) return side;
            side = pooled_side_stream(dev, s, slot);   // same device, another caller stream
            if (!side) { release(); enabled = false; return nullptr; }
            caller = s;
            return side;
        }
        release();
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(dev);
        side = pooled_side_stream(dev, s, slot);
        caller = s;
        const bool ok = side && hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) == hipSuccess;
        (void)hipSetDevice(cur);
        if (!ok) { (void)hipGetLastError(); release(); enabled = false; return nullptr; }
        device = dev;
        return side;
    }
    // s2 starts after everything enqueued on s so far
    hipError_t fork(hipStream_t s, hipStream_t s2) {
        if (hipError_t e = hipEventRecord(ev_fork, s)) return e;
        return hipStreamWaitEvent(s2, ev_fork, 0);
    }
    // s continues after everything enqueued on s2 so far
    hipError_t join(hipStream_t s, hipStream_t s2) {
        if (hipError_t e = hipEventRecord(ev_join, s2)) return e;
        return hipStreamWaitEvent(s, ev_join, 0);
    }
};

// The population engines' mpo_*_step_work walk the enqueue code of a train step with a
// tally set on their thread: every MPO_TALLY_LAUNCH adds its grid to the tally instead of
// running, so the figures cannot drift from what a step launches.  No HIP call is made
// while a tally is set: code on the walked path guards its other HIP calls with g_tally.
struct Tally {
    long long workgroups = 0, launches = 0;
};
inline thread_local Tally* g_tally = nullptr;

// hipGetLastError() after a launch that a tally may have counted instead
inline hipError_t tally_launch_error() { return g_tally ? hipSuccess : hipGetLastError(); }

// Static (compile-time) LDS bytes of a kernel, from its code object.
inline size_t static_lds_bytes(const void* kern) {
    hipFuncAttributes at{};
    if (hipFuncGetAttributes(&at, kern) != hipSuccess) {
        (void)hipGetLastError();
        return SIZE_MAX / 2;
    }
    return at.sharedSizeBytes;
}

// The device view of a pinned (hipHostMalloc / registered) host buffer, which a kernel reads
// and writes in place; nullptr when `h` is anything else.  The stream's device is current.
inline void* pinned_device_view(const void* h) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, h) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer) {
        (void)hipGetLastError();
        return nullptr;
    }
    return at.devicePointer;
}

// One pending L-BFGS-B round of one GP refit (gp_fit.hip): `batch` thetas of the
// problem (X, y, n) in the layout mpo_gp_lml_grad_host uses.  lml_launch_rounds
// evaluates the rounds of several refits in one launch set (same d, every n
// lml_groupable: the fused split sweep), enqueued on `s`, not synchronised.
struct LmlRound {
    const double* X;
    const double* y;
    int n, d, batch;
    double* theta_dev;         // [batch][d+2] device: the build's copy of theta_src
    const double* theta_src;   // [batch][d+2] pinned host, device view
    double* out;               // pinned host, device view: lml [batch] | grad [batch][d+2] | info
    double* ws;                // 256-B aligned, mpo_gp_lml_ws_bytes(n, d, batch)
};
bool lml_groupable(int n, int d);
int lml_launch_rounds(const LmlRound* r, int count, hipStream_t s);

// In-place lower blocked Cholesky (gp.hip: the bc_diag / bc_panel / bc_update steps of
// mpo_gp_prepare) of the padded row-major A [np][np], np a multiple of 32: reads the lower
// triangle and the full 32 x 32 diagonal blocks.  Dinv: np * 32 doubles of scratch.
// *info (device) = 0, or the first failed column + 1.  All sums in a fixed order.
hipError_t blocked_chol(double* A, int np, double* Dinv, int32_t* info, hipStream_t s);

// The scoring kernels' two-stage top-k merge (gp.hip: topk_merge_kernel) over nparts lists
// in the layout [part][3][k] (acquisition slots EI, PI, LCB; only those in `flags` are
// read), ties to the lowest index: out_idx / out_val [acq * k + r], index -1 where fewer
// than k entries exist.  mid_idx / mid_val: kTopkMergeGroups * 3 * k entries of scratch.
constexpr int kTopkMergeGroups = 256;
hipError_t topk_merge(const long long* part_idx, const double* part_val, int nparts, int k, unsigned flags,
                      long long* mid_idx, double* mid_val, long long* out_idx, double* out_val, hipStream_t s);

// The host-side refusals shared by every mpo_gp_committee_* entry point (gp_committee.hip) and
// mpo_gp_polish_committee_host (lbfgsb.cpp): MPO_OK, or MPO_EINVAL / MPO_ENOTSUP with the message
// set under `who` (null: a silent query).  Reads the host structs only.
int committee_models_ok(const char* who, const MpoGpModel* models, int E);

// The samplers' argmin fold (gp_paths.hip: argmin_fold_kernel; gp_joint.hip folds with it
// too): argmin[r] / minval[r] (either may be null) of draw r < n_draws from its nb
// workgroup partials part_val / part_idx [r * nb + b], folded in order, ties to the lowest
// index.
hipError_t argmin_fold(const double* part_val, const long long* part_idx, int n_draws, int nb, long long* argmin,
                       double* minval, hipStream_t s);

}  // namespace mpo

#define MPO_CHECK_ARG(cond, ...)              \
    do {                                      \
        if (!(cond)) {                        \
            ::mpo::set_error(__VA_ARGS__);    \
            return MPO_EINVAL;                \
        }                                     \
    } while (0)

#define MPO_HIP(call)                                                             \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) {                                                   \
            ::mpo::set_error("%s:%d %s: %s", __FILE__, __LINE__, #call,           \
                             hipGetErrorString(e_));                              \
            return MPO_EHIP;                                                      \
        }                                                                         \
    } while (0)

#define MPO_LAUNCH_CHECK() MPO_HIP(hipGetLastError())

// A kernel launch / launch check on a path that mpo_*_step_work walks (mpo::Tally)
#define MPO_TALLY_LAUNCH(kern, grid, block, lds, stream, ...)                    \
    do {                                                                         \
        if (::mpo::g_tally) {                                                    \
            const dim3 g_ = (grid);                                              \
            ::mpo::g_tally->workgroups += (long long)g_.x * g_.y * g_.z;         \
            ++::mpo::g_tally->launches;                                          \
        } else {                                                                 \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);     \
        }                                                                        \
    } while (0)
#define MPO_TALLY_LAUNCH_CHECK()                    \
    do {                                            \
        if (!::mpo::g_tally) MPO_LAUNCH_CHECK();    \
    } while (0)

#define MPO_GUARD_BEGIN try {
#define MPO_GUARD_END                                         \
    }                                                         \
    catch (...) {                                             \
        ::mpo::set_error("unexpected C++ exception");         \
        return MPO_EHIP;                                      \
    }

namespace mpo {

// One round of a polish objective on pinned host buffers (mpo_gp_acq_grad_host and its kin):
// makes the stream's device current, resolves x, ids, f, g and the optional `extra` to the
// device views a kernel reads and writes in place, runs launch(xd, idd, fd, gd, extrad) --
// the objective's own host-side checks and its enqueue -- and synchronises the stream.
template <class Launch>
int pinned_round(const char* who, void* stream, const double* x, const int32_t* ids, double* f, double* g,
                 double* extra, Launch&& launch) {
    StreamDeviceScope on_device(static_cast<hipStream_t>(stream));
    void* xd = pinned_device_view(x);
    void* id = pinned_device_view(ids);
    void* fd = pinned_device_view(f);
    void* gd = pinned_device_view(g);
    void* ed = extra ? pinned_device_view(extra) : nullptr;
    MPO_CHECK_ARG(xd && id && fd && gd && (ed || !extra), "%s: buffers must be pinned host memory", who);
    const int rc = launch(static_cast<const double*>(xd), static_cast<const int32_t*>(id), static_cast<double*>(fd),
                          static_cast<double*>(gd), static_cast<double*>(ed));
    if (rc != MPO_OK) return rc;
    MPO_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return MPO_OK;
}

}  // namespace mpo
