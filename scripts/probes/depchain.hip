// Micro-probe: how fast does one wave get through DEPENDENT v_fma_f64 chains on gfx950,
// with 1, 2 or 4 independent chains interleaved, alone on its SIMD, among five VALU
// waves per SIMD, and beside waves that stream v_mfma_f64_16x16x4 on the same SIMD?
// (f64rate.hip measured eight independent chains only.)  The scoring kernel's Matern is
// ~31 fp64 instructions per value, nearly each reading its predecessor's result.
//
// Workgroups of 4 waves (one per SIMD) with 32 KB of LDS each, so five are resident per
// CU; block b is a VALU block when b % mod == 0 and an MFMA block otherwise (mod = 0:
// every block VALU).  Which blocks share a CU is the dispatcher's choice: mod = 5 gives
// one VALU wave among four MFMA waves per SIMD on average, and the spread over the VALU
// waves is printed.  Each wave times itself with the 100 MHz wall clock.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int CH>
__global__ __launch_bounds__(256) void probe(double* out, long long* ticks, int iters, int mfma_iters, int mod) {
    const int wave = threadIdx.x >> 6;
    const bool valu = mod == 0 || blockIdx.x % mod == 0;
    const double a = 1.0 + threadIdx.x * 1e-9, b = 0.999999 + blockIdx.x * 1e-12;
    const long long t0 = wall_clock64();
    double r = 0.0;
    if (valu) {
        double v[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) v[j] = a + j;
        for (int i = 0; i < iters; ++i) {
#pragma unroll
            for (int u = 0; u < 32 / CH; ++u) {
#pragma unroll
                for (int j = 0; j < CH; ++j) v[j] = fma(v[j], b, 1e-9);   // 32 v_fma_f64 per iteration, CH chains
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) r += v[j];
    } else {
        f64x4 c0 = {0, 0, 0, 0}, c1 = c0;
        for (int i = 0; i < mfma_iters; ++i) {
            c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);
        }
        r = c0[0] + c1[1];
    }
    const long long t1 = wall_clock64();
    out[blockIdx.x * 256 + threadIdx.x] = r;
    if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * 4 + wave] = t1 - t0;
}

template <int CH>
void run(const char* what, int grid, int mod, double* out, long long* ticks, double cyc_per_tick) {
    const int iters = 4096, mfma_iters = 40000;
    for (int rep = 0; rep < 2; ++rep)
        hipLaunchKernelGGL(probe<CH>, dim3(grid), dim3(256), 32768, 0, out, ticks, iters, mfma_iters, mod);
    hipDeviceSynchronize();
    std::vector<long long> h(grid * 4);
    hipMemcpy(h.data(), ticks, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> v, m;
    for (int b = 0; b < grid; ++b)
        for (int w = 0; w < 4; ++w) ((mod == 0 || b % mod == 0) ? v : m).push_back((double)h[b * 4 + w]);
    std::sort(v.begin(), v.end());
    const double per = cyc_per_tick / (iters * 32.0);
    double mm = 0;
    for (double x : m) mm += x;
    printf("%-34s chains %d: cycles per v_fma_f64 of a VALU wave: median %.2f  min %.2f  max %.2f", what, CH,
           v[v.size() / 2] * per, v.front() * per, v.back() * per);
    if (!m.empty()) printf("   (MFMA waves: %.1f cycles per MFMA on average)", mm / m.size() * cyc_per_tick / (2.0 * mfma_iters));
    printf("\n");
}

int main() {
    int dev, cus, clk;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, dev);   // kHz
    const double cyc_per_tick = clk * 1e3 / 100e6;                   // wall_clock64 ticks at 100 MHz
    const int gmax = 5 * cus;
    double* out;
    long long* ticks;
    hipMalloc(&out, (size_t)gmax * 256 * 8);
    hipMalloc(&ticks, (size_t)gmax * 4 * 8);
    hipFuncSetAttribute(reinterpret_cast<const void*>(probe<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 32768);
    hipFuncSetAttribute(reinterpret_cast<const void*>(probe<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 32768);
    hipFuncSetAttribute(reinterpret_cast<const void*>(probe<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 32768);
    printf("%d CUs, %d MHz nominal\n", cus, clk / 1000);
#define ALL(WHAT, GRID, MOD)                                  \
    run<1>(WHAT, GRID, MOD, out, ticks, cyc_per_tick);        \
    run<2>(WHAT, GRID, MOD, out, ticks, cyc_per_tick);        \
    run<4>(WHAT, GRID, MOD, out, ticks, cyc_per_tick);
    ALL("1 wave/SIMD, VALU only", cus, 0)
    ALL("5 waves/SIMD, VALU only", gmax, 0)
    ALL("2 waves/SIMD, 1 VALU + 1 MFMA", 2 * cus, 2)
    ALL("5 waves/SIMD, 1 VALU + 4 MFMA", gmax, 5)
    return 0;
}
