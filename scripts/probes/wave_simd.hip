// Micro-probe: where do the waves of the GP scoring kernel's workgroups land?
// Launched with gp_score_kernel's geometry (256 threads, the flagship's dynamic LDS
// size, grid = resident capacity); every workgroup stays alive long enough for the
// whole grid to be resident at once.  Each wave records HW_ID and XCC_ID.
//   1. is wave index -> SIMD fixed (wave w of every workgroup on SIMD w)?
//   2. do the workgroups that share a CU differ in blockIdx.x & 3?  (gp_score_kernel
//      rotates per-wave shares by blockIdx.x; if a CU's workgroups share the low
//      bits, that rotation never moves a share off its SIMD.)
//   hipcc --offload-arch=gfx950 -O2 scripts/probes/wave_simd.hip -o scripts/probes/wave_simd
//   scripts/probes/wave_simd [lds_bytes = 30480] [blocks_per_cu = 0: from the occupancy query]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

__global__ __launch_bounds__(256) void probe(unsigned* out, long long spin) {
    extern __shared__ double smem[];
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    smem[threadIdx.x] = threadIdx.x;   // the dynamic LDS is really allocated
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < spin) __builtin_amdgcn_s_sleep(8);
    if ((threadIdx.x & 63) == 0) {
        const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6);
        out[2 * w] = hw;
        out[2 * w + 1] = xcc;
    }
}

int main(int argc, char** argv) {
    const int lds = argc > 1 ? atoi(argv[1]) : 30480;   // score_lds_bytes(12, 208): n = 200, dp = 12
    int per_cu = argc > 2 ? atoi(argv[2]) : 0;
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    hipFuncSetAttribute(reinterpret_cast<const void*>(probe), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (per_cu <= 0) hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, probe, 256, lds);
    const int grid = per_cu * cus;
    unsigned* out;
    hipMalloc(&out, (size_t)grid * 8 * sizeof(unsigned));
    std::vector<unsigned> h((size_t)grid * 8);
    for (int rep = 0; rep < 2; ++rep) {
        hipLaunchKernelGGL(probe, dim3(grid), dim3(256), lds, 0, out, 20000LL);   // 100 MHz clock: 200 us
        if (hipDeviceSynchronize() != hipSuccess) return 1;
    }
    hipMemcpy(h.data(), out, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
    printf("grid %d = %d per CU x %d CUs, %d B dynamic LDS\n", grid, per_cu, cus, lds);

    // HW_ID (gfx9): wave 3:0, SIMD 5:4, pipe 7:6, CU 11:8, SH 12, SE 15:13; XCC_ID 3:0
    long long ws[4][4] = {};
    std::map<unsigned, std::vector<int>> cu_blocks;        // (xcc, se, sh, cu) -> blocks
    std::map<unsigned, std::vector<int>> simd_waves;       // (xcc, se, sh, cu, simd) -> wave indices
    for (int b = 0; b < grid; ++b)
        for (int w = 0; w < 4; ++w) {
            const unsigned hw = h[2 * (b * 4 + w)], xcc = h[2 * (b * 4 + w) + 1] & 15;
            const unsigned simd = (hw >> 4) & 3, cu = ((hw >> 8) & 255) | (xcc << 8);
            ++ws[w][simd];
            if (w == 0) cu_blocks[cu].push_back(b);
            simd_waves[cu * 4 + simd].push_back(((b & 3) << 2) | w);
        }
    printf("wave index -> SIMD id (counts over all workgroups)\n");
    for (int w = 0; w < 4; ++w) printf("  wave %d: SIMD0 %lld  SIMD1 %lld  SIMD2 %lld  SIMD3 %lld\n", w, ws[w][0], ws[w][1], ws[w][2], ws[w][3]);

    std::map<int, int> per_cu_hist, distinct_hist;
    std::map<unsigned, int> xcc_of_b8;   // blockIdx & 7 -> mask of XCC ids seen
    for (auto& kv : cu_blocks) {
        ++per_cu_hist[(int)kv.second.size()];
        int mask = 0;
        for (int b : kv.second) {
            mask |= 1 << (b & 3);
            xcc_of_b8[b & 7] |= 1 << (kv.first >> 8);
        }
        ++distinct_hist[__builtin_popcount(mask)];
    }
    printf("CUs seen: %zu\n", cu_blocks.size());
    for (auto& kv : per_cu_hist) printf("  CUs holding %d workgroups: %d\n", kv.first, kv.second);
    for (auto& kv : distinct_hist) printf("  CUs whose workgroups show %d distinct blockIdx.x & 3: %d\n", kv.first, kv.second);
    for (auto& kv : xcc_of_b8) printf("  blockIdx.x & 7 = %u -> XCC mask 0x%02x\n", kv.first, kv.second);

    // waves per SIMD that carry share 0 (phase 1's extra block): by wave index, and by
    // (wave + blockIdx.x) & 3 (the rotation without a per-tile term)
    std::map<int, int> fixed_hist, rot_hist;
    for (auto& kv : simd_waves) {
        int fixed = 0, rot = 0;
        for (int v : kv.second) {
            fixed += (v & 3) == 0;
            rot += (((v & 3) + (v >> 2)) & 3) == 0;
        }
        ++fixed_hist[fixed];
        ++rot_hist[rot];
    }
    for (auto& kv : fixed_hist) printf("  SIMDs with %d waves of wave index 0: %d\n", kv.first, kv.second);
    for (auto& kv : rot_hist) printf("  SIMDs with %d waves of (wave + blockIdx.x) & 3 == 0: %d\n", kv.first, kv.second);
    const int cu0 = cu_blocks.begin()->first;
    printf("first CU (key 0x%x) blocks:", cu0);
    for (int b : cu_blocks.begin()->second) printf(" %d", b);
    printf("\n");
    return 0;
}
