// Design microbenchmark (gfx950), not part of the product: the histogram
// kernel (csrc/hh_hist_kern.h) as a function of its LDS copies per workgroup
// and of the persistent grid's workgroups per CU, on a file's bytes tiled to
// a given size (text is skewed: lanes that add to one counter serialise, and
// copies spread them).  Every configuration's counts are checked against the
// host's; the time is the median of 20 runs after 3 warm-ups (HIP events).
//
//   ub_hist FILE [MiB]      e.g.  build/ub_hist files/bible.txt 256
//
// Prints one line per configuration: copies, workgroups per CU, ms, GB/s.
// Build: hipcc -O3 --offload-arch=gfx950 -Ihuffmandecoderongpus_amd/csrc -o build/ub_hist tools/ubench/ub_hist.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hh_hist_kern.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <int COPIES>
static void launch(unsigned grid, const uint8_t *d, uint64_t n, uint32_t *slab, uint64_t *cnt) {
    hipLaunchKernelGGL(k_hist<COPIES>, dim3(grid), dim3(HIST_TB), 0, 0, d, n, slab);
    hipLaunchKernelGGL(k_hist_sum, dim3(HIST_SUM_WGS), dim3(HIST_SUM_TB), 0, 0, slab, grid, cnt);
}

static void launch_c(int copies, unsigned grid, const uint8_t *d, uint64_t n, uint32_t *slab, uint64_t *cnt) {
    switch (copies) {
    case 1: launch<1>(grid, d, n, slab, cnt); break;
    case 2: launch<2>(grid, d, n, slab, cnt); break;
    case 4: launch<4>(grid, d, n, slab, cnt); break;
    case 8: launch<8>(grid, d, n, slab, cnt); break;
    case 16: launch<16>(grid, d, n, slab, cnt); break;
    default: launch<32>(grid, d, n, slab, cnt); break;
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: ub_hist FILE [MiB]\n"); return 2; }
    const uint64_t n = (uint64_t)(argc > 2 ? atoi(argv[2]) : 256) << 20;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 1; }
    std::vector<uint8_t> text;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + got);
    fclose(f);
    if (text.empty()) { printf("%s is empty\n", argv[1]); return 1; }
    // the tiled input and its counts
    std::vector<uint8_t> h(n);
    for (uint64_t i = 0; i < n; i += text.size()) memcpy(&h[i], text.data(), std::min<uint64_t>(text.size(), n - i));
    uint64_t want[256] = {0};
    for (uint64_t i = 0; i < n; i++) want[h[i]]++;
    int cus = 0;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const unsigned max_grid = (unsigned)cus * 16u;
    uint8_t *d;
    uint32_t *slab;
    uint64_t *cnt;
    CK(hipMalloc(&d, n));
    CK(hipMalloc(&slab, (size_t)max_grid * 256 * 4));
    CK(hipMalloc(&cnt, 256 * 8));
    CK(hipMemcpy(d, h.data(), n, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("%s tiled to %llu MiB, %d CUs\ncopies wg/cu      ms    GB/s\n", argv[1], (unsigned long long)(n >> 20), cus);
    const int copies[] = {1, 2, 4, 8, 16, 32}, wpc[] = {2, 4, 8, 16};
    for (int c : copies)
        for (int w : wpc) {
            const unsigned grid = (unsigned)cus * (unsigned)w;
            std::vector<float> ms;
            for (int r = 0; r < 23; r++) {
                CK(hipEventRecord(e0, 0));
                launch_c(c, grid, d, n, slab, cnt);
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                float t;
                CK(hipEventElapsedTime(&t, e0, e1));
                if (r >= 3) ms.push_back(t);
            }
            uint64_t have[256];
            CK(hipMemcpy(have, cnt, sizeof have, hipMemcpyDeviceToHost));
            if (memcmp(have, want, sizeof have)) { printf("copies %d wg/cu %d: WRONG COUNTS\n", c, w); return 1; }
            std::sort(ms.begin(), ms.end());
            const float med = ms[ms.size() / 2];
            printf("%6d %5d %7.4f %7.1f\n", c, w, med, (double)n / med * 1e-6);
            fflush(stdout);
        }
    CK(hipFree(d));
    CK(hipFree(slab));
    CK(hipFree(cnt));
    return 0;
}
