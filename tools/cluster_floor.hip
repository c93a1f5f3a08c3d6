// Dev tool: the floor k_cluster_insert (csrc/yabpe_cluster_kernels.h) is held against -- what a stream of random 4-byte
// atomicMin reaches on this device.  One thread per entry does exactly one atomicMin at a hashed slot of a u32 table of
// 2^slots_log2 slots (the hash of cl_home: the high bits of mix(i * G)); nothing else is read or written.  Best of `reps`
// launches after a warm-up, HIP events; one JSON line.  tools/cluster_bench.py builds and runs it in the same run.
//   hipcc --offload-arch=gfx950 -O3 -o tools/cluster_floor tools/cluster_floor.hip && ./tools/cluster_floor 27 64000000 [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>

__device__ __forceinline__ unsigned long long mix(unsigned long long x) {  // splitmix64's finaliser (enc_mix of encode_logic.h)
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void k_fill(unsigned int *tab, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) tab[i] = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_floor(unsigned int *tab, unsigned int slots_log2, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long slot = mix((i + 1) * 0x9E3779B97F4A7C15ull) >> (64 - slots_log2);  // (< 2^slots_log2: inside tab)
    atomicMin(&tab[slot], (unsigned int)i);
}

#define CHECK(x)                                                                   \
    do {                                                                           \
        hipError_t e__ = (x);                                                      \
        if (e__ != hipSuccess) {                                                   \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__));               \
            return 1;                                                              \
        }                                                                          \
    } while (0)

int main(int argc, char **argv) {
    const unsigned int lg = argc > 1 ? (unsigned int)atoi(argv[1]) : 27;
    const unsigned long long n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 64000000ull;
    const int reps = argc > 3 ? atoi(argv[3]) : 5;
    if (lg < 10 || lg > 31 || n == 0 || n > (1ull << 30) || reps < 1) {
        fprintf(stderr, "usage: cluster_floor slots_log2[10..31] entries[1..2^30] [reps]\n");
        return 2;
    }
    const unsigned long long slots = 1ull << lg;
    unsigned int *tab = nullptr;
    CHECK(hipMalloc(&tab, slots * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int r = 0; r <= reps; ++r) {  // (the first one is the warm-up)
        hipLaunchKernelGGL(k_fill, dim3((unsigned int)((slots + 255) / 256)), dim3(256), 0, 0, tab, slots);
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_floor, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, 0, tab, lg, n);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipDeviceSynchronize());
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r) best = std::min(best, ms);
    }
    printf("{\"slots_log2\": %u, \"entries\": %llu, \"atomic_min_ms\": %.4f, \"G_atomics_per_s\": %.3f}\n", lg, n, best, n / best / 1e6);
    CHECK(hipFree(tab));
    return 0;
}
