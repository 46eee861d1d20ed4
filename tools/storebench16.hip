// tools/storebench16.hip - the store shape of the 16-bit observations (obs_dtype bfloat16 / float16): K2's grid (4, N) x 256
// threads, each workgroup one frame of 84 x 84 16-bit values (14,112 B), written through a buffer resource exactly as the
// product writes (store_obs, agx_k2_fixed.h).  Variants: 8 B per lane lane-linear (the product's form: one float4 of f32 outputs
// becomes 8 B) and 16 B per lane (8 outputs per lane, 882 groups per frame), each with the agent-scope write-through bit (sc1,
// aux 16) and plain; the f32 frame (28,224 B, 16 B per lane, sc1) as the reference.  Each variant writes the same buffer R times
// back to back (HIP events around the R launches).  The buffer-resource size is the frame: nothing outside it is written.
// build: hipcc --offload-arch=gfx950 -O3 tools/storebench16.hip -o tools/storebench16 ; run: tools/storebench16 [N]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// BYTES per lane per store (8 | 16), FRAME bytes per workgroup, AUX cache-policy bits (0 plain, 16 sc1)
template <int BYTES, int FRAME, int AUX>
__global__ __launch_bounds__(256) void k_frame(char *out, unsigned seed) {
    char *frame = out + ((size_t)blockIdx.y * 4 + blockIdx.x) * FRAME;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(frame, 0, FRAME, 0x00027000);
    constexpr int n = FRAME / BYTES;
    for (int q = threadIdx.x; q < n; q += 256) {
        unsigned x = ((unsigned)q * 2654435761u) ^ seed ^ (blockIdx.y << 8);
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15;
        if (BYTES == 8) {
            const u2v w = {x & 0x3f7f3f7fu, (x >> 3) & 0x3f7f3f7fu};
            __builtin_amdgcn_raw_buffer_store_b64(w, rs, q * 8, 0, AUX);
        } else {
            const u4v w = {x & 0x3f7f3f7fu, (x >> 3) & 0x3f7f3f7fu, (x >> 5) & 0x3f7f3f7fu, (x >> 7) & 0x3f7f3f7fu};
            __builtin_amdgcn_raw_buffer_store_b128(w, rs, q * 16, 0, AUX);
        }
    }
}

template <class F>
static float timeit(F launch, int R) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int r = 0; r < 5; ++r) launch(r);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int r = 0; r < R; ++r) launch(r);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return ms / R * 1e3f;
}

int main(int argc, char **argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 1024, R = 200;
    constexpr int F16 = 84 * 84 * 2, F32 = 84 * 84 * 4;
    char *buf;
    CK(hipMalloc(&buf, (size_t)N * 4 * F32));
    const dim3 grid(4, N), block(256);
    struct V { const char *name; int frame; float us; } v[5] = {
        {"16-bit  8 B/lane sc1  (product)", F16, 0}, {"16-bit  8 B/lane plain", F16, 0},
        {"16-bit 16 B/lane sc1", F16, 0}, {"16-bit 16 B/lane plain", F16, 0}, {"f32    16 B/lane sc1  (product)", F32, 0}};
    for (int rep = 0; rep < 3; ++rep) {      // interleaved repetitions, best of 3
        float t[5];
        t[0] = timeit([&](int r) { hipLaunchKernelGGL((k_frame<8, F16, 16>), grid, block, 0, 0, buf, (unsigned)r); }, R);
        t[1] = timeit([&](int r) { hipLaunchKernelGGL((k_frame<8, F16, 0>), grid, block, 0, 0, buf, (unsigned)r); }, R);
        t[2] = timeit([&](int r) { hipLaunchKernelGGL((k_frame<16, F16, 16>), grid, block, 0, 0, buf, (unsigned)r); }, R);
        t[3] = timeit([&](int r) { hipLaunchKernelGGL((k_frame<16, F16, 0>), grid, block, 0, 0, buf, (unsigned)r); }, R);
        t[4] = timeit([&](int r) { hipLaunchKernelGGL((k_frame<16, F32, 16>), grid, block, 0, 0, buf, (unsigned)r); }, R);
        CK(hipGetLastError());
        for (int i = 0; i < 5; ++i) v[i].us = rep == 0 ? t[i] : (t[i] < v[i].us ? t[i] : v[i].us);
    }
    printf("N = %d, grid (4, N) x 256, one frame per workgroup, best of 3 x %d back-to-back launches\n", N, R);
    for (auto &x : v) {
        const double bytes = (double)N * 4 * x.frame;
        printf("  %-34s %8.2f us  %6.1f MB  %5.2f TB/s\n", x.name, x.us, bytes / 1e6, bytes / (x.us * 1e-6) / 1e12);
    }
    CK(hipFree(buf));
    return 0;
}
