// The fp64 matrix rate of one MI355X by a calibration loop of v_mfma_f64_16x16x4_f64 (2048 FLOP each): 1024 workgroups x 4 waves, every
// wave runs a stream of MFMAs on 8 independent accumulators.  Prints one JSON line: TFLOP/s by HIP events for 4 and 8 waves per workgroup.
// scripts/prof_moments.py runs the program when it has been built (DESIGN finding 73):
//   hipcc --offload-arch=gfx950 -O3 scripts/micro/mfma_f64_rate.hip -o scripts/micro/mfma_f64_rate && scripts/micro/mfma_f64_rate
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void k(double* out, int iters) {
    const double a = 1.0 + threadIdx.x % 3, b = 1.0 / (1.0 + threadIdx.x % 5);
    f64x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}
int main() {
    const int blocks = 1024, iters = 4000;
    double* out;
    if (hipMalloc(&out, (size_t)blocks * 512 * 8) != hipSuccess) return 1;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    double tf[2] = {0.0, 0.0};
    for (int v = 0; v < 2; ++v) {
        const int waves = v ? 8 : 4;
        hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * waves), 0, 0, out, 50);
        if (hipDeviceSynchronize() != hipSuccess) return 1;
        hipEventRecord(e0); hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * waves), 0, 0, out, iters); hipEventRecord(e1);
        if (hipDeviceSynchronize() != hipSuccess) return 1;
        float ms = 0; hipEventElapsedTime(&ms, e0, e1);
        tf[v] = (double)blocks * waves * iters * 8 * 2048.0 / ms / 1e9;
    }
    printf("{\"instruction\": \"v_mfma_f64_16x16x4_f64\", \"tflops_4_waves\": %.2f, \"tflops_8_waves\": %.2f}\n", tf[0], tf[1]);
    return 0;
}
