// Interpolation-sampler kernels (include/mdm_interp.h): the clamped constant shift, the batch-shared row mask and the momentum
// write of the latent-interpolation reverse loop.  NCHW fp32 like the reference's tensors; pure HBM streaming: 256-thread
// workgroups, at most 2048 of them with a grid stride, 16 bytes per lane wherever the extents and the addresses allow it.
//
// Replaces reference scheduler.py:735-754 with :757-766 (shift), :553-557 (mask draw), sampler.py:326-333 (update).
#include "common.h"
#include "../../include/mdm_interp.h"

namespace mdm {

// Philox stream id of the row mask: ids 0-5 are listed in sched.hip; 6 is this file's and used nowhere else.
constexpr int INTERP_ROW_STREAM = 6;
constexpr int INTERP_MAX_GRID = 2048;

static inline int igrid(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > INTERP_MAX_GRID ? INTERP_MAX_GRID : b));
}
static inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// torch.clamp(v, lo, hi) = min(max(v, lo), hi) with NaN propagating from the value and from either bound (fmax / fmin drop a NaN)
__device__ __forceinline__ double clamp_nan(double v, double lo, double hi) {
    v = (lo != lo) ? lo : (v < lo ? lo : v);
    return (hi != hi) ? hi : (v > hi ? hi : v);
}
__device__ __forceinline__ float interp_shift_of(const float* mu, const double* ratio, float shift, int n) {
    const double rt = ratio[n], m = -(double)mu[n];
    const float sv = (float)((double)shift * rt);                     // scheduler.py:744-745: fp32 shift times fp64 ratio, one rounding
    return (float)clamp_nan((double)sv, m - rt, m + rt);             // :747-752: fp64 bounds, one rounding
}

// V = 4: one thread per four consecutive elements of one (n, c) plane (HW % 4 == 0); V = 1: one thread per element.
template <typename T, int V>
__global__ __launch_bounds__(256) void interp_shift_kernel(const float* x_t, const float* mu, const double* ratio, float shift, int C,
                                                           int HW, int64_t total, float* s_out, float* x_in, T* x_nhwc, int Cp) {
    const int64_t items = total / V;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = it * V;
        const int p = (int)(i % HW);
        const int64_t r = i / HW;
        const int c = (int)(r % C), n = (int)(r / C);
        const float sv = interp_shift_of(mu, ratio, shift, n);
        float xv[V];
        if constexpr (V == 4) {
            const float4 x = load4(x_t + i);
            xv[0] = x.x + sv; xv[1] = x.y + sv; xv[2] = x.z + sv; xv[3] = x.w + sv;
            if (s_out) store4(s_out + i, make_float4(sv, sv, sv, sv));
            if (x_in) store4(x_in + i, make_float4(xv[0], xv[1], xv[2], xv[3]));
        } else {
            xv[0] = x_t[i] + sv;
            if (s_out) s_out[i] = sv;
            if (x_in) x_in[i] = xv[0];
        }
        if (x_nhwc) {
            T* o = x_nhwc + ((int64_t)n * HW + p) * Cp + c;
#pragma unroll
            for (int k = 0; k < V; ++k) Elem<T>::st(o + (int64_t)k * Cp, xv[k]);
        }
    }
}

// grid.x walks the quads of the row, grid.y the samples: a thread makes the four uniforms of its quad ONCE (one Philox call, or one
// load of the caller's row) and thresholds them for every sample it visits, writing all C planes of that sample.
template <bool VEC>
__global__ __launch_bounds__(256) void interp_row_mask_kernel(const double* amount, const float* u_row, const uint64_t* rng, int N, int C,
                                                              int HW, float* mask) {
    const int quads = (HW + 3) >> 2;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const int p0 = q << 2;
        float u[4];
        if (u_row) {
            if (VEC) { const float4 v = load4(u_row + p0); u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w; }
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) u[k] = p0 + k < HW ? u_row[p0 + k] : 0.f;
            }
        } else {
            Philox ph(rng[0] & 0xFFFFFFFFull);       // the rank half of the key is dropped: one row for all shards of a batch
            const uint4 w = ph((uint64_t)q, rng[1] * 8 + (uint64_t)INTERP_ROW_STREAM);
            u[0] = u01(w.x); u[1] = u01(w.y); u[2] = u01(w.z); u[3] = u01(w.w);
        }
        for (int n = blockIdx.y; n < N; n += gridDim.y) {
            const double thr = amount[n];
            float k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = ((double)u[j] > thr) ? 1.f : 0.f;
            float* o = mask + (int64_t)n * C * HW + p0;
            for (int c = 0; c < C; ++c, o += HW) {
                if (VEC) store4(o, make_float4(k[0], k[1], k[2], k[3]));
                else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (p0 + j < HW) o[j] = k[j];
                }
            }
        }
    }
}

// VEC: four elements per thread over the first n / 4 * 4, the last n % 4 by the first lanes of workgroup 0.
template <bool VEC>
__global__ __launch_bounds__(256) void interp_update_kernel(const float* d_t, const float* d_next, float* x_t, float* diff, int update,
                                                            int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nv = VEC ? n >> 2 : 0;
    for (int64_t i = tid; i < nv; i += stride) {
        const float4 x = load4(x_t + 4 * i), d = load4(d_t + 4 * i);
        const float4 df = make_float4(x.x - d.x, x.y - d.y, x.z - d.z, x.w - d.w);
        store4(diff + 4 * i, df);
        if (update) {
            const float4 e = load4(d_next + 4 * i);
            store4(x_t + 4 * i, make_float4(e.x + df.x, e.y + df.y, e.z + df.z, e.w + df.w));
        }
    }
    for (int64_t i = 4 * nv + tid; i < n; i += stride) {
        const float df = x_t[i] - d_t[i];
        diff[i] = df;
        if (update) x_t[i] = d_next[i] + df;
    }
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_interp_shift(const float* x_t, const float* mu, const double* ratio, float shift, int N, int C, int H, int W,
                                float* s, float* x_in, int dtype, void* x_in_nhwc, int Cp, void* stream) {
    MDM_REQUIRE(x_t && mu && ratio, "interp_shift: x_t, mu and ratio are required");
    MDM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "interp_shift: N, C, H, W must be positive (%d, %d, %d, %d)", N, C, H, W);
    MDM_REQUIRE(C <= 8, "interp_shift: C = %d is more than 8", C);
    MDM_REQUIRE(dtype == MDM_F32 || dtype == MDM_BF16, "interp_shift: bad dtype %d", dtype);
    MDM_REQUIRE(!x_in_nhwc || (Cp >= C && Cp % 8 == 0), "interp_shift: Cp = %d must be a multiple of 8 and at least C", Cp);
    if (!s && !x_in && !x_in_nhwc) return 0;
    const int HW = H * W;
    const int64_t total = (int64_t)N * C * HW;
    const bool vec = HW % 4 == 0 && al16(x_t) && al16(s) && al16(x_in);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(igrid(vec ? total / 4 : total)), block(256);
#define MDM_INTERP_SHIFT(T, V) \
    hipLaunchKernelGGL((interp_shift_kernel<T, V>), grid, block, 0, st, x_t, mu, ratio, shift, C, HW, total, s, x_in, (T*)x_in_nhwc, Cp)
    if (dtype == MDM_BF16) { if (vec) MDM_INTERP_SHIFT(bf16_t, 4); else MDM_INTERP_SHIFT(bf16_t, 1); }
    else { if (vec) MDM_INTERP_SHIFT(float, 4); else MDM_INTERP_SHIFT(float, 1); }
#undef MDM_INTERP_SHIFT
    return launch_status("interp_shift");
}

extern "C" int mdm_interp_row_mask(const double* amount, const float* u_row, const uint64_t* rng, int N, int C, int HW, float* mask,
                                   void* stream) {
    MDM_REQUIRE(amount && mask, "interp_row_mask: amount and mask are required");
    MDM_REQUIRE(u_row || rng, "interp_row_mask: needs u_row or rng");
    MDM_REQUIRE(N > 0 && C > 0 && HW > 0, "interp_row_mask: N, C, HW must be positive (%d, %d, %d)", N, C, HW);
    MDM_REQUIRE(C <= 8, "interp_row_mask: C = %d is more than 8", C);
    const bool vec = HW % 4 == 0 && al16(mask) && al16(u_row);
    const int gx = igrid((HW + 3) / 4);
    const int gy = N < INTERP_MAX_GRID / gx ? N : INTERP_MAX_GRID / gx;          // gx <= INTERP_MAX_GRID, so at least 1
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(interp_row_mask_kernel<true>, dim3(gx, gy), dim3(256), 0, st, amount, u_row, rng, N, C, HW, mask);
    else hipLaunchKernelGGL(interp_row_mask_kernel<false>, dim3(gx, gy), dim3(256), 0, st, amount, u_row, rng, N, C, HW, mask);
    return launch_status("interp_row_mask");
}

extern "C" int mdm_interp_update(const float* d_t, const float* d_next, float* x_t, float* diff, int update, int64_t n, void* stream) {
    MDM_REQUIRE(d_t && x_t && diff, "interp_update: d_t, x_t and diff are required");
    MDM_REQUIRE(!update || d_next, "interp_update: update needs d_next");
    MDM_REQUIRE(n > 0, "interp_update: n must be positive");
    const bool vec = al16(d_t) && al16(x_t) && al16(diff) && al16(d_next);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(igrid(vec ? (n + 3) / 4 : n)), block(256);
    if (vec) hipLaunchKernelGGL(interp_update_kernel<true>, grid, block, 0, st, d_t, d_next, x_t, diff, update, n);
    else hipLaunchKernelGGL(interp_update_kernel<false>, grid, block, 0, st, d_t, d_next, x_t, diff, update, n);
    return launch_status("interp_update");
}
