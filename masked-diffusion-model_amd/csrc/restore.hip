// Restoration-sampler kernels (include/mdm_restore.h): the x0 reconstruction of a reverse step with the projection onto a
// measurement of group means (box-downsampled and / or grey), the measurement itself, and the start values of a run.  NCHW fp32;
// pure HBM streaming like inpaint.hip: 256-thread workgroups, at most 2048 of them with a grid stride (x0, measure) or one per
// image (start), 16 bytes per lane wherever the extents and the addresses allow it.
//
// Upstream has no counterpart.  The order of a group's sum is the header's: strips of min(k, 4) columns, each summed from +0 by
// sequential adds (channels, rows, columns), two strips of a k = 8 group added left + right.
#include "common.h"
#include "../../include/mdm_restore.h"

namespace mdm {

constexpr int RESTORE_MAX_GRID = 2048;
constexpr int RESTORE_GRAY_C = 4;             // channels a lane of the 16-byte gray route holds

static inline int rgrid(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > RESTORE_MAX_GRID ? RESTORE_MAX_GRID : b));
}
static inline bool ral16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The sums of the groups a strip of four columns meets: four groups of one column (K = 1), two of two (K = 2), one (K >= 4).
template <int K>
__device__ __forceinline__ void strip_add(float (&a)[4], const float4 v) {
    if constexpr (K == 1) { a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w; }
    else if constexpr (K == 2) { a[0] += v.x; a[0] += v.y; a[1] += v.z; a[1] += v.w; }
    else { a[0] += v.x; a[0] += v.y; a[0] += v.z; a[0] += v.w; }
}

// The 16-byte route.  One item = four consecutive columns of the K rows of one block row: a strip (K >= 4), two groups (K = 2)
// or four (K = 1, where the host passes the plane as one row of H W columns).  GRAY: the item spans all C <= 4 channels, else it
// lies in channel cg.  A lane keeps the item's x between the sum and the stores; the two strips of a K = 8 group sit in lanes
// 2 j and 2 j + 1 (the number of items of a row is even, and so are the workgroup size and the grid stride), which exchange their
// sums.  W4 = W / 4, Hk = H / K.
template <typename T, int K, bool GRAY>
__global__ __launch_bounds__(256) void restore_x0_kernel(const T* __restrict__ pred, int Cp, const float* __restrict__ x_in,
                                                         const float* __restrict__ s, const float* __restrict__ y, int C, int Hk, int W,
                                                         int64_t items, float* __restrict__ pred_nchw, float* __restrict__ shifted0,
                                                         float* __restrict__ x0_hat) {
    constexpr int CH = GRAY ? RESTORE_GRAY_C : 1;
    const int W4 = W >> 2, Cg = GRAY ? 1 : C, nch = GRAY ? C : 1;
    const int64_t HW = (int64_t)Hk * K * W;
    const float size = (float)(K * K * nch);
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        const int x4 = (int)(it % W4);
        int64_t t = it / W4;
        const int by = (int)(t % Hk);
        t /= Hk;
        const int cg = (int)(t % Cg);
        const int64_t n = t / Cg;
        float4 xv[CH][K];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) {
            if (cc < nch) {
                const int c = GRAY ? cc : cg;
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int64_t p = (int64_t)(by * K + r) * W + 4 * x4;
                    const int64_t i = (n * C + c) * HW + p;
                    const T* pp = pred + (n * HW + p) * Cp + c;
                    const float4 a = load4(x_in + i);
                    const float4 pv = make_float4(Elem<T>::ld(pp), Elem<T>::ld(pp + Cp), Elem<T>::ld(pp + 2 * (int64_t)Cp),
                                                  Elem<T>::ld(pp + 3 * (int64_t)Cp));
                    const float4 sh = make_float4(a.x + pv.x, a.y + pv.y, a.z + pv.z, a.w + pv.w);
                    float4 x = sh;
                    if (s) {
                        const float4 z = load4(s + i);
                        x = make_float4(sh.x - z.x, sh.y - z.y, sh.z - z.z, sh.w - z.w);
                    }
                    if (pred_nchw) store4(pred_nchw + i, pv);
                    if (shifted0) store4(shifted0 + i, sh);
                    xv[cc][r] = x;
                    strip_add<K>(acc, x);
                }
            }
        }
        float d[4];
        if constexpr (K == 1) {
            const float4 yv = load4(y + n * HW + 4 * x4);
            d[0] = yv.x - acc[0] / size; d[1] = yv.y - acc[1] / size; d[2] = yv.z - acc[2] / size; d[3] = yv.w - acc[3] / size;
        } else if constexpr (K == 2) {
            const float* yp = y + ((n * Cg + cg) * Hk + by) * (int64_t)(W >> 1) + 2 * x4;
            d[0] = d[1] = yp[0] - acc[0] / size;
            d[2] = d[3] = yp[1] - acc[1] / size;
        } else {
            float tot = acc[0];
            if constexpr (K == 8) tot += __shfl_xor(tot, 1, 64);               // left + right: the same bits in both lanes
            const float yv = y[((n * Cg + cg) * Hk + by) * (int64_t)(W / K) + (K == 8 ? x4 >> 1 : x4)];
            d[0] = d[1] = d[2] = d[3] = yv - tot / size;
        }
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) {
            if (cc < nch) {
                const int c = GRAY ? cc : cg;
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int64_t i = (n * C + c) * HW + (int64_t)(by * K + r) * W + 4 * x4;
                    const float4 x = xv[cc][r];
                    store4(x0_hat + i, make_float4(x.x + d[0], x.y + d[1], x.z + d[2], x.w + d[3]));
                }
            }
        }
    }
}

// The scalar route: one lane per group.  `out` false: the walk that forms the sum (and writes the unprojected outputs); true: the
// walk that forms x again, the same operations on the same operands, and stores x + d.
template <typename T, bool OUT>
__device__ __forceinline__ float restore_walk(const T* pred, int Cp, const float* x_in, const float* s, int64_t n, int C, int c0, int nch,
                                              int k, int H, int W, int y0, int x0, float d, float* pred_nchw, float* shifted0,
                                              float* x0_hat) {
    const int sw = k < 4 ? k : 4;
    const int64_t HW = (int64_t)H * W;
    float tot = 0.f;
    for (int st = 0; st < k / sw; ++st) {
        float sum = 0.f;
        for (int cc = 0; cc < nch; ++cc)
            for (int r = 0; r < k; ++r)
                for (int j = 0; j < sw; ++j) {
                    const int64_t p = (int64_t)(y0 + r) * W + x0 + st * sw + j;
                    const int64_t i = (n * C + c0 + cc) * HW + p;
                    const float pv = Elem<T>::ld(pred + (n * HW + p) * Cp + c0 + cc);
                    const float sh = x_in[i] + pv;
                    const float x = s ? sh - s[i] : sh;
                    if constexpr (OUT) x0_hat[i] = x + d;
                    else {
                        if (pred_nchw) pred_nchw[i] = pv;
                        if (shifted0) shifted0[i] = sh;
                        sum += x;
                    }
                }
        tot = st == 0 ? sum : tot + sum;
    }
    return tot;
}

template <typename T>
__global__ __launch_bounds__(256) void restore_x0_scalar_kernel(const T* pred, int Cp, const float* x_in, const float* s, const float* y,
                                                                int k, int gray, int C, int H, int W, int64_t groups, float* pred_nchw,
                                                                float* shifted0, float* x0_hat) {
    const int Hk = H / k, Wk = W / k, Cg = gray ? 1 : C, nch = gray ? C : 1;
    const float size = (float)(k * k * nch);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int bx = (int)(g % Wk);
        int64_t t = g / Wk;
        const int by = (int)(t % Hk);
        t /= Hk;
        const int cg = (int)(t % Cg);
        const int64_t n = t / Cg;
        const float tot = restore_walk<T, false>(pred, Cp, x_in, s, n, C, cg, nch, k, H, W, by * k, bx * k, 0.f, pred_nchw, shifted0, x0_hat);
        const float d = y[g] - tot / size;
        restore_walk<T, true>(pred, Cp, x_in, s, n, C, cg, nch, k, H, W, by * k, bx * k, d, pred_nchw, shifted0, x0_hat);
    }
}

// The measurement: items and routes as the x0 kernels, nothing to keep.
template <int K, bool GRAY>
__global__ __launch_bounds__(256) void restore_measure_kernel(const float* __restrict__ x, int C, int Hk, int W, int64_t items,
                                                              float* __restrict__ y) {
    const int W4 = W >> 2, Cg = GRAY ? 1 : C, nch = GRAY ? C : 1;
    const int64_t HW = (int64_t)Hk * K * W;
    const float size = (float)(K * K * nch);
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        const int x4 = (int)(it % W4);
        int64_t t = it / W4;
        const int by = (int)(t % Hk);
        t /= Hk;
        const int cg = (int)(t % Cg);
        const int64_t n = t / Cg;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int cc = 0; cc < nch; ++cc) {
            const int c = GRAY ? cc : cg;
#pragma unroll
            for (int r = 0; r < K; ++r) strip_add<K>(acc, load4(x + (n * C + c) * HW + (int64_t)(by * K + r) * W + 4 * x4));
        }
        if constexpr (K == 1) {
            store4(y + n * HW + 4 * x4, make_float4(acc[0] / size, acc[1] / size, acc[2] / size, acc[3] / size));
        } else if constexpr (K == 2) {
            float* yp = y + ((n * Cg + cg) * Hk + by) * (int64_t)(W >> 1) + 2 * x4;
            yp[0] = acc[0] / size;
            yp[1] = acc[1] / size;
        } else {
            float tot = acc[0];
            if constexpr (K == 8) tot += __shfl_xor(tot, 1, 64);
            if (K != 8 || (x4 & 1) == 0) y[((n * Cg + cg) * Hk + by) * (int64_t)(W / K) + (K == 8 ? x4 >> 1 : x4)] = tot / size;
        }
    }
}

__global__ __launch_bounds__(256) void restore_measure_scalar_kernel(const float* x, int k, int gray, int C, int H, int W, int64_t groups,
                                                                     float* y) {
    const int Hk = H / k, Wk = W / k, Cg = gray ? 1 : C, nch = gray ? C : 1, sw = k < 4 ? k : 4;
    const int64_t HW = (int64_t)H * W;
    const float size = (float)(k * k * nch);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int bx = (int)(g % Wk);
        int64_t t = g / Wk;
        const int by = (int)(t % Hk);
        t /= Hk;
        const int cg = (int)(t % Cg);
        const int64_t n = t / Cg;
        float tot = 0.f;
        for (int st = 0; st < k / sw; ++st) {
            float sum = 0.f;
            for (int cc = 0; cc < nch; ++cc)
                for (int r = 0; r < k; ++r)
                    for (int j = 0; j < sw; ++j) sum += x[(n * C + cg + cc) * HW + (int64_t)(by * k + r) * W + bx * k + st * sw + j];
            tot = st == 0 ? sum : tot + sum;
        }
        y[g] = tot / size;
    }
}

// One workgroup per image, the sums in inpaint_start_kernel's fixed order: a thread's elements in order, wave_sum, the four
// per-wave slots added as (0 + 1) + (2 + 3), channels in order.  VEC: W % 4 == 0 and a 16-byte aligned `expand`.
template <bool VEC>
__global__ __launch_bounds__(256) void restore_start_kernel(const float* y, int k, int gray, int per_channel, int C, int H, int W,
                                                            float* mu, float* expand) {
    const int img = blockIdx.x, t = threadIdx.x;
    const int Cy = gray ? 1 : C, Wk = W / k, HWk = (H / k) * Wk, HW = H * W;
    __shared__ float s_wsum[4][8], s_mu[8];
    const float* yi = y + (int64_t)img * Cy * HWk;
    if (mu) {
        for (int c = 0; c < Cy; ++c) {
            float sum = 0.f;
            for (int p = t; p < HWk; p += 256) sum += yi[(int64_t)c * HWk + p];
            sum = wave_sum(sum);
            if ((t & 63) == 0) s_wsum[t >> 6][c] = sum;
        }
        __syncthreads();
        if (t == 0) {
            float tot = 0.f, cs[8];
            for (int c = 0; c < Cy; ++c) {
                cs[c] = (s_wsum[0][c] + s_wsum[1][c]) + (s_wsum[2][c] + s_wsum[3][c]);
                tot += cs[c];
            }
            for (int c = 0; c < C; ++c) s_mu[c] = (per_channel && !gray) ? cs[c] / (float)HWk : tot / (float)(Cy * HWk);
        }
        __syncthreads();
        if (t < C) mu[(int64_t)img * C + t] = s_mu[t];
    }
    if (expand) {
        float* o = expand + (int64_t)img * C * HW;
        for (int c = 0; c < C; ++c) {
            const float* yc = yi + (int64_t)(gray ? 0 : c) * HWk;
            if (VEC) {
                for (int q = t; q < (HW >> 2); q += 256) {
                    const int p = 4 * q, row = p / W, col = p - row * W;
                    const float* yr = yc + (row / k) * Wk;
                    store4(o + (int64_t)c * HW + p, make_float4(yr[col / k], yr[(col + 1) / k], yr[(col + 2) / k], yr[(col + 3) / k]));
                }
            } else {
                for (int p = t; p < HW; p += 256) {
                    const int row = p / W, col = p - row * W;
                    o[(int64_t)c * HW + p] = yc[(row / k) * Wk + col / k];
                }
            }
        }
    }
}

// What every entry point refuses of the group description; -> 0 or -1 with the text set.
static int restore_groups(const char* who, int k, int gray, int N, int C, int H, int W) {
    MDM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "%s: N, C, H, W must be positive (%d, %d, %d, %d)", who, N, C, H, W);
    MDM_REQUIRE(C <= 8, "%s: C = %d is more than 8", who, C);
    MDM_REQUIRE(k == 1 || k == 2 || k == 4 || k == 8, "%s: k = %d must be 1, 2, 4 or 8", who, k);
    MDM_REQUIRE(H % k == 0 && W % k == 0, "%s: H = %d and W = %d must be multiples of k = %d", who, H, W, k);
    MDM_REQUIRE(gray == 0 || gray == 1, "%s: gray = %d must be 0 or 1", who, gray);
    MDM_REQUIRE(k * k * (gray ? C : 1) > 1, "%s: groups of one element (k = 1, %s) constrain nothing", who, gray ? "C = 1" : "no gray");
    return 0;
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_restore_x0(int dtype, const void* pred_nhwc, int Cp, const float* x_in, const float* s, const float* y, int k,
                              int gray, int N, int C, int H, int W, float* pred_nchw, float* shifted0, float* x0_hat, void* stream) {
    MDM_REQUIRE(pred_nhwc && x_in && y && x0_hat, "restore_x0: pred_nhwc, x_in, y and x0_hat are required");
    MDM_REQUIRE(dtype == MDM_F32 || dtype == MDM_BF16, "restore_x0: bad dtype %d", dtype);
    if (restore_groups("restore_x0", k, gray, N, C, H, W)) return -1;
    MDM_REQUIRE(Cp >= C, "restore_x0: Cp = %d is less than C = %d", Cp, C);
    const bool vec = ral16(x_in) && ral16(s) && ral16(pred_nchw) && ral16(shifted0) && ral16(x0_hat) && (!gray || C <= RESTORE_GRAY_C) &&
                     (k == 1 ? (H * W) % 4 == 0 && ral16(y) : W % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    const int Cg = gray ? 1 : C;
    if (!vec) {
        const int64_t groups = (int64_t)N * Cg * (H / k) * (W / k);
        const dim3 grid(rgrid(groups)), block(256);
        if (dtype == MDM_BF16)
            hipLaunchKernelGGL(restore_x0_scalar_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)pred_nhwc, Cp, x_in, s, y, k, gray, C, H,
                               W, groups, pred_nchw, shifted0, x0_hat);
        else
            hipLaunchKernelGGL(restore_x0_scalar_kernel<float>, grid, block, 0, st, (const float*)pred_nhwc, Cp, x_in, s, y, k, gray, C, H,
                               W, groups, pred_nchw, shifted0, x0_hat);
        return launch_status("restore_x0");
    }
    const int Hk = k == 1 ? 1 : H / k, Wr = k == 1 ? H * W : W;       // k = 1: the plane as one row
    const int64_t items = (int64_t)N * Cg * Hk * (Wr / 4);
    const dim3 grid(rgrid(items)), block(256);
#define MDM_RESTORE_X0(T, K, G)                                                                                                        \
    hipLaunchKernelGGL((restore_x0_kernel<T, K, G>), grid, block, 0, st, (const T*)pred_nhwc, Cp, x_in, s, y, C, Hk, Wr, items, pred_nchw, \
                       shifted0, x0_hat)
#define MDM_RESTORE_X0_K(T)                                                                                                            \
    do {                                                                                                                               \
        if (gray) {                                                                                                                    \
            if (k == 1) MDM_RESTORE_X0(T, 1, true); else if (k == 2) MDM_RESTORE_X0(T, 2, true);                                       \
            else if (k == 4) MDM_RESTORE_X0(T, 4, true); else MDM_RESTORE_X0(T, 8, true);                                              \
        } else {                                                                                                                       \
            if (k == 2) MDM_RESTORE_X0(T, 2, false); else if (k == 4) MDM_RESTORE_X0(T, 4, false); else MDM_RESTORE_X0(T, 8, false);   \
        }                                                                                                                              \
    } while (0)
    if (dtype == MDM_BF16) MDM_RESTORE_X0_K(bf16_t); else MDM_RESTORE_X0_K(float);
#undef MDM_RESTORE_X0_K
#undef MDM_RESTORE_X0
    return launch_status("restore_x0");
}

extern "C" int mdm_restore_measure(const float* x, int k, int gray, int N, int C, int H, int W, float* y, void* stream) {
    MDM_REQUIRE(x && y, "restore_measure: x and y are required");
    if (restore_groups("restore_measure", k, gray, N, C, H, W)) return -1;
    const bool vec = ral16(x) && (k == 1 ? (H * W) % 4 == 0 && ral16(y) : W % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    const int Cg = gray ? 1 : C;
    if (!vec) {
        const int64_t groups = (int64_t)N * Cg * (H / k) * (W / k);
        hipLaunchKernelGGL(restore_measure_scalar_kernel, dim3(rgrid(groups)), dim3(256), 0, st, x, k, gray, C, H, W, groups, y);
        return launch_status("restore_measure");
    }
    const int Hk = k == 1 ? 1 : H / k, Wr = k == 1 ? H * W : W;
    const int64_t items = (int64_t)N * Cg * Hk * (Wr / 4);
    const dim3 grid(rgrid(items)), block(256);
#define MDM_RESTORE_MEASURE(K, G) hipLaunchKernelGGL((restore_measure_kernel<K, G>), grid, block, 0, st, x, C, Hk, Wr, items, y)
    if (gray) {
        if (k == 1) MDM_RESTORE_MEASURE(1, true); else if (k == 2) MDM_RESTORE_MEASURE(2, true);
        else if (k == 4) MDM_RESTORE_MEASURE(4, true); else MDM_RESTORE_MEASURE(8, true);
    } else {
        if (k == 2) MDM_RESTORE_MEASURE(2, false); else if (k == 4) MDM_RESTORE_MEASURE(4, false); else MDM_RESTORE_MEASURE(8, false);
    }
#undef MDM_RESTORE_MEASURE
    return launch_status("restore_measure");
}

extern "C" int mdm_restore_start(const float* y, int k, int gray, int per_channel, int N, int C, int H, int W, float* mu, float* expand,
                                 void* stream) {
    MDM_REQUIRE(y, "restore_start: y is required");
    if (restore_groups("restore_start", k, gray, N, C, H, W)) return -1;
    if (!mu && !expand) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (W % 4 == 0 && ral16(expand))
        hipLaunchKernelGGL(restore_start_kernel<true>, dim3(N), dim3(256), 0, st, y, k, gray, per_channel, C, H, W, mu, expand);
    else
        hipLaunchKernelGGL(restore_start_kernel<false>, dim3(N), dim3(256), 0, st, y, k, gray, per_channel, C, H, W, mu, expand);
    return launch_status("restore_start");
}
