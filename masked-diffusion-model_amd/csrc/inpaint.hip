// Inpainting-sampler kernels (include/mdm_inpaint.h): the x0 reconstruction of a reverse step with the projection onto the given
// pixels, and the start image / hole size of a run.  NCHW fp32; pure HBM streaming like interp.hip: 256-thread workgroups, at most
// 2048 of them with a grid stride (x0) or one per image (start), 16 bytes per lane wherever the extents and the addresses allow it.
//
// Upstream has no counterpart.  A pixel is given where keep != 0: -0 is not given, NaN is given.
#include "common.h"
#include "../../include/mdm_inpaint.h"

namespace mdm {

constexpr int INPAINT_MAX_GRID = 2048;

static inline int pgrid(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > INPAINT_MAX_GRID ? INPAINT_MAX_GRID : b));
}
static inline bool pal16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// V = 4: one thread per four consecutive elements of one (n, c) plane (HW % 4 == 0); V = 1: one thread per element.  The NHWC
// prediction is read one element at a time on both routes (its pixels are Cp elements apart), as sampler_x0_kernel reads it.
template <typename T, int V>
__global__ __launch_bounds__(256) void inpaint_x0_kernel(const T* pred, int Cp, const float* x_in, const float* s, const float* known,
                                                         const float* keep, int keep_C, int C, int HW, int64_t total, float* pred_nchw,
                                                         float* shifted0, float* x0_hat) {
    const int64_t items = total / V;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = it * V;
        const int p = (int)(i % HW);
        const int64_t r = i / HW;
        const int c = (int)(r % C);
        const int64_t n = r / C;
        const int64_t ik = (n * keep_C + (keep_C == 1 ? 0 : c)) * HW + p;
        const T* pp = pred + (n * HW + p) * Cp + c;
        float pv[V], xi[V], sv[V], kn[V], kp[V];
        if constexpr (V == 4) {
            const float4 a = load4(x_in + i), b = load4(known + i), k = load4(keep + ik);
            const float4 z = s ? load4(s + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            xi[0] = a.x; xi[1] = a.y; xi[2] = a.z; xi[3] = a.w;
            kn[0] = b.x; kn[1] = b.y; kn[2] = b.z; kn[3] = b.w;
            kp[0] = k.x; kp[1] = k.y; kp[2] = k.z; kp[3] = k.w;
            sv[0] = z.x; sv[1] = z.y; sv[2] = z.z; sv[3] = z.w;
        } else {
            xi[0] = x_in[i]; kn[0] = known[i]; kp[0] = keep[ik]; sv[0] = s ? s[i] : 0.f;
        }
        float sh[V], xo[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            pv[k] = Elem<T>::ld(pp + (int64_t)k * Cp);
            sh[k] = xi[k] + pv[k];
            const float x = s ? sh[k] - sv[k] : sh[k];
            xo[k] = (kp[k] != 0.f) ? kn[k] : x;                // a select: the given value passes through untouched
        }
        if constexpr (V == 4) {
            if (pred_nchw) store4(pred_nchw + i, make_float4(pv[0], pv[1], pv[2], pv[3]));
            if (shifted0) store4(shifted0 + i, make_float4(sh[0], sh[1], sh[2], sh[3]));
            store4(x0_hat + i, make_float4(xo[0], xo[1], xo[2], xo[3]));
        } else {
            if (pred_nchw) pred_nchw[i] = pv[0];
            if (shifted0) shifted0[i] = sh[0];
            x0_hat[i] = xo[0];
        }
    }
}

// One workgroup per image, as degrade_kernel: pass A sums the given values and counts them per channel (fp32 sums in degrade_kernel's
// fixed order: wave_sum, four per-wave slots added as (0 + 1) + (2 + 3), channels in order; the counts are integers), pass B
// writes the start image, pass C counts the pixels with a channel not given.  VEC: HW % 4 == 0 and 16-byte aligned planes.
template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_start_kernel(const float* known, const float* keep, int keep_C, const float* fallback,
                                                            int per_channel, int C, int HW, float* x_start, float* mu, int32_t* unknown) {
    const int img = blockIdx.x, t = threadIdx.x;
    __shared__ float s_wsum[4][8], s_mu[8];
    __shared__ int s_wcnt[4][8], s_wunk[4];
    const float* kn = known + (int64_t)img * C * HW;
    const float* kp = keep + (int64_t)img * keep_C * HW;
    if (x_start || mu) {
        for (int c = 0; c < C; ++c) {
            const float* a = kn + (int64_t)c * HW;
            const float* k = kp + (int64_t)(keep_C == 1 ? 0 : c) * HW;
            float sum = 0.f;
            int cnt = 0;
            if (VEC) {
                for (int q = t; q < (HW >> 2); q += 256) {
                    const float4 av = load4(a + 4 * q), kv = load4(k + 4 * q);
                    if (kv.x != 0.f) { sum += av.x; ++cnt; }
                    if (kv.y != 0.f) { sum += av.y; ++cnt; }
                    if (kv.z != 0.f) { sum += av.z; ++cnt; }
                    if (kv.w != 0.f) { sum += av.w; ++cnt; }
                }
            } else {
                for (int p = t; p < HW; p += 256)
                    if (k[p] != 0.f) { sum += a[p]; ++cnt; }
            }
            sum = wave_sum(sum); cnt = wave_sum_i(cnt);
            if ((t & 63) == 0) { s_wsum[t >> 6][c] = sum; s_wcnt[t >> 6][c] = cnt; }
        }
        __syncthreads();
        if (t == 0) {
            float tot = 0.f;
            int ntot = 0;
            float cs[8];
            int cn[8];
            for (int c = 0; c < C; ++c) {
                cs[c] = (s_wsum[0][c] + s_wsum[1][c]) + (s_wsum[2][c] + s_wsum[3][c]);
                cn[c] = (s_wcnt[0][c] + s_wcnt[1][c]) + (s_wcnt[2][c] + s_wcnt[3][c]);
                tot += cs[c]; ntot += cn[c];
            }
            for (int c = 0; c < C; ++c) {
                const float fb = fallback[(int64_t)img * C + c];
                if (per_channel) s_mu[c] = cn[c] ? cs[c] / (float)cn[c] : fb;
                else s_mu[c] = ntot ? tot / (float)ntot : fb;
            }
        }
        __syncthreads();
        if (mu && t < C) mu[(int64_t)img * C + t] = s_mu[t];
        if (x_start) {
            float* o = x_start + (int64_t)img * C * HW;
            for (int c = 0; c < C; ++c) {
                const float* a = kn + (int64_t)c * HW;
                const float* k = kp + (int64_t)(keep_C == 1 ? 0 : c) * HW;
                const float m = s_mu[c];
                if (VEC) {
                    for (int q = t; q < (HW >> 2); q += 256) {
                        const float4 av = load4(a + 4 * q), kv = load4(k + 4 * q);
                        store4(o + (int64_t)c * HW + 4 * q, make_float4(kv.x != 0.f ? av.x : m, kv.y != 0.f ? av.y : m,
                                                                          kv.z != 0.f ? av.z : m, kv.w != 0.f ? av.w : m));
                    }
                } else {
                    for (int p = t; p < HW; p += 256) o[(int64_t)c * HW + p] = k[p] != 0.f ? a[p] : m;
                }
            }
        }
    }
    if (unknown) {
        int u = 0;
        for (int p = t; p < HW; p += 256) {
            bool hole = false;
            for (int c = 0; c < keep_C; ++c) hole = hole || !(kp[(int64_t)c * HW + p] != 0.f);
            u += hole ? 1 : 0;
        }
        u = wave_sum_i(u);
        if ((t & 63) == 0) s_wunk[t >> 6] = u;
        __syncthreads();
        if (t == 0) unknown[img] = (s_wunk[0] + s_wunk[1]) + (s_wunk[2] + s_wunk[3]);
    }
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_inpaint_x0(int dtype, const void* pred_nhwc, int Cp, const float* x_in, const float* s, const float* known,
                              const float* keep, int keep_C, int N, int C, int H, int W, float* pred_nchw, float* shifted0,
                              float* x0_hat, void* stream) {
    MDM_REQUIRE(pred_nhwc && x_in && known && keep && x0_hat, "inpaint_x0: pred_nhwc, x_in, known, keep and x0_hat are required");
    MDM_REQUIRE(dtype == MDM_F32 || dtype == MDM_BF16, "inpaint_x0: bad dtype %d", dtype);
    MDM_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "inpaint_x0: N, C, H, W must be positive (%d, %d, %d, %d)", N, C, H, W);
    MDM_REQUIRE(C <= 8, "inpaint_x0: C = %d is more than 8", C);
    MDM_REQUIRE(Cp >= C, "inpaint_x0: Cp = %d is less than C = %d", Cp, C);
    MDM_REQUIRE(keep_C == 1 || keep_C == C, "inpaint_x0: keep_C = %d must be 1 or C = %d", keep_C, C);
    const int HW = H * W;
    const int64_t total = (int64_t)N * C * HW;
    const bool vec = HW % 4 == 0 && pal16(x_in) && pal16(s) && pal16(known) && pal16(keep) && pal16(pred_nchw) && pal16(shifted0) &&
                     pal16(x0_hat);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(pgrid(vec ? total / 4 : total)), block(256);
#define MDM_INPAINT_X0(T, V)                                                                                                          \
    hipLaunchKernelGGL((inpaint_x0_kernel<T, V>), grid, block, 0, st, (const T*)pred_nhwc, Cp, x_in, s, known, keep, keep_C, C, HW, total, \
                       pred_nchw, shifted0, x0_hat)
    if (dtype == MDM_BF16) { if (vec) MDM_INPAINT_X0(bf16_t, 4); else MDM_INPAINT_X0(bf16_t, 1); }
    else { if (vec) MDM_INPAINT_X0(float, 4); else MDM_INPAINT_X0(float, 1); }
#undef MDM_INPAINT_X0
    return launch_status("inpaint_x0");
}

extern "C" int mdm_inpaint_start(const float* known, const float* keep, int keep_C, const float* fallback, int per_channel, int N, int C,
                                 int HW, float* x_start, float* mu, int32_t* unknown, void* stream) {
    MDM_REQUIRE(known && keep && fallback, "inpaint_start: known, keep and fallback are required");
    MDM_REQUIRE(N > 0 && C > 0 && HW > 0, "inpaint_start: N, C, HW must be positive (%d, %d, %d)", N, C, HW);
    MDM_REQUIRE(C <= 8, "inpaint_start: C = %d is more than 8", C);
    MDM_REQUIRE(keep_C == 1 || keep_C == C, "inpaint_start: keep_C = %d must be 1 or C = %d", keep_C, C);
    if (!x_start && !mu && !unknown) return 0;
    const bool vec = HW % 4 == 0 && pal16(known) && pal16(keep) && pal16(x_start);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(inpaint_start_kernel<true>, dim3(N), dim3(256), 0, st, known, keep, keep_C, fallback, per_channel, C, HW,
                                x_start, mu, unknown);
    else hipLaunchKernelGGL(inpaint_start_kernel<false>, dim3(N), dim3(256), 0, st, known, keep, keep_C, fallback, per_channel, C, HW,
                            x_start, mu, unknown);
    return launch_status("inpaint_start");
}
