// Image-quality kernels (include/mdm_metric.h): MSE, PSNR and SSIM of fp32 NCHW images against their originals, whole-image and
// hole-only, as eight numbers per image.  Two launches: metric_tile_kernel forms one 16 x 32 tile of the SSIM map per workgroup
// from its 26 x 42 halo of both images in LDS (separable 11-tap windows: along W into LDS, along H out of it) and leaves six double
// partial sums per tile in the caller's workspace; metric_finish_kernel adds a row's partial sums in a fixed order and writes the
// eight floats.  No floating-point atomics: two launches give the same bits.
//
// Upstream has no counterpart.  An element is hole where keep == 0: -0 is hole, NaN is given.
#include <float.h>
#include <math.h>

#include "common.h"
#include "../../include/mdm_metric.h"

namespace mdm {

constexpr int MT_K = 11, MT_HALO = MT_K - 1;
constexpr int MT_TH = 16, MT_TW = 32;                                  // a tile of the map
constexpr int MT_HH = MT_TH + MT_HALO, MT_HW = MT_TW + MT_HALO;        // its halo: 26 x 42
constexpr int MT_LP = 44;                                              // LDS pitch of a halo row: 11 float4
constexpr int MT_SLOTS = 6;                                            // sq, sq_hole, ssim, ssim_hole, n_hole, n_hole_pos
constexpr int MT_MAX_GRID = 1 << 20;
constexpr int MT_LDS = (2 * MT_HH * MT_LP + 5 * MT_HH * MT_TW) * 4 + 4 * MT_SLOTS * 8;

struct MetricWin { float w[MT_K]; };

struct MetricPlan {
    int tiles_y, tiles_x;
    int64_t tiles_per_row, total, grid;
};

// the double Gaussian, normalised in double, each weight rounded once to float
static void metric_window(float* w) {
    double g[MT_K], sum = 0.0;
    for (int i = 0; i < MT_K; ++i) { const double d = i - 5; g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < MT_K; ++i) w[i] = (float)(g[i] / sum);
}

static int metric_plan(const char* who, int64_t R, int C, int H, int W, MetricPlan* p) {
    MDM_REQUIRE(R > 0 && C > 0 && H > 0 && W > 0, "%s: R, C, H, W must be positive (%lld, %d, %d, %d)", who, (long long)R, C, H, W);
    MDM_REQUIRE(H >= MT_K && W >= MT_K, "%s: H = %d and W = %d must be at least 11, the window", who, H, W);
    MDM_REQUIRE((int64_t)C * H * W <= INT32_MAX, "%s: C H W = %lld is past 2^31 - 1", who, (long long)C * H * W);
    p->tiles_y = cdiv(H - MT_HALO, MT_TH);
    p->tiles_x = cdiv(W - MT_HALO, MT_TW);
    p->tiles_per_row = (int64_t)C * p->tiles_y * p->tiles_x;
    MDM_REQUIRE(R <= INT64_MAX / (p->tiles_per_row * MT_SLOTS * 8), "%s: R = %lld rows of %lld tiles overflow the workspace size", who,
                (long long)R, (long long)p->tiles_per_row);
    p->total = R * p->tiles_per_row;
    p->grid = p->total < MT_MAX_GRID ? p->total : MT_MAX_GRID;
    return 0;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float clampf_keep_nan(float p, float lo, float hi, bool on) {
    if (on) { p = p < lo ? lo : p; p = p > hi ? hi : p; }              // comparisons: a NaN fails both and stays
    return p;
}
__device__ __forceinline__ float finite_or_zero(float c) { return fabsf(c) <= FLT_MAX ? c : 0.f; }

// VEC: W % 4 == 0 and pred, truth 16-byte aligned -- every halo row then starts on a 16-byte boundary (x0 is a multiple of 32).
template <bool VEC>
__global__ __launch_bounds__(256) void metric_tile_kernel(const float* pred, const float* truth, const float* keep, int Ck, int N, int C,
                                                          int H, int W, float lo, float hi, int do_clamp, double C1, double C2,
                                                          MetricWin win, int tiles_y, int tiles_x, int64_t total, double* ws) {
    __shared__ float s_p[MT_HH][MT_LP], s_t[MT_HH][MT_LP];
    __shared__ float s_h[5][MT_HH][MT_TW];
    __shared__ double s_red[4][MT_SLOTS];
    const int t = threadIdx.x;
    const int MH = H - MT_HALO, MW = W - MT_HALO;
    const int64_t HW = (int64_t)H * W;
    for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y);
        const int64_t rc = tile / ((int64_t)tiles_x * tiles_y);
        const int c = (int)(rc % C);
        const int64_t r = rc / C, n = r % N;
        const int y0 = ty * MT_TH, x0 = tx * MT_TW;
        const float* pb = pred + (r * C + c) * HW;
        const float* tb = truth + (n * C + c) * HW;
        const float* kb = keep ? keep + (n * Ck + (Ck == 1 ? 0 : c)) * HW : nullptr;
        // the elements whose squared difference this tile sums: its map extent, up to the image's edge on the last tile of an axis
        const int own_y1 = ty == tiles_y - 1 ? H : y0 + MT_TH, own_x1 = tx == tiles_x - 1 ? W : x0 + MT_TW;
        const int yc = min(y0 + MT_HALO / 2 + MT_TH / 2, H - 1), xc = min(x0 + MT_HALO / 2 + MT_TW / 2, W - 1);
        const float cp = finite_or_zero(clampf_keep_nan(pb[(int64_t)yc * W + xc], lo, hi, do_clamp));
        const float ct = finite_or_zero(tb[(int64_t)yc * W + xc]);
        double a_sq = 0.0, a_sqh = 0.0, a_ss = 0.0, a_ssh = 0.0, a_nh = 0.0, a_nhp = 0.0;

        auto stage = [&](int rr, int col, float pv, float tv) {        // one in-image element of the halo
            const int gy = y0 + rr, gx = x0 + col;
            const float p = clampf_keep_nan(pv, lo, hi, do_clamp);
            if (gy < own_y1 && gx < own_x1) {
                const float d = p - tv;
                const float sq = d * d;
                a_sq += (double)sq;
                if (!kb || kb[(int64_t)gy * W + gx] == 0.f) { a_sqh += (double)sq; a_nh += 1.0; }
            }
            s_p[rr][col] = p - cp;
            s_t[rr][col] = tv - ct;
        };
        if (VEC) {
            for (int it = t; it < MT_HH * (MT_LP / 4); it += 256) {
                const int rr = it / (MT_LP / 4), col = 4 * (it % (MT_LP / 4));
                const int gy = y0 + rr, gx = x0 + col;
                if (gy < H && gx < W) {                                // W % 4 == 0: the four columns are inside together
                    const float4 pv = load4(pb + (int64_t)gy * W + gx), tv = load4(tb + (int64_t)gy * W + gx);
                    stage(rr, col, pv.x, tv.x); stage(rr, col + 1, pv.y, tv.y); stage(rr, col + 2, pv.z, tv.z); stage(rr, col + 3, pv.w, tv.w);
                } else {
                    store4(&s_p[rr][col], make_float4(0.f, 0.f, 0.f, 0.f));
                    store4(&s_t[rr][col], make_float4(0.f, 0.f, 0.f, 0.f));
                }
            }
        } else {
            for (int it = t; it < MT_HH * MT_LP; it += 256) {
                const int rr = it / MT_LP, col = it % MT_LP;
                const int gy = y0 + rr, gx = x0 + col;
                if (gy < H && gx < W) stage(rr, col, pb[(int64_t)gy * W + gx], tb[(int64_t)gy * W + gx]);
                else { s_p[rr][col] = 0.f; s_t[rr][col] = 0.f; }
            }
        }
        __syncthreads();
        // along W: lane = output column, so the 32 lanes of a half-wave read 32 consecutive floats of one halo row (no bank conflict)
        for (int it = t; it < MT_HH * MT_TW; it += 256) {
            const int rr = it / MT_TW, x = it % MT_TW;
            float m_d = 0.f, m_e = 0.f, s_dd = 0.f, s_ee = 0.f, s_de = 0.f;
#pragma unroll
            for (int j = 0; j < MT_K; ++j) {
                const float d = s_p[rr][x + j], e = s_t[rr][x + j], w = win.w[j];
                const float dd = d * d, ee = e * e, de = d * e;
                m_d = __fmaf_rn(w, d, m_d); m_e = __fmaf_rn(w, e, m_e);
                s_dd = __fmaf_rn(w, dd, s_dd); s_ee = __fmaf_rn(w, ee, s_ee); s_de = __fmaf_rn(w, de, s_de);
            }
            s_h[0][rr][x] = m_d; s_h[1][rr][x] = m_e; s_h[2][rr][x] = s_dd; s_h[3][rr][x] = s_ee; s_h[4][rr][x] = s_de;
        }
        __syncthreads();
        // along H: the lanes of a half-wave read one row of 32 floats per tap
        for (int it = t; it < MT_TH * MT_TW; it += 256) {
            const int y = it / MT_TW, x = it % MT_TW;
            if (y0 + y < MH && x0 + x < MW) {
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < MT_K; ++i) {
                    const float w = win.w[i];
#pragma unroll
                    for (int k = 0; k < 5; ++k) m[k] = __fmaf_rn(w, s_h[k][y + i][x], m[k]);
                }
                const double md = m[0], me = m[1];
                const double mu_p = (double)cp + md, mu_t = (double)ct + me;
                const double var_p = (double)m[2] - md * md, var_t = (double)m[3] - me * me, cov = (double)m[4] - md * me;
                const double v = ((2.0 * mu_p * mu_t + C1) * (2.0 * cov + C2)) / ((mu_p * mu_p + mu_t * mu_t + C1) * (var_p + var_t + C2));
                a_ss += v;
                if (!kb || kb[(int64_t)(y0 + y + MT_HALO / 2) * W + (x0 + x + MT_HALO / 2)] == 0.f) { a_ssh += v; a_nhp += 1.0; }
            }
        }
        double acc[MT_SLOTS] = {a_sq, a_sqh, a_ss, a_ssh, a_nh, a_nhp};
#pragma unroll
        for (int k = 0; k < MT_SLOTS; ++k) {
            const double s = wave_sum_d(acc[k]);
            if ((t & 63) == 0) s_red[t >> 6][k] = s;
        }
        __syncthreads();                                               // (also: every read of s_p, s_t, s_h is behind us)
        if (t < MT_SLOTS) ws[tile * MT_SLOTS + t] = (s_red[0][t] + s_red[1][t]) + (s_red[2][t] + s_red[3][t]);
        __syncthreads();                                               // s_red is free for the next tile
    }
}

// one wave per row: the row's tiles strided over the lanes in order, then the butterfly
__global__ __launch_bounds__(64) void metric_finish_kernel(const double* ws, int64_t tiles_per_row, double n_elem, double n_pos, double L2,
                                                           float* out) {
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const double* w = ws + r * tiles_per_row * MT_SLOTS;
    double s[MT_SLOTS];
#pragma unroll
    for (int k = 0; k < MT_SLOTS; ++k) {
        double a = 0.0;
        for (int64_t i = lane; i < tiles_per_row; i += 64) a += w[i * MT_SLOTS + k];
        s[k] = wave_sum_d(a);
    }
    if (lane == 0) {
        const double mse = s[0] / n_elem, mse_h = s[1] / s[4];
        float* o = out + r * 8;
        o[0] = (float)mse;
        o[1] = (float)(10.0 * log10(L2 / mse));
        o[2] = (float)(s[2] / n_pos);
        o[3] = (float)mse_h;
        o[4] = (float)(10.0 * log10(L2 / mse_h));
        o[5] = (float)(s[3] / s[5]);
        o[6] = (float)s[4];
        o[7] = (float)s[5];
    }
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_metric_plan(int64_t R, int C, int H, int W, int32_t* tile_h, int32_t* tile_w, int32_t* tiles_y, int32_t* tiles_x,
                               int64_t* grid, int32_t* lds_bytes, float* window) {
    MetricPlan p;
    if (metric_plan("metric_plan", R, C, H, W, &p)) return -1;
    if (tile_h) *tile_h = MT_TH;
    if (tile_w) *tile_w = MT_TW;
    if (tiles_y) *tiles_y = p.tiles_y;
    if (tiles_x) *tiles_x = p.tiles_x;
    if (grid) { grid[0] = p.grid; grid[1] = R; }
    if (lds_bytes) *lds_bytes = MT_LDS;
    if (window) metric_window(window);
    return 0;
}

extern "C" int64_t mdm_metric_ws_bytes(int64_t R, int C, int H, int W) {
    MetricPlan p;
    if (metric_plan("metric_ws_bytes", R, C, H, W, &p)) return -1;
    return p.total * MT_SLOTS * 8;
}

extern "C" int mdm_metric_image(const float* pred, const float* truth, const float* keep, int Ck, int64_t R, int N, int C, int H, int W,
                                float clamp_lo, float clamp_hi, float data_range, void* ws, int64_t ws_bytes, float* out, void* stream) {
    MDM_REQUIRE(pred && truth && out && ws, "metric_image: pred, truth, out and ws are required");
    MDM_REQUIRE(N > 0, "metric_image: N = %d must be positive", N);
    MetricPlan p;
    if (metric_plan("metric_image", R, C, H, W, &p)) return -1;
    MDM_REQUIRE(R <= INT32_MAX, "metric_image: R = %lld is past 2^31 - 1", (long long)R);
    MDM_REQUIRE(R % N == 0, "metric_image: R = %lld is not a multiple of N = %d", (long long)R, N);
    MDM_REQUIRE(!keep || Ck == 1 || Ck == C, "metric_image: Ck = %d must be 1 or C = %d", Ck, C);
    MDM_REQUIRE(data_range > 0.f && data_range <= FLT_MAX, "metric_image: data_range = %g must be positive and finite", (double)data_range);
    MDM_REQUIRE(ws_bytes >= p.total * MT_SLOTS * 8, "metric_image: ws_bytes = %lld, mdm_metric_ws_bytes asks for %lld", (long long)ws_bytes,
                (long long)(p.total * MT_SLOTS * 8));
    MDM_REQUIRE(((uintptr_t)ws & 7u) == 0, "metric_image: ws is not 8-byte aligned");
    MetricWin win;
    metric_window(win.w);
    const double L = (double)data_range, C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    const int do_clamp = clamp_lo < clamp_hi;
    const bool vec = W % 4 == 0 && (((uintptr_t)pred | (uintptr_t)truth) & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    double* wsd = (double*)ws;
    if (vec) hipLaunchKernelGGL(metric_tile_kernel<true>, dim3((unsigned)p.grid), dim3(256), 0, st, pred, truth, keep, Ck, N, C, H, W, clamp_lo,
                                clamp_hi, do_clamp, C1, C2, win, p.tiles_y, p.tiles_x, p.total, wsd);
    else hipLaunchKernelGGL(metric_tile_kernel<false>, dim3((unsigned)p.grid), dim3(256), 0, st, pred, truth, keep, Ck, N, C, H, W, clamp_lo,
                            clamp_hi, do_clamp, C1, C2, win, p.tiles_y, p.tiles_x, p.total, wsd);
    if (int rc = launch_status("metric_image")) return rc;
    hipLaunchKernelGGL(metric_finish_kernel, dim3((unsigned)R), dim3(64), 0, st, (const double*)wsd, p.tiles_per_row,
                       (double)C * H * W, (double)C * (H - MT_HALO) * (W - MT_HALO), L * L, out);
    return launch_status("metric_image");
}
