// Image grids on the device (include/mdm_vis.h): the {min, max} of images and the grid of torchvision's make_grid with upstream's two
// normalisations and save_image's quantisation in one pass.
//
// Replaces reference utils/datautils.py:211-229 (normalize01, normalize01_global), torchvision.utils.make_grid / save_image as
// sampler.py:369-387 (_save_image_grid), :390-417 and :474-484 call them.  Both kernels stream: the range kernel reads every element
// once, the grid kernel is driven by its OUTPUT -- a lane owns four consecutive elements of each output and looks up where they come
// from -- so every store is whole and nothing is written twice.
#include "common.h"
#include "../../include/mdm_vis.h"

namespace mdm {

constexpr int RANGE_MAX_PARTS = 1024;       // workgroups of a global range at most
constexpr int RANGE_PART_ELEMS = 16384;     // elements of one image a workgroup of a global range takes at least
static_assert(MDM_VIS_RANGE_SCRATCH_FLOATS == 4, "the four words of range_global_kernel");

struct Range { float lo, hi, bad; };

__device__ __forceinline__ void range_take(Range& r, float v) {
    r.lo = fminf(r.lo, v); r.hi = fmaxf(r.hi, v);      // fminf / fmaxf drop a NaN operand: it is carried in `bad`
    if (v != v) r.bad = 1.f;
}
// p[0 .. n): scalar loads up to the first 16-byte boundary, float4 over the aligned middle, scalar loads behind it
__device__ __forceinline__ void range_span(Range& r, const float* p, int64_t n, int t) {
    int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
    if (((uintptr_t)p & 3u) != 0 || head > n) head = n;        // (a float pointer is 4-byte aligned; if it is not, all scalar)
    for (int64_t i = t; i < head; i += 256) range_take(r, p[i]);
    const float* q = p + head;
    const int64_t n4 = (n - head) >> 2;
    for (int64_t i = t; i < n4; i += 256) {
        const float4 v = load4(q + 4 * i);
        range_take(r, v.x); range_take(r, v.y); range_take(r, v.z); range_take(r, v.w);
    }
    for (int64_t i = head + 4 * n4 + t; i < n; i += 256) range_take(r, p[i]);
}
// the workgroup's pair in every lane; a NaN seen by any lane makes both NaN
__device__ __forceinline__ void range_block(Range& r, int t) {
    __shared__ float s_lo[4], s_hi[4], s_bad[4];
    r.hi = wave_max(r.hi);
    r.lo = -wave_max(-r.lo);
    r.bad = wave_max(r.bad);
    __syncthreads();                                            // a second use of the arrays waits for the readers of the first
    if ((t & 63) == 0) { s_lo[t >> 6] = r.lo; s_hi[t >> 6] = r.hi; s_bad[t >> 6] = r.bad; }
    __syncthreads();
    r.lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    r.hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    r.bad = (s_bad[0] + s_bad[1]) + (s_bad[2] + s_bad[3]);
    if (r.bad != 0.f) r.lo = r.hi = __builtin_nanf("");
}

// one workgroup per image
__global__ __launch_bounds__(256) void range_image_kernel(const float* x, int64_t img_stride, int E, float* lohi) {
    const int t = threadIdx.x;
    const int64_t k = blockIdx.x;
    Range r = {__builtin_inff(), -__builtin_inff(), 0.f};
    range_span(r, x + k * img_stride, E, t);
    range_block(r, t);
    if (t == 0) { lohi[2 * k] = r.lo; lohi[2 * k + 1] = r.hi; }
}

// Global pair in one launch.  Workgroup b = (image slot, part): images slot, slot + slots, ..., of each the elements
// [part * chunk, (part + 1) * chunk).  Its pair goes into three words of scratch by device-scope atomics -- max of an order-preserving
// integer code of hi, max of the inverted code of lo, or of the NaN flag: 0 is below every code, so zeroed words are the empty range --
// and it then counts itself in the fourth.  The workgroup that counts last takes the three words, leaves 0 behind and writes lohi;
// atomicInc wraps at the workgroup count, so all four words are 0 again when the kernel ends.
__device__ __forceinline__ unsigned range_code(float v) {      // a < b  <=>  code(a) < code(b), -0 below +0; never 0 for a non-NaN
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float range_decode(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }

__global__ __launch_bounds__(256) void range_global_kernel(const float* x, int64_t img_stride, int K, int E, int slots, int nparts,
                                                           int chunk, float* lohi, unsigned* scratch) {
    const int t = threadIdx.x, b = blockIdx.x, nb = gridDim.x;
    const int slot = b / nparts, part = b - slot * nparts;
    const int64_t e0 = (int64_t)part * chunk;
    const int64_t len = e0 < E ? (E - e0 < chunk ? E - e0 : chunk) : 0;
    Range r = {__builtin_inff(), -__builtin_inff(), 0.f};
    for (int64_t k = slot; k < K; k += slots) range_span(r, x + k * img_stride + e0, len, t);
    range_block(r, t);
    if (t != 0) return;
    if (r.bad != 0.f) atomicOr(scratch + 2, 1u);
    else { atomicMax(scratch + 0, range_code(r.hi)); atomicMax(scratch + 1, ~range_code(r.lo)); }
    __threadfence();                                            // the three are done before this workgroup is counted
    if (atomicInc(scratch + 3, (unsigned)(nb - 1)) != (unsigned)(nb - 1)) return;
    __threadfence();
    const unsigned hi = atomicExch(scratch + 0, 0u), lo = atomicExch(scratch + 1, 0u), bad = atomicExch(scratch + 2, 0u);
    lohi[0] = bad ? __builtin_nanf("") : range_decode(~lo);
    lohi[1] = bad ? __builtin_nanf("") : range_decode(hi);
}

// ------------------------------------------------------------------ the grid
struct GridGeom {
    int K, C, H, W, Cg, Hg, Wg, xmaps, cellH, cellW, padding, mode;
    int64_t img_stride;
    float pad_value;
};

// source of grid element (y, x): image k and the offset of (iy, ix) in a channel plane, or k < 0 for padding
__device__ __forceinline__ int grid_source(const GridGeom& g, int y, int x, int& off) {
    if (g.K == 1) { off = y * g.W + x; return 0; }
    const int yy = y - g.padding, xx = x - g.padding;
    if (yy < 0 || xx < 0) return -1;
    const int r = yy / g.cellH, iy = yy - r * g.cellH, c = xx / g.cellW, ix = xx - c * g.cellW;
    if (iy >= g.H || ix >= g.W) return -1;
    const int64_t k = (int64_t)r * g.xmaps + c;
    if (k >= g.K) return -1;
    off = iy * g.W + ix;
    return (int)k;
}
__device__ __forceinline__ float grid_norm(const GridGeom& g, const float* lohi, int k, float v) {
    if (g.mode == 1) {
        const float lo = lohi[2 * k], hi = lohi[2 * k + 1];
        v = (v - lo) / (hi - lo);
        return v != v ? 0.f : v;
    }
    if (g.mode == 2) return (v - lohi[0]) / (lohi[1] - lohi[0]);
    return v;
}
__device__ __forceinline__ float grid_value(const GridGeom& g, const float* x, const float* lohi, int c, int y, int xc) {
    int off;
    const int k = grid_source(g, y, xc, off);
    if (k < 0) return g.pad_value;
    const int cs = g.C == 1 ? 0 : c;
    return grid_norm(g, lohi, k, x[k * g.img_stride + (int64_t)cs * g.H * g.W + off]);
}
// save_image: mul(255), add(0.5), clamp(0, 255), to uint8 -- product and sum rounded one after the other as torch does; fmaxf drops a NaN
__device__ __forceinline__ uint32_t grid_quant(float v) {
#pragma clang fp contract(off)
    float q = v * 255.f;
    q = q + 0.5f;
    return (uint32_t)(int)fminf(fmaxf(q, 0.f), 255.f);
}

// lane i: elements [4i, 4i + 4) of grid_f32 (flat over [Cg][Hg][Wg]) and elements [4i, 4i + 4) of grid_u8 (flat over [Hg][Wg][Cg])
__global__ __launch_bounds__(256) void grid_kernel(GridGeom g, const float* x, const float* lohi, float* gf, uint8_t* gu, int64_t total,
                                                   int f_vec, int u_vec) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= total) return;
    const int n = total - i0 < 4 ? (int)(total - i0) : 4;
    if (gf) {
        int xc = (int)(i0 % g.Wg);
        const int64_t r = i0 / g.Wg;
        int y = (int)(r % g.Hg), c = (int)(r / g.Hg);
        float v[4];
        int off = 0;
        const int k = n == 4 && xc + 3 < g.Wg ? grid_source(g, y, xc, off) : -1;
        const float* src = k < 0 ? nullptr : x + k * g.img_stride + (int64_t)(g.C == 1 ? 0 : c) * g.H * g.W + off;
        if (src && off % g.W + 3 < g.W && ((uintptr_t)src & 15u) == 0) {      // four pixels of one image row, aligned: one load
            const float4 q = load4(src);
            v[0] = grid_norm(g, lohi, k, q.x); v[1] = grid_norm(g, lohi, k, q.y);
            v[2] = grid_norm(g, lohi, k, q.z); v[3] = grid_norm(g, lohi, k, q.w);
        } else {
            for (int j = 0; j < n; ++j) {
                v[j] = grid_value(g, x, lohi, c, y, xc);
                if (++xc == g.Wg) { xc = 0; if (++y == g.Hg) { y = 0; ++c; } }
            }
        }
        if (n == 4 && f_vec) store4(gf + i0, make_float4(v[0], v[1], v[2], v[3]));
        else for (int j = 0; j < n; ++j) gf[i0 + j] = v[j];
    }
    if (gu) {
        int c = (int)(i0 % g.Cg);
        const int64_t r = i0 / g.Cg;
        int xc = (int)(r % g.Wg), y = (int)(r / g.Wg);
        uint32_t b[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < n; ++j) {
            b[j] = grid_quant(grid_value(g, x, lohi, c, y, xc));
            if (++c == g.Cg) { c = 0; if (++xc == g.Wg) { xc = 0; ++y; } }
        }
        if (n == 4 && u_vec) *reinterpret_cast<uint32_t*>(gu + i0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        else for (int j = 0; j < n; ++j) gu[i0 + j] = (uint8_t)b[j];
    }
}

static int grid_geom(int K, int C, int H, int W, int nrow, int padding, GridGeom& g, const char* who) {
    MDM_REQUIRE(K > 0 && C > 0 && H > 0 && W > 0, "%s: K, C, H, W must be positive (%d, %d, %d, %d)", who, K, C, H, W);
    MDM_REQUIRE(nrow > 0 && padding >= 0, "%s: nrow > 0 and padding >= 0 (%d, %d)", who, nrow, padding);
    g.K = K; g.C = C; g.H = H; g.W = W; g.padding = padding;
    g.Cg = C == 1 ? 3 : C;
    g.xmaps = nrow < K ? nrow : K;
    const int64_t ymaps = ((int64_t)K + g.xmaps - 1) / g.xmaps;
    const int64_t cellH = (int64_t)H + padding, cellW = (int64_t)W + padding;
    const int64_t Hg = K == 1 ? H : ymaps * cellH + padding, Wg = K == 1 ? W : g.xmaps * cellW + padding;
    MDM_REQUIRE(Hg <= INT32_MAX && Wg <= INT32_MAX && (int64_t)C * H * W <= INT32_MAX, "%s: the grid %lld x %lld is past 2^31 - 1", who,
                (long long)Hg, (long long)Wg);
    g.cellH = (int)cellH; g.cellW = (int)cellW; g.Hg = (int)Hg; g.Wg = (int)Wg;
    return 0;
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_vis_grid_shape(int K, int C, int H, int W, int nrow, int padding, int32_t out[3]) {
    MDM_REQUIRE(out, "vis_grid_shape: out is NULL");
    GridGeom g;
    if (int rc = grid_geom(K, C, H, W, nrow, padding, g, "vis_grid_shape")) return rc;
    out[0] = g.Cg; out[1] = g.Hg; out[2] = g.Wg;
    return 0;
}

extern "C" int mdm_vis_range(const float* x, int64_t img_stride, int K, int E, int global, float* lohi, float* scratch, void* stream) {
    MDM_REQUIRE(x && lohi, "vis_range: x or lohi is NULL");
    MDM_REQUIRE(K > 0 && E > 0, "vis_range: K and E must be positive (%d, %d)", K, E);
    MDM_REQUIRE(img_stride >= E, "vis_range: img_stride %lld < E %d", (long long)img_stride, E);
    if (!global) {
        hipLaunchKernelGGL(range_image_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, x, img_stride, E, lohi);
        return launch_status("vis_range");
    }
    MDM_REQUIRE(scratch && ((uintptr_t)scratch & 15u) == 0, "vis_range: a global range needs 16-byte aligned scratch");
    const int slots = K < RANGE_MAX_PARTS ? K : RANGE_MAX_PARTS;
    int nparts = cdiv(E, RANGE_PART_ELEMS);
    if (nparts > RANGE_MAX_PARTS / slots) nparts = RANGE_MAX_PARTS / slots;
    const int chunk = cdiv(E, nparts);
    hipLaunchKernelGGL(range_global_kernel, dim3(slots * nparts), dim3(256), 0, (hipStream_t)stream, x, img_stride, K, E, slots, nparts,
                       chunk, lohi, reinterpret_cast<unsigned*>(scratch));
    return launch_status("vis_range");
}

extern "C" int mdm_vis_grid(const float* x, int64_t img_stride, int K, int C, int H, int W, const float* lohi, int mode, int nrow,
                            int padding, float pad_value, float* grid_f32, uint8_t* grid_u8, void* stream) {
    GridGeom g;
    if (int rc = grid_geom(K, C, H, W, nrow, padding, g, "vis_grid")) return rc;
    MDM_REQUIRE(x, "vis_grid: x is NULL");
    MDM_REQUIRE(img_stride >= (int64_t)C * H * W, "vis_grid: img_stride %lld < C H W", (long long)img_stride);
    MDM_REQUIRE(grid_f32 || grid_u8, "vis_grid: both outputs are NULL");
    MDM_REQUIRE(mode >= 0 && mode <= 2, "vis_grid: mode %d is not 0, 1 or 2", mode);
    MDM_REQUIRE(mode == 0 || lohi, "vis_grid: mode %d needs lohi", mode);
    g.mode = mode; g.img_stride = img_stride; g.pad_value = pad_value;
    const int64_t total = (int64_t)g.Cg * g.Hg * g.Wg, lanes = (total + 3) / 4;
    MDM_REQUIRE((lanes + 255) / 256 <= INT32_MAX, "vis_grid: the grid has too many elements");
    hipLaunchKernelGGL(grid_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, x, lohi, grid_f32, grid_u8,
                       total, (int)(((uintptr_t)grid_f32 & 15u) == 0), (int)(((uintptr_t)grid_u8 & 3u) == 0));
    return launch_status("vis_grid");
}
