// Host check of csrc/vis.hip: the device code of grid_kernel and range_span, compiled for the CPU between the shims below, run lane by
// lane under AddressSanitizer / UBSan (scripts/vis_host_check.sh builds and runs it).  grid_kernel: image shapes x (K, nrow) x paddings x
// modes x image strides x aligned / misaligned pointers against a plain make_grid loop, inputs and outputs allocated at their exact sizes,
// so a read or write past an end is caught.  range_span: lengths x alignments with a NaN planted at the first, middle and last element --
// exactly one lane must see it.  No GPU is involved: this checks indices and bounds before a kernel runs on one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
static inline float4 load4(const float* p) { if ((uintptr_t)p & 15) { printf("MISALIGNED load4\n"); abort(); } return {p[0], p[1], p[2], p[3]}; }
static inline void store4(float* p, float4 v) { if ((uintptr_t)p & 15) { printf("MISALIGNED store4\n"); abort(); } p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
static inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
struct dim3s { unsigned x; } blockIdx, threadIdx;
#define MDM_REQUIRE(cond, ...) do { if (!(cond)) return -1; } while (0)
namespace mdm {
#include "range_part.inc"
#include "grid_part.inc"
}
using namespace mdm;

static std::vector<float> ref_grid(const std::vector<float>& xs, size_t xoff, int64_t stride, int K, int C, int H, int W, const float* lohi, int mode,
                                   int nrow, int padding, float pad, int& Cg, int& Hg, int& Wg) {
    Cg = C == 1 ? 3 : C;
    auto val = [&](int k, int c, int y, int x) {
        float v = xs[xoff + k * stride + ((size_t)(C == 1 ? 0 : c) * H + y) * W + x];
        if (mode == 1) { v = (v - lohi[2 * k]) / (lohi[2 * k + 1] - lohi[2 * k]); if (v != v) v = 0; }
        if (mode == 2) v = (v - lohi[0]) / (lohi[1] - lohi[0]);
        return v;
    };
    if (K == 1) { Hg = H; Wg = W; std::vector<float> g((size_t)Cg * H * W); for (int c = 0; c < Cg; ++c) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) g[((size_t)c * H + y) * W + x] = val(0, c, y, x); return g; }
    int xmaps = nrow < K ? nrow : K, ymaps = (K + xmaps - 1) / xmaps, h = H + padding, w = W + padding;
    Hg = h * ymaps + padding; Wg = w * xmaps + padding;
    std::vector<float> g((size_t)Cg * Hg * Wg, pad);
    int k = 0;
    for (int yy = 0; yy < ymaps; ++yy) for (int xx = 0; xx < xmaps; ++xx) { if (k >= K) break;
        for (int c = 0; c < Cg; ++c) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) g[((size_t)c * Hg + yy * h + padding + y) * Wg + xx * w + padding + x] = val(k, c, y, x);
        ++k; }
    return g;
}
static uint8_t ref_q(float v) { volatile float q = v * 255.f; q = q + 0.5f; float r = q; if (r != r) return 0; if (r < 0) r = 0; if (r > 255) r = 255; return (uint8_t)r; }

int main() {
    int fails = 0, rows = 0;
    // ---- range_span: every element is read exactly by one lane, whatever the alignment
    for (int n : {1, 2, 3, 4, 5, 7, 8, 255, 257, 768, 1000, 1031, 4099}) for (int mis = 0; mis < 4; ++mis) {
        float* raw = (float*)aligned_alloc(16, (n + mis) * 4 + 16 - ((n + mis) * 4) % 16);
        for (int i = 0; i < n; ++i) raw[mis + i] = (float)i;
        for (int pos : {0, n / 2, n - 1}) {
            float keep = raw[mis + pos]; raw[mis + pos] = NAN;
            Range r = {INFINITY, -INFINITY, 0.f}; int seen = 0;
            for (int t = 0; t < 256; ++t) { Range q = {INFINITY, -INFINITY, 0.f}; range_span(q, raw + mis, n, t); if (q.bad != 0) ++seen; r.lo = fminf(r.lo, q.lo); r.hi = fmaxf(r.hi, q.hi); }
            raw[mis + pos] = keep;
            float wlo = pos == 0 ? (n > 1 ? 1.f : INFINITY) : 0.f, whi = pos == n - 1 ? (n > 1 ? n - 2.f : -INFINITY) : n - 1.f;
            if (seen != 1 || r.lo != wlo || r.hi != whi) { printf("range n=%d mis=%d pos=%d seen=%d lo=%g hi=%g\n", n, mis, pos, seen, r.lo, r.hi); ++fails; }
            ++rows;
        }
        free(raw);
    }
    // ---- grid
    int chw[][3] = {{1, 1, 1}, {1, 3, 5}, {3, 16, 16}, {4, 8, 24}, {3, 5, 7}, {2, 4, 4}};
    int kn[][2] = {{1, 1}, {2, 2}, {4, 2}, {5, 3}, {7, 8}, {7, 1}, {100, 10}};
    for (auto& s : chw) for (auto& q : kn) for (int padding : {0, 2, 3}) for (int mode = 0; mode < 3; ++mode) for (int extra : {0, 7, 8}) for (int omis = 0; omis < 2; ++omis) {
        int C = s[0], H = s[1], W = s[2], K = q[0], nrow = q[1];
        int64_t E = (int64_t)C * H * W, stride = E + extra;
        size_t xoff = omis;                       // input misaligned too
        std::vector<float> xs(xoff + (K - 1) * stride + E);   // exact size: ASan catches a read past the last image
        for (size_t i = 0; i < xs.size(); ++i) xs[i] = (float)((i * 2654435761u) % 1000) / 999.f - 0.2f;
        std::vector<float> lohi(2 * K);
        for (int k = 0; k < K; ++k) { lohi[2 * k] = -0.3f - k; lohi[2 * k + 1] = 1.1f + k; }
        float pad = 0.5f;
        int Cg, Hg, Wg;
        std::vector<float> want = ref_grid(xs, xoff, stride, K, C, H, W, lohi.data(), mode, nrow, padding, pad, Cg, Hg, Wg);
        GridGeom g;
        if (grid_geom(K, C, H, W, nrow, padding, g, "t")) { printf("geom refused\n"); ++fails; continue; }
        if (g.Cg != Cg || g.Hg != Hg || g.Wg != Wg) { printf("shape\n"); ++fails; continue; }
        g.mode = mode; g.img_stride = stride; g.pad_value = pad;
        int64_t total = (int64_t)Cg * Hg * Wg, lanes = (total + 3) / 4;
        float* gfraw = (float*)aligned_alloc(16, (total + 4 + 3) / 4 * 16);
        float* gf = gfraw + (omis ? 1 : 0);
        uint8_t* gu = (uint8_t*)malloc(total + omis) + omis;    // exact size: a write past the end is caught
        for (int64_t i = 0; i < total; ++i) { gf[i] = -777.f; gu[i] = 0xAB; }
        std::vector<float> xin = xs;
        for (int64_t b = 0; b < (lanes + 255) / 256; ++b) for (int t = 0; t < 256; ++t) {
            blockIdx.x = (unsigned)b; threadIdx.x = t;
            grid_kernel(g, xs.data() + xoff, lohi.data(), gf, gu, total, ((uintptr_t)gf & 15) == 0, ((uintptr_t)gu & 3) == 0);
        }
        int bad = 0;
        for (int64_t i = 0; i < total; ++i) if (memcmp(&gf[i], &want[i], 4)) ++bad;
        for (int y = 0; y < Hg; ++y) for (int x = 0; x < Wg; ++x) for (int c = 0; c < Cg; ++c)
            if (gu[((size_t)y * Wg + x) * Cg + c] != ref_q(want[((size_t)c * Hg + y) * Wg + x])) ++bad;
        if (xin != xs) ++bad;
        if (bad) { printf("grid C%d H%d W%d K%d nrow%d pad%d mode%d extra%d omis%d: %d wrong\n", C, H, W, K, nrow, padding, mode, extra, omis, bad); ++fails; }
        ++rows;
        free(gfraw); free(gu - omis);
    }
    printf("%d rows, %d failed\n", rows, fails);
    return fails != 0;
}
