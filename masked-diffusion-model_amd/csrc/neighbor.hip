// Nearest-neighbour search on the stored data set (include/mdm_neighbor.h): one launch turns stored images -- uint8 or float, as
// include/mdm_data.h keeps them -- into unit-length feature rows (normalize01, mirror, separable resize, 1 / norm), and a column
// arg-max searches the similarity matrices of those rows chunk by chunk.
//
// Replaces reference sampler.py:487-518 (Sampler.get_nearest_neighbor: a DataLoader pass per query with normalize01, Resize([32, 32]),
// RandomHorizontalFlip and B x M cosine similarities) and the full-resolution pass of tester.py:189-206.  mdm_nn_plan states torch's
// interpolate tap tables on the host.  The row kernel streams: one workgroup per image reads the storage once for the range and once
// for the taps -- 16-byte loads over the aligned middle of every span -- and writes only the row.  With a resize, a tile of source
// rows of one channel is staged in LDS as normalised floats (odd pitch: the lanes of the horizontal pass walk down a column of the
// tile), filtered along W into S values per source row, and each of those is added into the accumulators of the output rows whose
// support holds that source row; every lane touches only its own accumulators, in source-row order.  No atomics.
#include "common.h"
#include "../../include/mdm_neighbor.h"

#include <math.h>

namespace mdm {

constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 4096;            // floats of one staged tile of source rows; also the cap of the horizontal-pass buffer
constexpr int NN_HTABLE = 2048;          // floats of the horizontal weight table kept in LDS
constexpr int NN_MAX_S = 64;             // S S accumulators of one channel live in LDS

struct NnArgs {
    const void* src;
    const float* lut;
    const int32_t *hfirst, *hcount, *vfirst, *vcount;
    const float *hweight, *vweight;
    float* rows;
    int64_t img_stride, first, row_ld;
    int C, H, W, S, htaps, vtaps, normalize, flip;
    int P, TR, HP;                       // tile pitch (W | 1), source rows per tile, pitch of the horizontal-pass buffer (TR | 1)
    float eps;
};

__device__ __forceinline__ int nn_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// f(i0, v, n): the values of stored elements [off + i0, off + i0 + n), n <= 16, every element of [off, off + len) exactly once over the
// workgroup: scalar loads up to the first 16-byte boundary, 16-byte loads over the aligned middle, scalar loads behind it.
// lut: the workgroup's LDS copy of the table (kind 1).
template <int KIND, class F>
__device__ __forceinline__ void nn_span(const void* src, const float* lut, int64_t off, int len, int t, F&& f) {
    if (KIND == 0) {
        const float* p = static_cast<const float*>(src) + off;
        int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
        if (((uintptr_t)p & 3u) != 0 || head > len) head = len;
        for (int i = t; i < head; i += NN_THREADS) { const float v = p[i]; f(i, &v, 1); }
        const float* q = p + head;
        const int n4 = (len - head) >> 2;
        for (int i = t; i < n4; i += NN_THREADS) {
            const float4 w = load4(q + 4 * (int64_t)i);
            const float v[4] = {w.x, w.y, w.z, w.w};
            f(head + 4 * i, v, 4);
        }
        for (int i = head + 4 * n4 + t; i < len; i += NN_THREADS) { const float v = p[i]; f(i, &v, 1); }
    } else {
        const uint8_t* p = static_cast<const uint8_t*>(src) + off;
        int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
        if (head > len) head = len;
        for (int i = t; i < head; i += NN_THREADS) { const float v = lut[p[i]]; f(i, &v, 1); }
        const uint8_t* q = p + head;
        const int n16 = (len - head) >> 4;
        for (int i = t; i < n16; i += NN_THREADS) {
            const uint4 w = *reinterpret_cast<const uint4*>(q + 16 * (int64_t)i);
            const uint32_t u[4] = {w.x, w.y, w.z, w.w};
            float v[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[4 * j] = lut[u[j] & 255u]; v[4 * j + 1] = lut[(u[j] >> 8) & 255u];
                v[4 * j + 2] = lut[(u[j] >> 16) & 255u]; v[4 * j + 3] = lut[u[j] >> 24];
            }
            f(head + 16 * i, v, 16);
        }
        for (int i = head + 16 * n16 + t; i < len; i += NN_THREADS) { const float v = lut[p[i]]; f(i, &v, 1); }
    }
}

// normalize01 of one value as normalize01_kernel (eval.hip) computes it: an IEEE division, NaN -> 0
__device__ __forceinline__ float nn_norm01(float v, float lo, float range) {
    const float r = (v - lo) / range;
    return r != r ? 0.f : r;
}

// sum over the workgroup in one order: the wave butterflies, then (p0 + p1) + (p2 + p3); every thread gets the sum
__device__ __forceinline__ float nn_block_sum(float a, float* part, int t) {
    a = wave_sum(a);
    __syncthreads();
    if ((t & 63) == 0) part[t >> 6] = a;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// one workgroup per row r.  Dynamic LDS: lut[256] | S == 0: nothing more
//                                                  | S > 0: tile[TR P] | hbuf[S HP] | acc[S S] | hw[S htaps] | hf[S] | hc[S]
template <int KIND> __global__ __launch_bounds__(NN_THREADS) void nn_rows_kernel(NnArgs a) {
    extern __shared__ float nn_lds[];
    __shared__ float s_lo[4], s_hi[4], s_bad[4], s_part[4];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int E = a.C * a.H * a.W, HW = a.H * a.W;
    const int64_t img = (a.first + r) * a.img_stride;
    float* row = a.rows + r * a.row_ld;
    float* s_lut = nn_lds;
    if (KIND == 1) {
        s_lut[t] = a.lut[t];
        __syncthreads();
    }

    // ---- the range of the image: min and max hand a NaN on (fminf / fmaxf drop it, so it is carried beside them)
    float lo = 0.f, range = 1.f;
    if (a.normalize) {
        float mn = __builtin_inff(), mx = -__builtin_inff(), bad = 0.f;
        nn_span<KIND>(a.src, s_lut, img, E, t, [&](int, const float* v, int n) {
            for (int j = 0; j < n; ++j) { mn = fminf(mn, v[j]); mx = fmaxf(mx, v[j]); if (v[j] != v[j]) bad = 1.f; }
        });
        mx = wave_max(mx);
        mn = -wave_max(-mn);
        bad = wave_max(bad);
        if ((t & 63) == 0) { s_lo[t >> 6] = mn; s_hi[t >> 6] = mx; s_bad[t >> 6] = bad; }
        __syncthreads();
        lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        const float hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
        bad = (s_bad[0] + s_bad[1]) + (s_bad[2] + s_bad[3]);
        range = bad != 0.f ? __builtin_nanf("") : hi - lo;
        if (KIND == 1) {                 // a value depends on its byte alone: 256 divisions per image instead of C H W
            __syncthreads();
            s_lut[t] = nn_norm01(s_lut[t], lo, range);
            __syncthreads();
        }
    }
    const bool scale_here = a.normalize && KIND == 0;

    const int D = a.S > 0 ? a.C * a.S * a.S : E;
    float ss = 0.f;
    if (a.S == 0) {
        // ---- full resolution: lane groups of four consecutive row elements, g = t, t + 256, ...
        const bool vec = ((uintptr_t)row & 15u) == 0;
        for (int g = t; 4 * (int64_t)g < D; g += NN_THREADS) {
            const int e0 = 4 * g, cnt = D - e0 < 4 ? D - e0 : 4;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cnt; ++j) {
                int e = e0 + j;
                if (a.flip) { const int w = e % a.W; e += a.W - 1 - 2 * w; }
                float x;
                if (KIND == 0) x = static_cast<const float*>(a.src)[img + e];
                else x = s_lut[static_cast<const uint8_t*>(a.src)[img + e]];
                v[j] = scale_here ? nn_norm01(x, lo, range) : x;
                ss = fmaf(v[j], v[j], ss);
            }
            if (vec && cnt == 4) store4(row + e0, make_float4(v[0], v[1], v[2], v[3]));
            else for (int j = 0; j < cnt; ++j) row[e0 + j] = v[j];
        }
    } else {
        const int S = a.S, SS = S * S;
        float* tile = nn_lds + 256;
        float* hbuf = tile + a.TR * a.P;
        float* acc = hbuf + S * a.HP;
        float* hw = acc + SS;
        int* hf = reinterpret_cast<int*>(hw + S * a.htaps);
        int* hc = hf + S;
        for (int i = t; i < S * a.htaps; i += NN_THREADS) hw[i] = a.hweight[i];
        for (int i = t; i < S; i += NN_THREADS) {
            hf[i] = nn_clamp(a.hfirst[i], 0, a.W - 1);
            hc[i] = nn_clamp(a.hcount[i], 0, a.htaps);
        }
        for (int c = 0; c < a.C; ++c) {
            for (int e = t; e < SS; e += NN_THREADS) acc[e] = 0.f;
            for (int y0 = 0; y0 < a.H; y0 += a.TR) {
                const int nrows = a.H - y0 < a.TR ? a.H - y0 : a.TR;
                __syncthreads();                                   // the tile and hbuf of the pass before are read out (and hw is there)
                nn_span<KIND>(a.src, s_lut, img + (int64_t)c * HW + (int64_t)y0 * a.W, nrows * a.W, t, [&](int i0, const float* v, int n) {
                    int rr = i0 / a.W, cc = i0 - rr * a.W;
                    for (int j = 0; j < n; ++j) {
                        tile[rr * a.P + (a.flip ? a.W - 1 - cc : cc)] = scale_here ? nn_norm01(v[j], lo, range) : v[j];
                        if (++cc == a.W) { cc = 0; ++rr; }
                    }
                });
                __syncthreads();
                // along W: q = ox nrows + tr, the source row fastest, so that a wave reads down a column of the odd-pitched tile
                for (int q = t; q < nrows * S; q += NN_THREADS) {
                    const int ox = q / nrows, tr = q - ox * nrows;
                    const float* trow = tile + tr * a.P;
                    const float* w = hw + ox * a.htaps;
                    const int f0 = hf[ox], n = hc[ox];
                    float h = 0.f;
                    for (int i = 0; i < n; ++i) {
                        const int col = f0 + i < a.W ? f0 + i : a.W - 1;
                        h = fmaf(w[i], trow[col], h);
                    }
                    hbuf[ox * a.HP + tr] = h;
                }
                __syncthreads();
                // along H: output e = oy S + ox takes the rows of this tile that its support holds, in source-row order
                for (int e = t; e < SS; e += NN_THREADS) {
                    const int oy = e / S, ox = e - oy * S;
                    const int f0 = nn_clamp(a.vfirst[oy], 0, a.H - 1), n = nn_clamp(a.vcount[oy], 0, a.vtaps);
                    const int ylo = f0 > y0 ? f0 : y0, yhi = f0 + n < y0 + nrows ? f0 + n : y0 + nrows;
                    float s = acc[e];
                    for (int y = ylo; y < yhi; ++y) s = fmaf(a.vweight[oy * a.vtaps + (y - f0)], hbuf[ox * a.HP + (y - y0)], s);
                    acc[e] = s;
                }
            }
            for (int e = t; e < SS; e += NN_THREADS) {
                const float v = acc[e];
                ss = fmaf(v, v, ss);
                row[c * SS + e] = v;
            }
        }
    }

    // ---- 1 / max(||row||, eps) as unit_rows_kernel: every lane scales the elements it wrote itself
    const float inv = 1.f / fmaxf(sqrtf(nn_block_sum(ss, s_part, t)), a.eps);
    if (a.S == 0) {
        const bool vec = ((uintptr_t)row & 15u) == 0;
        for (int g = t; 4 * (int64_t)g < D; g += NN_THREADS) {
            const int e0 = 4 * g, cnt = D - e0 < 4 ? D - e0 : 4;
            if (vec && cnt == 4) {
                const float4 v = load4(row + e0);
                store4(row + e0, make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv));
            } else {
                for (int j = 0; j < cnt; ++j) row[e0 + j] *= inv;
            }
        }
    } else {
        const int SS = a.S * a.S;
        for (int c = 0; c < a.C; ++c)
            for (int e = t; e < SS; e += NN_THREADS) row[c * SS + e] *= inv;
    }
    for (int64_t i = D + t; i < a.row_ld; i += NN_THREADS) row[i] = 0.f;
}

// torch.max(dim=0)'s order on (value, row) as col_argmax_kernel (eval.hip) has it: a NaN beats every number, among equals (two NaNs
// count as equal) the FIRST row wins.  Row -1 is the carried result of the chunks before.
__device__ __forceinline__ bool nn_takes(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn || v == bv) return i < bi;
    return v > bv;
}
__global__ __launch_bounds__(256) void nn_col_argmax_kernel(const float* S, const float* S_aug, const uint8_t* row_aug, int M, int B,
                                                             int64_t ld, int64_t row0, int carry, float* val, int64_t* idx) {
    const int b = blockIdx.x, t = threadIdx.x;
    float best = -__builtin_inff();
    int bi = 0x7fffffff;
    if (carry && t == 0) { best = val[b]; bi = -1; }
    for (int m = t; m < M; m += 256) {
        float v = S[(int64_t)m * ld + b];
        if (S_aug && (!row_aug || row_aug[m])) {
            const float u = S_aug[(int64_t)m * ld + b];
            v = (v != v || u != u) ? __builtin_nanf("") : fmaxf(v, u);
        }
        if (nn_takes(v, m, best, bi)) { best = v; bi = m; }
    }
    __shared__ float sv[256];
    __shared__ int si[256];
    sv[t] = best; si[t] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const float v = sv[t + o];
            const int i = si[t + o];
            if (nn_takes(v, i, sv[t], si[t])) { sv[t] = v; si[t] = i; }
        }
        __syncthreads();
    }
    if (t == 0 && si[0] >= 0) { val[b] = sv[0]; idx[b] = row0 + si[0]; }
}

}  // namespace mdm
using namespace mdm;

// torch's tap tables (aten UpSampleKernel: _compute_indices_min_size_weights_aa for antialias, compute_source_index_and_lambda
// without).  Contraction is off for the whole function: a fused multiply-add in `c` moves a boundary by an ulp.
#pragma clang fp contract(off)
extern "C" int mdm_nn_plan(int n_in, int n_out, int antialias, int32_t* first, int32_t* count, float* weight, int max_taps) {
    MDM_REQUIRE(n_in > 0 && n_out > 0, "nn_plan: n_in and n_out must be positive (%d, %d)", n_in, n_out);
    const int given = (first != nullptr) + (count != nullptr) + (weight != nullptr);
    MDM_REQUIRE(given == 0 || given == 3, "nn_plan: first, count and weight are given together or not at all");
    const double scale = (double)n_in / (double)n_out;
    const double support = scale < 1.0 ? 1.0 : scale, inv = 1.0 / support;
    for (int pass = 0; pass < 2; ++pass) {          // pass 0 counts, pass 1 writes: a refused table writes nothing
        int most = 0;
        for (int i = 0; i < n_out; ++i) {
            int lo, n;
            double w2[2] = {0.0, 0.0};
            if (antialias) {
                const double c = scale * (i + 0.5);
                lo = (int)(c - support + 0.5);
                if (lo < 0) lo = 0;
                int hi = (int)(c + support + 0.5);
                if (hi > n_in) hi = n_in;
                n = hi - lo;
                if (n < 0) n = 0;
                if (pass) {
                    auto wgt = [&](int j) {
                        double x = (j - c + 0.5) * inv;
                        if (x < 0.0) x = -x;
                        return x < 1.0 ? 1.0 - x : 0.0;
                    };
                    double total = 0.0;
                    for (int j = lo; j < lo + n; ++j) total += wgt(j);
                    for (int j = 0; j < n; ++j) {
                        double w = wgt(lo + j);
                        if (total != 0.0) w /= total;
                        weight[(size_t)i * max_taps + j] = (float)w;
                    }
                }
            } else {
                double s = scale * (i + 0.5) - 0.5;
                if (s < 0.0) s = 0.0;
                int j0 = (int)s;
                if (j0 > n_in - 1) j0 = n_in - 1;
                const int j1 = j0 + 1 < n_in ? j0 + 1 : n_in - 1;
                const double l1 = s - j0;
                lo = j0;
                n = j1 == j0 ? 1 : 2;
                w2[0] = n == 1 ? (1.0 - l1) + l1 : 1.0 - l1;
                w2[1] = l1;
                if (pass)
                    for (int j = 0; j < n; ++j) weight[(size_t)i * max_taps + j] = (float)w2[j];
            }
            if (n > most) most = n;
            if (pass) {
                for (int j = n; j < max_taps; ++j) weight[(size_t)i * max_taps + j] = 0.f;
                first[i] = lo;
                count[i] = n;
            }
        }
        if (!given) return most;
        if (pass) return most;
        MDM_REQUIRE(max_taps >= most, "nn_plan: max_taps %d is below the %d taps of %d -> %d", max_taps, most, n_in, n_out);
    }
    return -1;
}

extern "C" int mdm_nn_rows(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                           int64_t first, int R, int normalize, int flip, int S,
                           const int32_t* hfirst, const int32_t* hcount, const float* hweight, int htaps,
                           const int32_t* vfirst, const int32_t* vcount, const float* vweight, int vtaps,
                           float eps, float* rows, int64_t row_ld, void* stream) {
    MDM_REQUIRE(src, "nn_rows: src is NULL");
    MDM_REQUIRE(rows, "nn_rows: rows is NULL");
    MDM_REQUIRE(kind == 0 || kind == 1, "nn_rows: kind %d is not 0 (float) or 1 (uint8)", kind);
    MDM_REQUIRE(kind == 0 || lut, "nn_rows: kind 1 needs lut");
    MDM_REQUIRE(M > 0, "nn_rows: M must be positive (%lld)", (long long)M);
    MDM_REQUIRE(R > 0, "nn_rows: R must be positive (%d)", R);
    MDM_REQUIRE(C > 0 && H > 0 && W > 0, "nn_rows: C, H, W must be positive (%d, %d, %d)", C, H, W);
    MDM_REQUIRE(S >= 0, "nn_rows: S %d is negative", S);
    MDM_REQUIRE((int64_t)C * H * W <= INT32_MAX, "nn_rows: C H W = %lld is past 2^31 - 1", (long long)((int64_t)C * H * W));
    MDM_REQUIRE(img_stride >= (int64_t)C * H * W, "nn_rows: img_stride %lld < C H W", (long long)img_stride);
    MDM_REQUIRE(first >= 0, "nn_rows: first %lld is negative", (long long)first);
    MDM_REQUIRE(first + R <= M, "nn_rows: first + R = %lld is past M = %lld", (long long)(first + R), (long long)M);
    NnArgs a;
    memset(&a, 0, sizeof a);
    size_t lds = 256 * sizeof(float);
    int64_t D = (int64_t)C * H * W;
    if (S > 0) {
        MDM_REQUIRE(hfirst && hcount && hweight && vfirst && vcount && vweight, "nn_rows: S > 0 needs the two axis tables");
        MDM_REQUIRE(htaps >= 1 && vtaps >= 1, "nn_rows: htaps and vtaps must be positive (%d, %d)", htaps, vtaps);
        MDM_REQUIRE(S <= NN_MAX_S, "nn_rows: S = %d: the S S accumulators of a channel are kept in LDS up to S = %d", S, NN_MAX_S);
        MDM_REQUIRE(W < NN_TILE, "nn_rows: a source row of W = %d floats does not fit the LDS tile of %d", W, NN_TILE);
        MDM_REQUIRE((int64_t)S * htaps <= NN_HTABLE, "nn_rows: the horizontal table of %d x %d weights does not fit the %d floats of LDS kept for it",
                    S, htaps, NN_HTABLE);
        D = (int64_t)C * S * S;
        MDM_REQUIRE(D <= INT32_MAX, "nn_rows: C S S = %lld is past 2^31 - 1", (long long)D);
        a.P = W | 1;
        a.TR = NN_TILE / a.P;
        if (a.TR > NN_TILE / S) a.TR = NN_TILE / S;
        if (a.TR > H) a.TR = H;
        a.HP = a.TR | 1;
        lds += ((size_t)a.TR * a.P + (size_t)S * a.HP + (size_t)S * S + (size_t)S * htaps + 2 * (size_t)S) * sizeof(float);
    }
    MDM_REQUIRE(row_ld >= D, "nn_rows: row_ld %lld < D = %lld", (long long)row_ld, (long long)D);
    a.src = src; a.lut = lut; a.rows = rows;
    a.hfirst = hfirst; a.hcount = hcount; a.hweight = hweight; a.vfirst = vfirst; a.vcount = vcount; a.vweight = vweight;
    a.img_stride = img_stride; a.first = first; a.row_ld = row_ld;
    a.C = C; a.H = H; a.W = W; a.S = S; a.htaps = htaps; a.vtaps = vtaps; a.normalize = normalize != 0; a.flip = flip != 0;
    a.eps = eps;
    if (kind == 0) hipLaunchKernelGGL(nn_rows_kernel<0>, dim3((unsigned)R), dim3(NN_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(nn_rows_kernel<1>, dim3((unsigned)R), dim3(NN_THREADS), lds, (hipStream_t)stream, a);
    return launch_status("nn_rows");
}

extern "C" int mdm_nn_col_argmax(const float* S, const float* S_aug, const uint8_t* row_aug, int M, int B, int64_t ld, int64_t row0,
                                 int carry, float* val, int64_t* idx, void* stream) {
    MDM_REQUIRE(S, "nn_col_argmax: S is NULL");
    MDM_REQUIRE(val && idx, "nn_col_argmax: val and idx are both needed");
    MDM_REQUIRE(M > 0 && B > 0, "nn_col_argmax: M and B must be positive (%d, %d)", M, B);
    MDM_REQUIRE(ld >= B, "nn_col_argmax: ld %lld < B = %d", (long long)ld, B);
    MDM_REQUIRE(row0 >= 0, "nn_col_argmax: row0 %lld is negative", (long long)row0);
    hipLaunchKernelGGL(nn_col_argmax_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, S, S_aug, row_aug, M, B, ld, row0, carry != 0, val, idx);
    return launch_status("nn_col_argmax");
}
