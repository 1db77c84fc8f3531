// Set-moment kernels (include/mdm_moment.h): sum = X^T 1 and outer = X^T X of R feature rows in fp64, on v_mfma_f64_16x16x4_f64.
// Two launches: moment_tile_kernel forms one 64 x 64 tile of the upper triangle over one split of the rows per workgroup and leaves
// it in the caller's workspace; moment_finish_kernel adds a tile's splits in index order, then the carry, and writes the tile and
// its mirror image, a strip of 16 rows per workgroup.  No floating-point atomics: two launches give the same bits.
//
// Upstream has no counterpart.
#include "common.h"
#include "../../include/mdm_moment.h"

namespace mdm {

constexpr int MO_TILE = 64;                        // outputs along an edge of a tile
constexpr int MO_KB = 16;                          // rows staged per barrier pair: four steps of the K = 4 instruction
constexpr int MO_LP = 80;                          // LDS pitch of a staged row in doubles: the four rows (k = lane >> 4) of one operand
                                                   // read start 160 dwords apart, on both halves of the 64 banks (not measured)
constexpr int MO_FS = 16, MO_STRIPS = MO_TILE / MO_FS;   // the combining launch: strips of 16 rows of a tile, so few tiles still fill the device
constexpr int MO_FP = 65;                          // LDS pitch of the combining launch's transpose
constexpr int MO_TARGET_WG = 512;                  // two workgroups per CU of a 256-CU device before the rows stay in one split
constexpr int MO_MAX_D = 8192;
constexpr int MO_TILE_LDS = 2 * MO_KB * MO_LP * 8 + 256 * 4;
constexpr int MO_FINISH_LDS = MO_FS * MO_FP * 8;

typedef double double4_t __attribute__((ext_vector_type(4)));

struct MomentPlan {
    int T, splits;
    int64_t tiles, rps, ws_doubles;
};

static int moment_plan(const char* who, int64_t R, int d, MomentPlan* p) {
    MDM_REQUIRE(R > 0 && d > 0, "%s: R and d must be positive (%lld, %d)", who, (long long)R, d);
    MDM_REQUIRE(d <= MO_MAX_D, "%s: d = %d is past %d", who, d, MO_MAX_D);
    MDM_REQUIRE(R <= (int64_t)1 << 40, "%s: R = %lld is past 2^40", who, (long long)R);
    p->T = cdiv(d, MO_TILE);
    p->tiles = (int64_t)p->T * (p->T + 1) / 2;
    const int64_t want = p->tiles >= MO_TARGET_WG ? 1 : (MO_TARGET_WG + p->tiles - 1) / p->tiles;
    p->rps = ((R + want - 1) / want + MO_KB - 1) / MO_KB * MO_KB;
    p->splits = (int)((R + p->rps - 1) / p->rps);
    p->ws_doubles = (int64_t)p->splits * (p->tiles * MO_TILE * MO_TILE + (int64_t)p->T * MO_TILE);
    return 0;
}

// tile -> (I, J), J >= I: the tiles of row I of the triangle follow those of row I - 1
__host__ __device__ __forceinline__ void moment_tile_of(int tile, int T, int& I, int& J) {
    I = 0;
    while (tile >= T - I) { tile -= T - I; ++I; }
    J = I + tile;
}

// four consecutive columns of one row, widened; what lies past the row range or past d is never loaded and stands as +0
template <int KIND, bool VEC>
__device__ __forceinline__ void moment_load4(const void* rows, const float* s_lut, int64_t row_ld, int64_t r, int64_t r_end, int c, int d,
                                             double* v) {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (r >= r_end || c >= d) return;
    if (KIND == 0) {
        const float* p = (const float*)rows + r * row_ld + c;
        if (VEC && c + 3 < d) {
            const float4 q = load4(p);
            v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < d) v[e] = (double)p[e];
        }
    } else {
        const uint8_t* p = (const uint8_t*)rows + r * row_ld + c;
        if (VEC && c + 3 < d) {
            const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (double)s_lut[(q >> (8 * e)) & 255u];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < d) v[e] = (double)s_lut[p[e]];
        }
    }
}

__device__ __forceinline__ void moment_stage(double* s, int row, int col, const double* v) {
    double2* q = reinterpret_cast<double2*>(s + row * MO_LP + col);         // MO_LP and col are even: 16-byte aligned
    q[0] = make_double2(v[0], v[1]);
    q[1] = make_double2(v[2], v[3]);
}

// VEC: rows is 16-byte (float) / 4-byte (uint8) aligned and row_ld is a multiple of 4 -- four columns from a multiple of 4 are one load
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void moment_tile_kernel(const void* rows, const float* lut, int64_t row_ld, int64_t R, int d, int T,
                                                          int64_t tiles, int64_t rps, double* ws_tile, double* ws_sum) {
    __shared__ double s_a[MO_KB * MO_LP], s_b[MO_KB * MO_LP];
    __shared__ float s_lut[256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tile = (int)(blockIdx.x % tiles);
    const int64_t split = blockIdx.x / tiles;
    int I, J;
    moment_tile_of(tile, T, I, J);
    const bool diag = I == J;
    const int64_t r0 = split * rps, r_end = r0 + rps < R ? r0 + rps : R;
    if (KIND == 1) { s_lut[t] = lut[t]; __syncthreads(); }
    // staging: thread t holds columns 4 (t & 15) .. + 3 of row t >> 4 of both slices
    const int srow = t >> 4, scol = 4 * (t & 15);
    const int ca = I * MO_TILE + scol, cb = J * MO_TILE + scol;
    double va[4], vb[4];
    moment_load4<KIND, VEC>(rows, s_lut, row_ld, r0 + srow, r_end, ca, d, va);
    if (!diag) moment_load4<KIND, VEC>(rows, s_lut, row_ld, r0 + srow, r_end, cb, d, vb);
    const double* sb = diag ? s_a : s_b;
    // wave w owns outputs i in [32 (w >> 1), + 32) x j in [32 (w & 1), + 32): 2 x 2 results of the instruction
    const int wi = 32 * (w >> 1) + (lane & 15), wj = 32 * (w & 1) + (lane & 15), kl = lane >> 4;
    double4_t acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = double4_t{0.0, 0.0, 0.0, 0.0};
    double csum = 0.0;
    for (int64_t rb = r0; rb < r_end; rb += MO_KB) {
        moment_stage(s_a, srow, scol, va);
        if (!diag) moment_stage(s_b, srow, scol, vb);
        __syncthreads();
        if (rb + MO_KB < r_end) {                                      // the next block's loads fly under this block's products
            moment_load4<KIND, VEC>(rows, s_lut, row_ld, rb + MO_KB + srow, r_end, ca, d, va);
            if (!diag) moment_load4<KIND, VEC>(rows, s_lut, row_ld, rb + MO_KB + srow, r_end, cb, d, vb);
        }
#pragma unroll
        for (int kk = 0; kk < MO_KB / 4; ++kk) {
            const int k = 4 * kk + kl;
            // A[i][k] = x[rb + k][64 I + i] on lane (i & 15) + 16 k, B[k][j] = x[rb + k][64 J + j] on lane (j & 15) + 16 k
            const double a0 = s_a[k * MO_LP + wi], a1 = s_a[k * MO_LP + wi + 16];
            const double b0 = sb[k * MO_LP + wj], b1 = sb[k * MO_LP + wj + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (diag && t < MO_TILE) {                                     // the column sums: rows in order, one add each
#pragma unroll
            for (int k = 0; k < MO_KB; ++k) csum += s_a[k * MO_LP + t];
        }
        __syncthreads();
    }
    // C/D of the f64 instruction: column = lane & 15, row = (lane >> 4) + 4 reg
    double* out = ws_tile + ((size_t)split * tiles + tile) * (MO_TILE * MO_TILE);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = 32 * (w >> 1) + 16 * m + kl + 4 * reg, j = 32 * (w & 1) + 16 * n + (lane & 15);
                out[i * MO_TILE + j] = acc[m][n][reg];
            }
    if (diag && t < MO_TILE) ws_sum[(size_t)split * T * MO_TILE + I * MO_TILE + t] = csum;
}

// one workgroup per strip of MO_FS rows of a tile: splits in index order, then the carry; the strip as it lies, then its mirror image
// through LDS.  A diagonal tile uses its elements j >= i only, so both halves of it come from one value too.  Strip 0 of a diagonal
// tile adds the column sums.
__global__ __launch_bounds__(256) void moment_finish_kernel(const double* ws_tile, const double* ws_sum, int splits, int64_t tiles, int T,
                                                            int d, int carry, double* sum, double* outer, int64_t outer_ld) {
    __shared__ double s_t[MO_FS * MO_FP];
    const int t = threadIdx.x, tile = blockIdx.x / MO_STRIPS, strip = blockIdx.x % MO_STRIPS;
    int I, J;
    moment_tile_of(tile, T, I, J);
    const bool diag = I == J;
    const int i0 = I * MO_TILE, j0 = J * MO_TILE, is = strip * MO_FS;
    for (int e = t; e < MO_FS * MO_TILE; e += 256) {
        const int il = e >> 6, i = is + il, j = e & 63;
        if (i0 + i < d && j0 + j < d && (!diag || j >= i)) {
            const size_t at = (size_t)i * MO_TILE + j;
            double v = ws_tile[(size_t)tile * (MO_TILE * MO_TILE) + at];
            for (int s = 1; s < splits; ++s) v += ws_tile[((size_t)s * tiles + tile) * (MO_TILE * MO_TILE) + at];
            double* o = outer + (int64_t)(i0 + i) * outer_ld + (j0 + j);
            if (carry) v = *o + v;
            *o = v;
            s_t[il * MO_FP + j] = v;
        }
    }
    __syncthreads();
    for (int e = t; e < MO_FS * MO_TILE; e += 256) {
        const int a = e / MO_FS, bl = e % MO_FS, b = is + bl;              // outer[j0 + a][i0 + b] = the tile's (i, j) = (b, a)
        if (j0 + a < d && i0 + b < d && (!diag || a > b)) outer[(int64_t)(j0 + a) * outer_ld + (i0 + b)] = s_t[bl * MO_FP + a];
    }
    if (diag && strip == 0 && t < MO_TILE && i0 + t < d) {
        double v = ws_sum[i0 + t];
        for (int s = 1; s < splits; ++s) v += ws_sum[(size_t)s * T * MO_TILE + i0 + t];
        if (carry) v = sum[i0 + t] + v;
        sum[i0 + t] = v;
    }
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_moment_plan(int64_t R, int d, int32_t* tile, int64_t* tiles, int32_t* splits, int64_t* rows_per_split, int64_t* grid,
                               int32_t* lds_bytes) {
    MomentPlan p;
    if (moment_plan("moment_plan", R, d, &p)) return -1;
    if (tile) *tile = MO_TILE;
    if (tiles) *tiles = p.tiles;
    if (splits) *splits = p.splits;
    if (rows_per_split) *rows_per_split = p.rps;
    if (grid) { grid[0] = p.tiles * p.splits; grid[1] = p.tiles * MO_STRIPS; }
    if (lds_bytes) { lds_bytes[0] = MO_TILE_LDS; lds_bytes[1] = MO_FINISH_LDS; }
    return 0;
}

extern "C" int mdm_moment_tile_of(int d, int64_t tile, int32_t* I, int32_t* J) {
    MomentPlan p;
    if (moment_plan("moment_tile_of", 1, d, &p)) return -1;
    MDM_REQUIRE(tile >= 0 && tile < p.tiles, "moment_tile_of: tile = %lld, d = %d has %lld tiles", (long long)tile, d, (long long)p.tiles);
    int i, j;
    moment_tile_of((int)tile, p.T, i, j);
    if (I) *I = i;
    if (J) *J = j;
    return 0;
}

extern "C" int64_t mdm_moment_ws_bytes(int64_t R, int d) {
    MomentPlan p;
    if (moment_plan("moment_ws_bytes", R, d, &p)) return -1;
    return p.ws_doubles * 8;
}

extern "C" int mdm_moment_accumulate(const void* rows, int kind, const float* lut, int64_t row_ld, int64_t R, int d, int carry, double* sum,
                                     double* outer, int64_t outer_ld, void* ws, int64_t ws_bytes, void* stream) {
    MDM_REQUIRE(rows && sum && outer && ws, "moment_accumulate: rows, sum, outer and ws are required");
    MDM_REQUIRE(kind == 0 || kind == 1, "moment_accumulate: kind = %d, 0 (float) or 1 (uint8 through lut)", kind);
    MDM_REQUIRE(kind == 0 || lut, "moment_accumulate: kind 1 reads through lut, which is NULL");
    MomentPlan p;
    if (moment_plan("moment_accumulate", R, d, &p)) return -1;
    MDM_REQUIRE(kind != 0 || ((uintptr_t)rows & 3u) == 0, "moment_accumulate: rows of kind 0 is not 4-byte aligned, the alignment of a float");
    MDM_REQUIRE(row_ld >= d, "moment_accumulate: row_ld = %lld is below d = %d", (long long)row_ld, d);
    MDM_REQUIRE(outer_ld >= d, "moment_accumulate: outer_ld = %lld is below d = %d", (long long)outer_ld, d);
    MDM_REQUIRE(((uintptr_t)sum & 7u) == 0, "moment_accumulate: sum is not 8-byte aligned");
    MDM_REQUIRE(((uintptr_t)outer & 7u) == 0, "moment_accumulate: outer is not 8-byte aligned");
    MDM_REQUIRE(((uintptr_t)ws & 7u) == 0, "moment_accumulate: ws is not 8-byte aligned");
    MDM_REQUIRE(ws_bytes >= p.ws_doubles * 8, "moment_accumulate: ws_bytes = %lld, mdm_moment_ws_bytes asks for %lld", (long long)ws_bytes,
                (long long)(p.ws_doubles * 8));
    MDM_REQUIRE(p.tiles * p.splits <= INT32_MAX, "moment_accumulate: %lld workgroups are past 2^31 - 1", (long long)(p.tiles * p.splits));
    hipStream_t st = (hipStream_t)stream;
    double* ws_tile = (double*)ws;
    double* ws_sum = ws_tile + (int64_t)p.splits * p.tiles * MO_TILE * MO_TILE;
    const bool vec = row_ld % 4 == 0 && ((uintptr_t)rows & (kind == 0 ? 15u : 3u)) == 0;
    const dim3 grid((unsigned)(p.tiles * p.splits)), block(256);
#define MDM_MOMENT_LAUNCH(KIND, VEC) \
    hipLaunchKernelGGL((moment_tile_kernel<KIND, VEC>), grid, block, 0, st, rows, lut, row_ld, R, d, p.T, p.tiles, p.rps, ws_tile, ws_sum)
    if (kind == 0) { if (vec) MDM_MOMENT_LAUNCH(0, true); else MDM_MOMENT_LAUNCH(0, false); }
    else { if (vec) MDM_MOMENT_LAUNCH(1, true); else MDM_MOMENT_LAUNCH(1, false); }
#undef MDM_MOMENT_LAUNCH
    if (int rc = launch_status("moment_accumulate")) return rc;
    hipLaunchKernelGGL(moment_finish_kernel, dim3((unsigned)(p.tiles * MO_STRIPS)), block, 0, st, (const double*)ws_tile, (const double*)ws_sum, p.splits,
                       p.tiles, p.T, d, carry != 0, sum, outer, outer_ld);
    return launch_status("moment_accumulate");
}
