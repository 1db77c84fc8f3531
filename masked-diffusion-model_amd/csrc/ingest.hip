// Image ingest (include/mdm_ingest.h): decoded interleaved uint8 images -> the planar uint8 storage of mdm_data.h, resized and
// cropped as PIL's 8-bit bilinear resample and torchvision's centre crop give them, byte for byte.
//
// Replaces the transform of reference utils/mydataset.py:77-83 (Resize, CenterCrop on the PIL image) under MyDataset.__init__
// (:245-265).  mdm_ingest_plan states PIL's coefficient tables on the host; the kernel streams: one workgroup per (image, tile of
// TR output rows) walks the source rows of the tile's vertical span ONCE.  A row is staged in LDS (16-byte loads over its aligned
// middle, the next row while this one is filtered), filtered horizontally once into S C uint8 values -- lane j owns kept column
// j % S of channel j / S -- and each value is added into the int32 accumulators of the output rows whose support holds that source
// row.  The accumulators live in LDS, every lane touches only its own, so LDS is 2 rows + the horizontal table + TR S C words
// whatever the scale factor: 1024 -> 32 (65 taps and more) is the same code as 28 -> 32.  Integer adds, no atomics.
#include "common.h"
#include "../../include/mdm_ingest.h"

#include <math.h>

namespace mdm {

constexpr int INGEST_BITS = 22;                 // PIL's PRECISION_BITS for 8-bit channels
constexpr int INGEST_THREADS = 256;
constexpr int INGEST_MAX_TR = 8;
constexpr int64_t INGEST_LDS = 64 * 1024;

struct IngestArgs {
    const uint8_t* src;
    const int32_t *hbounds, *hcoeffs, *vbounds, *vcoeffs;
    uint8_t* dst;
    int64_t src_stride, dst_stride, first;
    int h, w, C, S, ksh, ksv;
    int TR;             // output rows per workgroup
    int row_bytes;      // one LDS row buffer: w C + 16, rounded up to 16
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// clip8 of PIL: the accumulator shifted down (arithmetic shift), cut to a byte
__device__ __forceinline__ uint32_t ingest_clip8(uint32_t acc) { return (uint32_t)clampi((int32_t)acc >> INGEST_BITS, 0, 255); }

// source row [p, p + len) -> buf[mis + i], mis = p & 15, so that global and LDS addresses are 16-byte aligned together: scalar loads
// up to the first boundary, 16-byte loads over the middle, scalar loads behind it.  Reads exactly the row's bytes.
__device__ __forceinline__ void ingest_stage(const uint8_t* p, int len, uint8_t* buf, int t) {
    const int mis = (int)((uintptr_t)p & 15u);
    int head = (16 - mis) & 15;
    if (head > len) head = len;
    for (int i = t; i < head; i += INGEST_THREADS) buf[mis + i] = p[i];
    const int n16 = (len - head) >> 4;
    const uint4* q = reinterpret_cast<const uint4*>(p + head);
    uint4* b = reinterpret_cast<uint4*>(buf + mis + head);
    for (int i = t; i < n16; i += INGEST_THREADS) b[i] = q[i];
    for (int i = head + 16 * n16 + t; i < len; i += INGEST_THREADS) buf[mis + i] = p[i];
}

// workgroup b = (image k, row tile): blockIdx.x = k tiles + tile.  TABLE_LDS: the horizontal table is copied into LDS (it fits);
// else it is read where it lies -- one body, the address space of the table known at compile time (no flat loads)
template <bool TABLE_LDS> __global__ __launch_bounds__(INGEST_THREADS) void ingest_resize_crop_kernel(IngestArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int t = threadIdx.x;
    const int S = a.S, C = a.C, NJ = S * C, TR = a.TR, w = a.w, h = a.h;
    const int tiles = (S + TR - 1) / TR;
    const int k = blockIdx.x / tiles, r0 = (blockIdx.x - k * tiles) * TR;
    const int rows = S - r0 < TR ? S - r0 : TR;
    const int len = w * C;

    // LDS: [row 0][row 1][TR x NJ accumulators][2 TR vertical bounds][S x 2 bounds, S x ksh coefficients when they fit]
    uint8_t* rowbuf = lds;
    uint32_t* acc = reinterpret_cast<uint32_t*>(lds + 2 * (size_t)a.row_bytes);
    int* vb = reinterpret_cast<int*>(acc + (size_t)TR * NJ);
    int32_t* tb = vb + 2 * TR;
    int32_t* tc = tb + 2 * S;
    if (TABLE_LDS) {
        for (int i = t; i < 2 * S; i += INGEST_THREADS) tb[i] = a.hbounds[i];
        for (int i = t; i < S * a.ksh; i += INGEST_THREADS) tc[i] = a.hcoeffs[i];
    }
    for (int i = t; i < TR * NJ; i += INGEST_THREADS) acc[i] = 1u << (INGEST_BITS - 1);
    // the tile's vertical bounds, clamped: first row into [0, h - 1], taps into [0, ksv]
    if (t < rows) {
        vb[2 * t] = clampi(a.vbounds[2 * (r0 + t)], 0, h - 1);
        vb[2 * t + 1] = clampi(a.vbounds[2 * (r0 + t) + 1], 0, a.ksv);
    }
    __syncthreads();
    int y0 = h, y1 = 0;                                             // the source rows this tile needs: [y0, y1)
    for (int r = 0; r < rows; ++r) {
        const int lo = vb[2 * r], hi = lo + vb[2 * r + 1];
        if (vb[2 * r + 1] > 0) { y0 = lo < y0 ? lo : y0; y1 = hi > y1 ? hi : y1; }
    }
    if (y1 > h) y1 = h;

    const uint8_t* img = a.src + (int64_t)k * a.src_stride;
    if (y0 < y1) ingest_stage(img + (int64_t)y0 * len, len, rowbuf + (size_t)(y0 & 1) * a.row_bytes, t);
    __syncthreads();
    for (int y = y0; y < y1; ++y) {
        // the next row goes into the other buffer while this one is read: one barrier per row
        if (y + 1 < y1) ingest_stage(img + (int64_t)(y + 1) * len, len, rowbuf + (size_t)((y + 1) & 1) * a.row_bytes, t);
        const uint8_t* row = rowbuf + (size_t)(y & 1) * a.row_bytes + (int)((uintptr_t)(img + (int64_t)y * len) & 15u);
        for (int j = t; j < NJ; j += INGEST_THREADS) {
            const int c = j / S, x = j - c * S;
            const int xmin = clampi(TABLE_LDS ? tb[2 * x] : a.hbounds[2 * x], 0, w - 1);
            const int cnt = clampi(TABLE_LDS ? tb[2 * x + 1] : a.hbounds[2 * x + 1], 0, a.ksh);
            const size_t c0 = (size_t)x * a.ksh;
            uint32_t s = 1u << (INGEST_BITS - 1);
            for (int i = 0; i < cnt; ++i) {
                const int sx = xmin + i < w ? xmin + i : w - 1;
                s += (uint32_t)row[sx * C + c] * (uint32_t)(TABLE_LDS ? tc[c0 + i] : a.hcoeffs[c0 + i]);
            }
            const uint32_t v = ingest_clip8(s);                      // the uint8 between the passes
            for (int r = 0; r < rows; ++r) {
                const int d = y - vb[2 * r];
                if (d >= 0 && d < vb[2 * r + 1]) acc[r * NJ + j] += v * (uint32_t)a.vcoeffs[(size_t)(r0 + r) * a.ksv + d];
            }
        }
        __syncthreads();
    }
    uint8_t* out = a.dst + (a.first + k) * a.dst_stride;
    for (int r = 0; r < rows; ++r)
        for (int j = t; j < NJ; j += INGEST_THREADS) {
            const int c = j / S, x = j - c * S;
            out[(size_t)c * S * S + (size_t)(r0 + r) * S + x] = (uint8_t)ingest_clip8(acc[r * NJ + j]);
        }
}

}  // namespace mdm
using namespace mdm;

// PIL's precompute_coeffs (bilinear) + normalize_coeffs_8bpc.  Contraction is off for the whole function: a fused multiply-add in
// `center` moves a boundary by an ulp.  (File scope: it holds for the lambda too; only host integer code follows.)
#pragma clang fp contract(off)
extern "C" int mdm_ingest_plan(int in_size, int out_size, int first, int count, int32_t* bounds, int32_t* coeffs) {
    MDM_REQUIRE(in_size > 0 && out_size > 0, "ingest_plan: in_size and out_size must be positive (%d, %d)", in_size, out_size);
    MDM_REQUIRE(count > 0, "ingest_plan: count must be positive (%d)", count);
    MDM_REQUIRE(first >= 0, "ingest_plan: first %d is negative", first);
    MDM_REQUIRE((int64_t)first + count <= out_size, "ingest_plan: first + count = %lld is past out_size %d", (long long)first + count, out_size);
    MDM_REQUIRE((bounds == nullptr) == (coeffs == nullptr), "ingest_plan: bounds and coeffs are given together or not at all");
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const int ks = 2 * (int)ceil(support) + 1;
    if (!bounds) return ks;
    for (int n = 0; n < count; ++n) {
        const int xx = first + n;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        // a weight is made twice, for the sum and for its own row entry: the same operations give the same double, and no
        // buffer grows with the number of taps
        auto weight = [&](int x) {
            double a = (x + xmin - center + 0.5) / fs;
            if (a < 0.0) a = -a;
            return a < 1.0 ? 1.0 - a : 0.0;
        };
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) ww += weight(x);
        int32_t* k = coeffs + (size_t)n * ks;
        for (int x = 0; x < xmax; ++x) {
            double wgt = weight(x);
            if (ww != 0.0) wgt /= ww;
            k[x] = wgt < 0.0 ? (int32_t)(-0.5 + wgt * (double)(1 << INGEST_BITS)) : (int32_t)(0.5 + wgt * (double)(1 << INGEST_BITS));
        }
        for (int x = xmax < 0 ? 0 : xmax; x < ks; ++x) k[x] = 0;
        bounds[2 * n] = xmin;
        bounds[2 * n + 1] = xmax;
    }
    return ks;
}

// The launch geometry of mdm_ingest_resize_crop, stated once: the launcher takes every number of its launch from here and
// mdm_ingest_launch_of reports the same numbers.  Pure host arithmetic on w, C, S and ksh (the callers have checked them): the row
// tile shrinks from min(S, 8) until two row buffers, its accumulators and its vertical bounds fit the LDS of a workgroup; the
// horizontal table joins them there when it still fits and stays in global memory when it does not.
struct IngestGeometry {
    int tr;             // output rows per workgroup
    bool table_lds;     // the horizontal table is copied into LDS (ingest_resize_crop_kernel<true>)
    int64_t row_bytes;  // one LDS row buffer: w C + 16, rounded up to 16
    int64_t lds;        // dynamic LDS of a workgroup, bytes
    int64_t tiles;      // workgroups per image
};
static int ingest_geometry(int w, int C, int S, int ksh, IngestGeometry& g) {
    const int64_t row_bytes = (((int64_t)w * C + 16) + 15) & ~(int64_t)15;
    const int64_t NJ = (int64_t)S * C;
    // LDS of a workgroup with TR output rows: two row buffers, TR NJ accumulators, 2 TR vertical bounds (+ the horizontal table)
    auto lds_of = [&](int tr) { return 2 * row_bytes + 4 * (tr * NJ + 2 * tr); };
    int tr = S < INGEST_MAX_TR ? S : INGEST_MAX_TR;
    while (tr > 1 && lds_of(tr) > INGEST_LDS) --tr;
    MDM_REQUIRE(lds_of(tr) <= INGEST_LDS,
                "ingest_resize_crop: two rows of w C = %lld bytes and S C = %lld accumulators need %lld bytes of LDS, past %lld",
                (long long)w * C, (long long)NJ, (long long)lds_of(tr), (long long)INGEST_LDS);
    const int64_t table = 4 * (2 * (int64_t)S + (int64_t)S * ksh);
    g.tr = tr;
    g.row_bytes = row_bytes;
    g.table_lds = lds_of(tr) + table <= INGEST_LDS;
    g.lds = lds_of(tr) + (g.table_lds ? table : 0);
    g.tiles = (S + tr - 1) / tr;
    return 0;
}

extern "C" int mdm_ingest_launch_of(int w, int C, int S, int ksh, int32_t out[4]) {
    MDM_REQUIRE(out, "ingest_launch_of: out is NULL");
    MDM_REQUIRE(C == 1 || C == 3, "ingest_launch_of: C = %d is not 1 or 3", C);
    MDM_REQUIRE(w > 0, "ingest_launch_of: w must be positive (%d)", w);
    MDM_REQUIRE(S > 0, "ingest_launch_of: S must be positive (%d)", S);
    MDM_REQUIRE(ksh >= 1, "ingest_launch_of: ksh = %d is below 1", ksh);
    IngestGeometry g;
    if (int rc = ingest_geometry(w, C, S, ksh, g)) return rc;
    out[0] = g.tr; out[1] = g.table_lds ? 1 : 0; out[2] = (int32_t)g.lds; out[3] = (int32_t)g.tiles;
    return 0;
}

extern "C" int mdm_ingest_resize_crop(const uint8_t* src, int64_t src_stride, int K, int h, int w, int C,
                                      const int32_t* hbounds, const int32_t* hcoeffs, int ksh,
                                      const int32_t* vbounds, const int32_t* vcoeffs, int ksv,
                                      uint8_t* dst, int64_t dst_stride, int64_t M, int64_t first, int S, void* stream) {
    MDM_REQUIRE(src, "ingest_resize_crop: src is NULL");
    MDM_REQUIRE(hbounds && hcoeffs, "ingest_resize_crop: hbounds or hcoeffs is NULL");
    MDM_REQUIRE(vbounds && vcoeffs, "ingest_resize_crop: vbounds or vcoeffs is NULL");
    MDM_REQUIRE(dst, "ingest_resize_crop: dst is NULL");
    MDM_REQUIRE(C == 1 || C == 3, "ingest_resize_crop: C = %d is not 1 or 3", C);
    MDM_REQUIRE(K > 0, "ingest_resize_crop: K must be positive (%d)", K);
    MDM_REQUIRE(h > 0 && w > 0, "ingest_resize_crop: h, w must be positive (%d, %d)", h, w);
    MDM_REQUIRE(S > 0, "ingest_resize_crop: S must be positive (%d)", S);
    MDM_REQUIRE(M > 0, "ingest_resize_crop: M must be positive (%lld)", (long long)M);
    MDM_REQUIRE(ksh >= 1, "ingest_resize_crop: ksh = %d is below 1", ksh);
    MDM_REQUIRE(ksv >= 1, "ingest_resize_crop: ksv = %d is below 1", ksv);
    const int64_t in_bytes = (int64_t)h * w * C, out_bytes = (int64_t)C * S * S;
    MDM_REQUIRE(in_bytes <= INT32_MAX, "ingest_resize_crop: h w C = %lld is past 2^31 - 1", (long long)in_bytes);
    MDM_REQUIRE(out_bytes <= INT32_MAX, "ingest_resize_crop: C S S = %lld is past 2^31 - 1", (long long)out_bytes);
    MDM_REQUIRE(src_stride >= in_bytes, "ingest_resize_crop: src_stride %lld < h w C", (long long)src_stride);
    MDM_REQUIRE(dst_stride >= out_bytes, "ingest_resize_crop: dst_stride %lld < C S S", (long long)dst_stride);
    MDM_REQUIRE(first >= 0, "ingest_resize_crop: first %lld is negative", (long long)first);
    MDM_REQUIRE(first <= M - K, "ingest_resize_crop: first + K = %lld is past M = %lld", (long long)(first + K), (long long)M);

    IngestGeometry g;
    if (int rc = ingest_geometry(w, C, S, ksh, g)) return rc;
    IngestArgs a;
    a.src = src; a.hbounds = hbounds; a.hcoeffs = hcoeffs; a.vbounds = vbounds; a.vcoeffs = vcoeffs; a.dst = dst;
    a.src_stride = src_stride; a.dst_stride = dst_stride; a.first = first;
    a.h = h; a.w = w; a.C = C; a.S = S; a.ksh = ksh; a.ksv = ksv;
    a.TR = g.tr; a.row_bytes = (int)g.row_bytes;
    const int64_t blocks = (int64_t)K * g.tiles;
    MDM_REQUIRE(blocks <= INT32_MAX, "ingest_resize_crop: K = %d images of S = %d rows are too many workgroups for one launch", K, S);
    if (g.table_lds) hipLaunchKernelGGL(ingest_resize_crop_kernel<true>, dim3((unsigned)blocks), dim3(INGEST_THREADS), (size_t)g.lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(ingest_resize_crop_kernel<false>, dim3((unsigned)blocks), dim3(INGEST_THREADS), (size_t)g.lds, (hipStream_t)stream, a);
    return launch_status("ingest_resize_crop");
}
