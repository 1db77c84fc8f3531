// GroupNorm(32)+SiLU forward/backward, row softmax, column sums, 2x2 sum-pool,
// NCHW<->NHWC converters.  All HBM-bound streaming kernels over NHWC with 16-byte
// vectors (8 channels) per lane.  Reductions inside a workgroup have a FIXED order (LDS column sums, one thread per
// group); across workgroups the fp32 path goes through per-image partials + a second stage (bit-reproducible), the
// bf16 path through one float atomic per channel per image.
//
// Replaces nn.GroupNorm / nn.SiLU (reference unet6.py:288-293, 358-360), torch.softmax
// (unet6.py:320-322), nn.Upsample backward (unet6.py:472), and the bias / time-embedding
// broadcast backward sums (unet6.py:233, 359).
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace mdm {

// GroupNorm is ONE kernel per direction.  A workgroup owns one image and a block of CBLK channels
// made of whole groups (CBLK = multiple of lcm(C/G, 8), >= 32): pass 1 streams its [P][CBLK] slice
// once for the statistics (lane = fixed 8-channel vector, so per-channel partials stay in registers;
// pixel lanes meet in LDS), pass 2 re-reads the slice (64 KB for the largest unet6 tensor: L2-resident)
// and applies.  No scratch buffers, no zeroing, no atomics on the statistics.
template <typename T>
__device__ __forceinline__ const T* src_ptr(const T* s0, const T* s1, int C0, int C1, int64_t pix, int c) {
    return c < C0 ? s0 + pix * C0 + c : s1 + pix * C1 + (c - C0);
}
// K = the group's first element of that image.  Shifting the sums by it removes the cancellation of
// E[x^2]-mean^2 and makes constant feature maps (a fully degraded, all-zero input image gives them)
// come out with variance exactly 0 and mean exactly K, as the reference's two-pass group_norm does.
template <typename T>
__device__ __forceinline__ float gn_pivot(const T* s0, const T* s1, int C0, int C1, int64_t img_pix0, int grp, int cpg) {
    return Elem<T>::ld(src_ptr(s0, s1, C0, C1, img_pix0, grp * cpg));
}
#define F8_TO_ARR(v) {v.lo.x, v.lo.y, v.lo.z, v.lo.w, v.hi.x, v.hi.y, v.hi.z, v.hi.w}

// Sum over the lanes of a wave that own the same channel vector (lane ids congruent mod VB, VB a power of two):
// butterfly over the offsets VB, 2VB, ... 32.  Afterwards lanes 0..VB-1 hold the wave's totals, and only those
// touch LDS -- 64 lanes adding to one LDS address with ds_add_f32 would serialise completely.
// ---- workgroup column sums through LDS.  Every thread holds K partial values; thread t belongs to column
// v = t % VB (its 8-channel vector) and the sums run over the 256/VB pixel lanes of each column.
// (The first version reduced with __shfl_xor: 4 ds_bpermute round trips per value, 128 per thread in the
// backward -- 20k cycles of a 36k-cycle kernel.)  scratch: K * CS_PITCH floats; out[k * VB + v].
// Column sums inside the wave by RECURSIVE HALVING (VB a power of two: the lanes of a column are those with equal low log2(VB) bits):
// at the step over lane bit b a lane keeps one half of the quantities it still holds (the upper half where its bit is set), sends the
// other half to its partner and adds what the partner sends -- K/2 + K/4 + ... <= K - 1 ds_bpermute per lane for ALL K quantities
// (the plain butterfly of the first version needed log2(lanes) per quantity: 128 in the backward), after which lane l holds quantity
// q0(l) (+ r, r < K >> steps) summed over its column's lanes of this wave.  Those K * VB values per wave go to LDS ([wave][k][v]) and
// K * VB threads add the waves up in ascending order.  LDS traffic: NT/64 * K * VB floats instead of K * NT.
template <int K, int S>
__device__ __forceinline__ void colsum_halving_step(float (&cur)[K], int& q0, int l, int vsh) {
    const int bitpos = vsh + S;
    if (bitpos < 6) {                                                 // uniform
        const int mask = 1 << bitpos;
        const bool up = (l >> bitpos) & 1;
        constexpr int n = (K >> S) > 1 ? (K >> S) : 1;                // quantities a lane holds in front of step S
        if constexpr (n > 1) {
            constexpr int half = n / 2;
#pragma unroll
            for (int j = 0; j < half; ++j) {
                const float send = up ? cur[j] : cur[half + j];
                const float keep = up ? cur[half + j] : cur[j];
                cur[j] = keep + __shfl_xor(send, mask, 64);
            }
            q0 += up ? half : 0;
        } else {
            cur[0] += __shfl_xor(cur[0], mask, 64);
        }
    }
}
template <int K, int NT = 256>
__device__ __forceinline__ void block_colsum_shfl(const float (&val)[K], float* scratch, float* out, int t, int VB) {
    static_assert((K & (K - 1)) == 0 && K >= 8, "block_colsum_shfl: K a power of two");
    const int l = t & 63, w = t >> 6, v = l & (VB - 1);
    const int vsh = __builtin_ctz(VB);                               // uniform
    float cur[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cur[k] = val[k];
    int q0 = 0;
    colsum_halving_step<K, 0>(cur, q0, l, vsh); colsum_halving_step<K, 1>(cur, q0, l, vsh); colsum_halving_step<K, 2>(cur, q0, l, vsh);
    colsum_halving_step<K, 3>(cur, q0, l, vsh); colsum_halving_step<K, 4>(cur, q0, l, vsh); colsum_halving_step<K, 5>(cur, q0, l, vsh);
    const int steps = 6 - vsh;
    const int R = (K >> steps) > 1 ? (K >> steps) : 1;               // quantities left per lane (K >> steps == 0: duplicates, same value)
    constexpr int RMAX = (K >> 3) > 1 ? (K >> 3) : 1;                // VB <= 8
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
        if (r < R) scratch[(w * K + q0 + r) * VB + v] = cur[r];
    __syncthreads();
    if (t < K * VB) {
        float sum = 0.f;
#pragma unroll
        for (int ww = 0; ww < NT / 64; ++ww) sum += scratch[ww * K * VB + t];
        out[t] = sum;
    }
    __syncthreads();
}
// SHFL: the bf16 kernels (measured: step 3.528 -> 3.502 ms); the fp32-storage forward of the reverse sampler keeps the LDS sums (its
// lanes hold 8 NP fp32 registers of the slice: with the halving's K more the sampler read 5.36 - 5.47 against 5.33 ms per reverse step)
template <int K, int NT = 256, bool SHFL = true>
__device__ __forceinline__ void block_colsum(const float (&val)[K], float* scratch, float* out, int t, int VB, int PL) {
    if (SHFL && (VB & (VB - 1)) == 0 && VB <= 8) {     // uniform
        block_colsum_shfl<K, NT>(val, scratch, out, t, VB);
        return;
    }
    constexpr int CS_PITCH = NT + 4;
#pragma unroll
    for (int k = 0; k < K; ++k) scratch[k * CS_PITCH + t] = val[k];
    __syncthreads();
    const int cols = K * VB;                       // <= 256
    int tpc = 1, tpc_sh = 0;                       // threads per column (power of two)
    while (tpc * 2 * cols <= NT) { tpc *= 2; ++tpc_sh; }
    const int col = t >> tpc_sh, part = t - (col << tpc_sh);
    float sum = 0.f;
    if (col < cols) {
        const int k = div_small(col, rcp_small(VB)), v = col - k * VB;
        // the tpc threads of a column take the pixel lanes INTERLEAVED (l = part, part + tpc, ...): neighbouring lanes then
        // read neighbouring LDS words.  (Contiguous shares put the threads of a column a multiple of 64 words apart --
        // 8-way bank conflicts, 62 % of the GroupNorm kernels' LDS cycles by SQ_LDS_BANK_CONFLICT.)
        const float* src = scratch + k * CS_PITCH + v;
        for (int l = part; l < PL; l += tpc) sum += src[l * VB];
    }
    for (int o = 1; o < tpc; o <<= 1) sum += __shfl_xor(sum, o, 64);     // <= 3 steps on ONE value
    if (col < cols && part == 0) out[col] = sum;
    __syncthreads();
}

// out[w] = sum over the `cpg` consecutive channels lc0 .. lc0+cpg-1 (local to the workgroup's channel block) of quantity w of
// block_colsum's output: quantity w of channel lc sits at csum[(w * qstride + (lc & 7)) * VB + (lc >> 3)].
// One thread, ascending channel order.
template <int NQ>
__device__ __forceinline__ void group_sums(const float* csum, int VB, int lc0, int cpg, int qstride, float* out) {
    float a[NQ];
#pragma unroll
    for (int w = 0; w < NQ; ++w) a[w] = 0.f;
    for (int j = 0; j < cpg; ++j) {
        const int lc = lc0 + j, vv = lc >> 3, e = lc & 7;
#pragma unroll
        for (int w = 0; w < NQ; ++w) a[w] += csum[(w * qstride + e) * VB + vv];
    }
#pragma unroll
    for (int w = 0; w < NQ; ++w) out[w] = a[w];
}

// ---- dropout on the output of a residual block's norm2 (nn.Dropout between silu(norm2(.)) and conv2, unet6.py:354, 360), fused into
// the standalone GroupNorm kernels: no extra pass over memory and no stored mask.  Element e = (n P + p) C + c of dropout site k has
// the global index g = base_k + e (base_k: the host's running element count of the sites before it, a multiple of 8); its random word
// is the 16-bit lane g & 7 of philox_at(rng, 5, g >> 3) (lane j = half j & 1 of 32-bit word j >> 1, low half first): ONE Philox call
// per 16-byte bf16 vector.  Kept iff lane >= thr; kept values are multiplied by scale = 65536 / (65536 - thr), dropped ones are exact
// zeros.  ctl = {uint32 thr, float scale} lives in device memory (eval mode rewrites it to {0, 1.0f} under plans and graphs that are
// already recorded); thr == 0 skips the Philox work (a uniform branch).  The forward masks y in registers before the store, the
// backward masks dy right behind its load -- from the same (seed, offset, g), so both see the same mask and none is stored.
__device__ __forceinline__ uint4 drop_keep_bits(const uint64_t* rng, uint64_t g, uint32_t thr) {      // 0xffff per kept lane
    const uint4 r = philox_at(rng, 5, g >> 3);
    auto m = [&](uint32_t w) { return ((w & 0xffffu) >= thr ? 0x0000ffffu : 0u) | ((w >> 16) >= thr ? 0xffff0000u : 0u); };
    return make_uint4(m(r.x), m(r.y), m(r.z), m(r.w));
}
__device__ __forceinline__ void drop_apply(float (&v)[8], const uint4& k, float scale) {
    const uint32_t kw[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ((kw[e >> 1] >> ((e & 1) * 16)) & 1u) ? v[e] * scale : 0.f;
}
__device__ __forceinline__ void drop_apply(float8& d, const uint4& k, float scale) {
    float v[8] = F8_TO_ARR(d);
    drop_apply(v, k, scale);
    d.lo = make_float4(v[0], v[1], v[2], v[3]); d.hi = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- register-cached variants (bf16): a lane's share of the slice is at most NP 16-byte vectors per tensor,
// so it is loaded ONCE (all NP loads in flight together), kept in registers across the statistics and the
// apply pass, and global memory sees a single read.  Same arithmetic as the streaming kernels above.
__device__ __forceinline__ float8 unpack8(const uint4& r) {
    float8 o;
    o.lo = make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u),
                       __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u));
    o.hi = make_float4(__uint_as_float(r.z << 16), __uint_as_float(r.z & 0xffff0000u),
                       __uint_as_float(r.w << 16), __uint_as_float(r.w & 0xffff0000u));
    return o;
}

#ifdef MDM_STAMP
__device__ unsigned long long g_nstamp_buf[4096 * 16];
__device__ __forceinline__ unsigned long long nstamp_now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define MDM_T(...) __VA_ARGS__
#else
#define MDM_T(...)
#endif

// MODE 0, the only one instantiated: the whole GroupNorm in one workgroup per (image, channel block).  Large maps leave few such
// workgroups to pull HBM bandwidth (128 for a 32x32x128 map: 14/24 us fwd/bwd against ~6/9 us of traffic).  MODE 1 / 2 cut the
// pixels into gridDim.z chunks (statistics of one chunk -> partials in ws, then an apply launch); the pair was measured no faster
// than the single launch at cfg2 (13.4 vs 13.7 us forward, 25.3 vs 24.1 us backward on 32x32x128) and nothing launches it.  Its
// text stays in the kernels: without it the same arithmetic compiles to a schedule that measured slower on the step
// (profiles/r13_gn_routes.md: gn_fwd_reg_kernel<1,256> 5.2 -> 5.7 us, gn_bwd_reg_kernel<8,512> 40.8 -> 42.9 us).
// NT = threads per workgroup: 512 on the larger slices (the kernels are VALU- and latency-bound at one wave per SIMD:
// twice the waves per workgroup halve each thread's serial share of exp / rcp work)
// (T = float, round 3: the fp32 forward -- the reverse sampler -- ran on the streaming kernel, two reads and a write per element;
//  a lane's share of 8 channels x NP pixels is NP float8, 8 NP registers.)
template <typename T> struct RegVec;
template <> struct RegVec<bf16_t> {
    typedef uint4 type;
    static __device__ __forceinline__ uint4 zero() { return make_uint4(0, 0, 0, 0); }
    static __device__ __forceinline__ uint4 ld(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
    static __device__ __forceinline__ float8 unpack(const uint4& r) { return unpack8(r); }
};
template <> struct RegVec<float> {
    typedef float8 type;
    static __device__ __forceinline__ float8 zero() { return {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}; }
    static __device__ __forceinline__ float8 ld(const float* p) { return load8(p); }
    static __device__ __forceinline__ float8 unpack(const float8& r) { return r; }
};

// ---- the four standalone kernels (gn_fwd_kernel, gn_bwd_kernel, gn_fwd_reg_kernel, gn_bwd_reg_kernel), once as they are and
// once with dropout (gn_*_kernel_drop): gn_kernels.inc
#define GN_DROP 0
#define GN_K(name) name
#define GN_DROP_PARAMS
#define GN_LOAD_DY(pix) load8(dy + (pix) * C + c)
#define GN_DZ(v) v
#include "gn_kernels.inc"
#undef GN_DROP
#undef GN_K
#undef GN_DROP_PARAMS
#undef GN_LOAD_DY
#undef GN_DZ
#define GN_DROP 1
#define GN_K(name) name##_drop
#define GN_DROP_PARAMS , const uint64_t* rng, uint64_t dbase, const uint32_t* ctl
#define GN_LOAD_DY(pix) load_dy(pix)
#define GN_DZ(v) ((v) * dscale)
#include "gn_kernels.inc"
#undef GN_DROP
#undef GN_K
#undef GN_DROP_PARAMS
#undef GN_LOAD_DY
#undef GN_DZ

// second stage of the fixed-order GroupNorm backward over part[img][{dgamma, dbeta, colsum(dx)}][C]: dgamma[c] += sum_img
// part[img][0][c], dbeta[c] += sum_img part[img][1][c], sum_all[c] += sum_img part[img][2][c], images in ascending order
// (one thread per channel)
__global__ __launch_bounds__(256) void gn_param_reduce_kernel(const float* part, int N, int C, float* dgamma, float* dbeta, float* sum_all) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, b = 0.f, s = 0.f;
    for (int n = 0; n < N; ++n) {
        a += part[((int64_t)n * 3) * C + c];
        b += part[((int64_t)n * 3 + 1) * C + c];
        if (sum_all) s += part[((int64_t)n * 3 + 2) * C + c];
    }
    dgamma[c] += a; dbeta[c] += b;
    if (sum_all) sum_all[c] += s;
}


// keep flags of n consecutive elements from global index `base` on (tests, debugging): one thread per 8-element vector
__global__ __launch_bounds__(256) void dropout_mask_kernel(const uint64_t* rng, uint64_t base, const uint32_t* ctl, int64_t n, uint8_t* keep) {
    const uint32_t thr = ctl[0];
    const uint64_t v = (base >> 3) + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v * 8 >= base + (uint64_t)n) return;
    const uint4 k = thr ? drop_keep_bits(rng, v * 8, thr) : make_uint4(~0u, ~0u, ~0u, ~0u);
    const uint32_t kw[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t g = v * 8 + j;
        if (g >= base && g < base + (uint64_t)n) keep[g - base] = (kw[j >> 1] >> ((j & 1) * 16)) & 1u;
    }
}

// ---- row softmax: one wave per row
template <typename T>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(T* S, int rows, int L) {
    int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    T* p = S + (int64_t)row * L;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, Elem<T>::ld(p + j));
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < L; j += 64) sum += __expf(Elem<T>::ld(p + j) - mx);
    sum = wave_sum(sum);
    float inv = 1.f / sum;
    for (int j = lane; j < L; j += 64) Elem<T>::st(p + j, __expf(Elem<T>::ld(p + j) - mx) * inv);
}
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const T* Pm, T* dP, int rows, int L) {
    int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T* p = Pm + (int64_t)row * L;
    T* g = dP + (int64_t)row * L;
    float dot = 0.f;
    for (int j = lane; j < L; j += 64) dot = fmaf(Elem<T>::ld(p + j), Elem<T>::ld(g + j), dot);
    dot = wave_sum(dot);
    for (int j = lane; j < L; j += 64) Elem<T>::st(g + j, Elem<T>::ld(p + j) * (Elem<T>::ld(g + j) - dot));
}

// ---- column sums of dY[N][P][C]: per_img[n][c] (=|+=) sum_p dY[n][p][c], dbias[c] += sum_n sum_p dY[n][p][c].
// A workgroup owns 64 channels (8 vectors x 32 pixel lanes) of `imgs` consecutive images and walks them in order, so that
// with imgs = N (the fp32 path) dbias has ONE writer per channel and a fixed summation order; with imgs = 1 (bf16: more
// workgroups) the images meet through one float atomic per channel per image.
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* dY, int P, int C, float* per_img, int ld, int acc_img, float* dbias,
                                                     int imgs, int N) {
    __shared__ float red[32][65];
    const int t = threadIdx.x;
    const int v = blockIdx.x * 8 + (t & 7), lanep = t >> 3;      // 8 vectors x 32 pixel lanes
    float total = 0.f;
    for (int img = blockIdx.y * imgs; img < min(N, (int)(blockIdx.y + 1) * imgs); ++img) {
        float s[8] = {};
        if (v * 8 < C) {
            for (int p = lanep; p < P; p += 32) {
                float8 x = load8(dY + ((int64_t)img * P + p) * C + v * 8);
                s[0] += x.lo.x; s[1] += x.lo.y; s[2] += x.lo.z; s[3] += x.lo.w;
                s[4] += x.hi.x; s[5] += x.hi.y; s[6] += x.hi.z; s[7] += x.hi.w;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[lanep][(t & 7) * 8 + e] = s[e];
        __syncthreads();
        if (t < 64) {
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < 32; ++r) a += red[r][t];
            const int c = blockIdx.x * 64 + t;
            if (c < C && per_img) {
                float* q = per_img + (int64_t)img * ld + c;
                *q = acc_img ? *q + a : a;
            }
            total += a;
        }
        __syncthreads();
    }
    if (t < 64) {
        const int c = blockIdx.x * 64 + t;
        if (c < C && dbias) {
            if (imgs >= N) dbias[c] += total;            // single writer
            else atomicAdd(&dbias[c], total);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sumpool2_kernel(const T* g, T* dst, int acc, int H, int W, int C, int64_t total_vec) {
    const int VPP = C / 8;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t pix, img;
        int c, x, y;
        if (total_vec < (1ll << 31)) {          // 32-bit quotients (a 64-bit division is ~100 instructions)
            const unsigned iu = (unsigned)i, pu = iu / (unsigned)VPP, ru = pu / (unsigned)W, mu = ru / (unsigned)H;
            pix = pu; c = (int)(iu - pu * (unsigned)VPP) * 8; x = (int)(pu - ru * (unsigned)W); y = (int)(ru - mu * (unsigned)H); img = mu;
        } else {
            pix = i / VPP;
            c = (int)(i - pix * VPP) * 8;
            x = (int)(pix % W);
            const int64_t r = pix / W;
            y = (int)(r % H);
            img = r / H;
        }
        const T* base = g + (((img * 2 * H + 2 * y) * 2 * W) + 2 * x) * (int64_t)C + c;
        float8 a = load8(base), b = load8(base + C), cc = load8(base + (int64_t)2 * W * C), dd = load8(base + (int64_t)2 * W * C + C);
        float8 o;
        o.lo = make_float4(a.lo.x + b.lo.x + cc.lo.x + dd.lo.x, a.lo.y + b.lo.y + cc.lo.y + dd.lo.y,
                           a.lo.z + b.lo.z + cc.lo.z + dd.lo.z, a.lo.w + b.lo.w + cc.lo.w + dd.lo.w);
        o.hi = make_float4(a.hi.x + b.hi.x + cc.hi.x + dd.hi.x, a.hi.y + b.hi.y + cc.hi.y + dd.hi.y,
                           a.hi.z + b.hi.z + cc.hi.z + dd.hi.z, a.hi.w + b.hi.w + cc.hi.w + dd.hi.w);
        T* q = dst + pix * C + c;
        if (acc) {
            float8 old = load8(q);
            o.lo.x += old.lo.x; o.lo.y += old.lo.y; o.lo.z += old.lo.z; o.lo.w += old.lo.w;
            o.hi.x += old.hi.x; o.hi.y += old.hi.y; o.hi.z += old.hi.z; o.hi.w += old.hi.w;
        }
        store8(q, o);
    }
}

// ---- resample_with_conv=False (unet6.py:441-442, 472-475): the 2x2 average pool and the bare nearest x2 upsample.  Pure streaming
// kernels, one 8-channel vector of the SMALL map per lane: vector i of [N][H][W][C/8] <-> the 2x2 block of [N][2H][2W][C] it pairs with.
struct Quad { int64_t small, big; };        // element offsets of the vector in the small map and of the block's top-left vector
__device__ __forceinline__ Quad quad_of(int64_t i, int64_t total_vec, int H, int W, int C) {
    const int VPP = C / 8;
    int64_t pix, img;
    int c, x, y;
    if (total_vec < (1ll << 31)) {              // 32-bit quotients, as sumpool2_kernel
        const unsigned iu = (unsigned)i, pu = iu / (unsigned)VPP, ru = pu / (unsigned)W, mu = ru / (unsigned)H;
        pix = pu; c = (int)(iu - pu * (unsigned)VPP) * 8; x = (int)(pu - ru * (unsigned)W); y = (int)(ru - mu * (unsigned)H); img = mu;
    } else {
        pix = i / VPP;
        c = (int)(i - pix * VPP) * 8;
        x = (int)(pix % W);
        const int64_t r = pix / W;
        y = (int)(r % H);
        img = r / H;
    }
    return {pix * C + c, (((img * 2 * H + 2 * y) * 2 * W) + 2 * x) * (int64_t)C + c};
}
__device__ __forceinline__ float8 scale8(float s, const float8& v) {
    float8 r;
    r.lo = make_float4(s * v.lo.x, s * v.lo.y, s * v.lo.z, s * v.lo.w);
    r.hi = make_float4(s * v.hi.x, s * v.hi.y, s * v.hi.z, s * v.hi.w);
    return r;
}
__device__ __forceinline__ float8 axpy8(float s, const float8& v, const float8& o) {      // o + s * v: product and sum each rounded (no fma)
#pragma clang fp contract(off)
    float8 r;
    r.lo = make_float4(s * v.lo.x + o.lo.x, s * v.lo.y + o.lo.y, s * v.lo.z + o.lo.z, s * v.lo.w + o.lo.w);
    r.hi = make_float4(s * v.hi.x + o.hi.x, s * v.hi.y + o.hi.y, s * v.hi.z + o.hi.z, s * v.hi.w + o.hi.w);
    return r;
}

// dst[N][H][W][C] (=|+=) 0.25 * (((a + b) + c) + d) over the 2x2 block of src[N][2H][2W][C]: the taps in sumpool2_kernel's order
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_kernel(const T* src, T* dst, int acc, int H, int W, int C, int64_t total_vec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec; i += (int64_t)gridDim.x * blockDim.x) {
        const Quad q = quad_of(i, total_vec, H, W, C);
        const T* base = src + q.big;
        float8 a = load8(base), b = load8(base + C), cc = load8(base + (int64_t)2 * W * C), dd = load8(base + (int64_t)2 * W * C + C);
        float8 s;
        s.lo = make_float4(a.lo.x + b.lo.x + cc.lo.x + dd.lo.x, a.lo.y + b.lo.y + cc.lo.y + dd.lo.y,
                           a.lo.z + b.lo.z + cc.lo.z + dd.lo.z, a.lo.w + b.lo.w + cc.lo.w + dd.lo.w);
        s.hi = make_float4(a.hi.x + b.hi.x + cc.hi.x + dd.hi.x, a.hi.y + b.hi.y + cc.hi.y + dd.hi.y,
                           a.hi.z + b.hi.z + cc.hi.z + dd.hi.z, a.hi.w + b.hi.w + cc.hi.w + dd.hi.w);
        T* o = dst + q.small;
        store8(o, acc ? axpy8(0.25f, s, load8(o)) : scale8(0.25f, s));
    }
}

// dst[N][2H][2W][C] (=|+=) scale * src[N][H][W][C] at the four pixels of the block: ONE load of the source vector, four stores
template <typename T>
__global__ __launch_bounds__(256) void upsample2_kernel(const T* src, T* dst, int acc, float scale, int H, int W, int C, int64_t total_vec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total_vec; i += (int64_t)gridDim.x * blockDim.x) {
        const Quad q = quad_of(i, total_vec, H, W, C);
        const float8 v = load8(src + q.small);
        T* o = dst + q.big;
        const int64_t row = (int64_t)2 * W * C;
        if (acc) {
            const float8 a = load8(o), b = load8(o + C), cc = load8(o + row), dd = load8(o + row + C);
            store8(o, axpy8(scale, v, a)); store8(o + C, axpy8(scale, v, b));
            store8(o + row, axpy8(scale, v, cc)); store8(o + row + C, axpy8(scale, v, dd));
        } else {
            const float8 r = scale8(scale, v);
            store8(o, r); store8(o + C, r); store8(o + row, r); store8(o + row + C, r);
        }
    }
}

template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* x, T* y, int C, int HW, int Cp, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over N*HW*Cp
    if (i >= total) return;
    int c = (int)(i % Cp);
    int64_t pix = i / Cp;
    int64_t img = pix / HW;
    int p = (int)(pix - img * HW);
    float v = c < C ? x[(img * C + c) * HW + p] : 0.f;
    Elem<T>::st(y + i, v);
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* x, float* y, int C, int HW, int Cp, int64_t total) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over N*C*HW
    if (i >= total) return;
    int p = (int)(i % HW);
    int64_t r = i / HW;
    int c = (int)(r % C);
    int64_t img = r / C;
    y[i] = Elem<T>::ld(x + (img * HW + p) * Cp + c);
}

template <typename T>
__global__ void add_kernel(T* dst, const T* x, const T* y, int64_t nvec) {       // dst = x + y (y == nullptr: copy)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float8 a = load8(x + i * 8);
        if (y) {
            float8 b = load8(y + i * 8);
            a.lo.x += b.lo.x; a.lo.y += b.lo.y; a.lo.z += b.lo.z; a.lo.w += b.lo.w;
            a.hi.x += b.hi.x; a.hi.y += b.hi.y; a.hi.z += b.hi.z; a.hi.w += b.hi.w;
        }
        store8(dst + i * 8, a);
    }
}

// flip = 0, shift = 1: unet6.py:18-34 ([sin | cos], exponent / (half - 1)); flip = 1, shift = 0: diffusers' `Timesteps(
// flip_sin_to_cos=True, downscale_freq_shift=0)` as UNet2DModel builds it ([cos | sin], exponent / half)
__global__ void temb_kernel(const float* t, int N, int dim, int flip, float shift, float* y) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int half = dim / 2;
    if (i >= N * half) return;
    int n = i / half, j = i - n * half;
    float f = expf(-(float)j * (logf(10000.f) / ((float)half - shift)));
    float a = t[n] * f;
    y[n * dim + (flip ? half : 0) + j] = sinf(a);
    y[n * dim + (flip ? 0 : half) + j] = cosf(a);
    if ((dim & 1) && j == 0) y[n * dim + dim - 1] = 0.f;
}
__global__ void silu_fwd_kernel(const float* x, float* y, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { float v = x[i]; y[i] = v / (1.f + expf(-v)); }
}
__global__ void silu_bwd_kernel(const float* x, const float* dy, float* dx, int acc, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float v = x[i], s = 1.f / (1.f + expf(-v));
        float g = dy[i] * s * (1.f + v * (1.f - s));
        dx[i] = acc ? dx[i] + g : g;
    }
}

__global__ void zero_f32_kernel(float* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

static inline int stream_grid(int64_t work_items) {
    int64_t b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace mdm

using namespace mdm;

#define DISPATCH_T(dtype, ...)                                      \
    do {                                                            \
        if ((dtype) == MDM_F32) { typedef float T; __VA_ARGS__; }   \
        else if ((dtype) == MDM_BF16) { typedef bf16_t T; __VA_ARGS__; } \
        else { set_error("bad dtype %d", (dtype)); return -1; }     \
    } while (0)

static int gn_check(int C0, int C1, int G, int N, int P) {
    MDM_REQUIRE(C0 > 0 && C0 % 8 == 0 && C1 >= 0 && C1 % 8 == 0, "groupnorm: channel counts must be multiples of 8 (C0=%d C1=%d)", C0, C1);
    MDM_REQUIRE(G > 0 && G <= 64 && (C0 + C1) % G == 0, "groupnorm: C=%d not divisible by G=%d", C0 + C1, G);
    MDM_REQUIRE((C0 + C1) / 8 <= 256, "groupnorm: C=%d too large", C0 + C1);
    MDM_REQUIRE(N > 0 && P > 0, "groupnorm: bad N/P");
    return 0;
}

// channels per workgroup: whole groups, whole 16-byte vectors, at least 32 channels
static int gn_cblk(int C, int G, int P) {
    int cpg = C / G, l = cpg;
    while (l % 8) l += cpg;            // lcm(cpg, 8)
    // 32 channels per workgroup; 16 on large maps (more workgroups pulling HBM: 12.3 -> 10.1 us forward,
    // 21.0 -> 15.8 us backward on 32x32x128; slower on the small maps, where the launch floor dominates;
    // re-measured at the end of round 2 on the whole step: 8 channels 3.989, 16 channels 3.958, 32 channels 4.008 ms)
    int want = P > 256 ? 16 : 32;
    int cb = l;
    while (cb < want) cb += l;
    return cb > C ? C : cb;
}

// ---- the routes (mdm_gn_route_of / mdm_gn_last_route): which GroupNorm kernel a descriptor runs on.  gn_route is the only
// statement of the rule -- pure host code, no HIP call; mdm_groupnorm_fwd, mdm_groupnorm_bwd and the route queries all ask it.
// Storage type and dropout are not part of a route (the launchers below resolve them), so a dropout site runs on the kernel its
// plain GroupNorm runs on and the fp32 forward on the register kernels of the bf16 one.
enum { GN_FWD_REG = 0, GN_FWD = 5, GN_BWD_REG = 6, GN_BWD = 11, GN_BWD_REDUCE = 12, GN_ROUTES = 13 };      // *_REG: + rung of the ladder
struct GnPlan { int route, cblk, grid_x, grid_y; };
// which: 0 forward, 1 backward -> 0 and *out, or -1 and the message
static int gn_route(int which, const mdm_gn_desc& d, GnPlan* out) {
    MDM_REQUIRE(which == 0 || which == 1, "groupnorm: bad direction %d", which);
    if (int rc = gn_check(d.C0, d.C1, d.G, d.N, d.P)) return rc;
    const int C = d.C0 + d.C1, P = d.P;
    int cblk = gn_cblk(C, d.G, P);
    // fp32 forward on large maps: 32 channels per workgroup = whole 128-byte lines per pixel (16 fp32 channels are 64-byte pieces:
    // 3.0 TB/s on the sampler's 32x32x128 maps), as long as the slice still fits the register-cached kernels
    if (which == 0 && d.dtype == MDM_F32 && P > 256) {
        const int wide = gn_cblk(C, d.G, 256);
        if (cdiv(P, 256 / (wide / 8)) <= 16) cblk = wide;
    }
    MDM_REQUIRE(cblk <= 64 && cblk / (C / d.G) <= 64, "groupnorm: unsupported channel/group combination C=%d G=%d", C, d.G);
    MDM_REQUIRE(d.dtype == MDM_F32 || d.dtype == MDM_BF16, "bad dtype %d", d.dtype);
    const int np = cdiv(P, 256 / (cblk / 8));          // 16-byte vectors per lane of a 256-thread workgroup
    // the register-cached kernels hold up to 16 of them (8 per lane of a 512-thread workgroup): <NP, NT> = <1,256>, <2,256>,
    // <2,512>, <4,512>, <8,512> for np <= 1, 2, 4, 8, 16; the backward has them for bf16 only
    int rung = 0;
    while (np > (1 << rung)) ++rung;
    if (rung <= 4 && (which == 0 || d.dtype == MDM_BF16)) out->route = (which ? GN_BWD_REG : GN_FWD_REG) + rung;
    // fp32 backward: fixed summation order across the images too (per-image partials in ws + a second stage); bf16 large maps: atomics
    else out->route = which == 0 ? GN_FWD : d.dtype == MDM_F32 ? GN_BWD_REDUCE : GN_BWD;
    out->cblk = cblk; out->grid_x = d.N; out->grid_y = cdiv(C, cblk);
    return 0;
}

// ---- the launchers: one per kernel shape, each kernel's argument list written once
// f(T(), bool_constant<DROP>()) for the descriptor's storage type and dropout (desc.rng != NULL: the gn_*_kernel_drop variants)
template <typename F>
static void gn_resolve(const mdm_gn_desc& d, F f) {
    if (d.dtype == MDM_F32) d.rng ? f(float(), std::true_type()) : f(float(), std::false_type());
    else d.rng ? f(bf16_t(), std::true_type()) : f(bf16_t(), std::false_type());
}
// the kernel on the route's grid with the arguments a...; its dropout variant takes the descriptor's rng, drop_base, ctl behind them
template <bool DROP, typename KP, typename KD, typename... A>
static void gn_launch(KP* plain, KD* drop, int nt, const mdm_gn_desc& d, const GnPlan& r, hipStream_t s, A... a) {
    const dim3 grid(r.grid_x, r.grid_y);
    if constexpr (DROP) hipLaunchKernelGGL(drop, grid, dim3(nt), 0, s, a..., d.rng, d.drop_base, d.ctl);
    else hipLaunchKernelGGL(plain, grid, dim3(nt), 0, s, a...);
}
template <typename T, bool DROP, typename KP, typename KD, typename... Ws>
static void gn_fwd_args(KP* plain, KD* drop, int nt, const mdm_gn_desc& d, const GnPlan& r, hipStream_t s, Ws... ws) {      // register kernels: + ws
    gn_launch<DROP>(plain, drop, nt, d, r, s, (const T*)d.src0, d.C0, (const T*)d.src1, d.C1, d.P, d.G, r.cblk, d.eps, d.gamma, d.beta, d.silu,
                    (T*)d.y, d.stats, ws...);
}
template <typename T, bool DROP, typename KP, typename KD>
static void gn_bwd_args(KP* plain, KD* drop, int nt, const mdm_gn_desc& d, const GnPlan& r, hipStream_t s, float* part) {      // register kernels: ws
    gn_launch<DROP>(plain, drop, nt, d, r, s, (const T*)d.src0, d.C0, (const T*)d.src1, d.C1, d.P, d.G, r.cblk, d.gamma, d.beta, d.silu,
                    (const T*)d.dy, d.stats, (T*)d.dst0, (const T*)d.add0, (T*)d.dst1, (const T*)d.add1, (const T*)d.add0b, d.dgamma, d.dbeta,
                    d.sum_img, d.sum_ld, d.sum_all, part);
}
template <int NP, int NT>
static void gn_fwd_reg_launch(const mdm_gn_desc& d, const GnPlan& r, hipStream_t s) {
    gn_resolve(d, [&](auto t, auto drop) {
        typedef decltype(t) T;
        gn_fwd_args<T, decltype(drop)::value>(gn_fwd_reg_kernel<NP, 0, NT, T>, gn_fwd_reg_kernel_drop<NP, 0, NT, T>, NT, d, r, s, d.ws);
    });
}
static void gn_fwd_launch(const mdm_gn_desc& d, const GnPlan& r, hipStream_t s) {
    gn_resolve(d, [&](auto t, auto drop) {
        typedef decltype(t) T;
        gn_fwd_args<T, decltype(drop)::value>(gn_fwd_kernel<T>, gn_fwd_kernel_drop<T>, 256, d, r, s);
    });
}
template <int NP, int NT>
static void gn_bwd_reg_launch(const mdm_gn_desc& d, const GnPlan& r, hipStream_t s) {      // bf16 only
    auto go = [&](auto drop) {
        gn_bwd_args<bf16_t, decltype(drop)::value>(gn_bwd_reg_kernel<NP, 0, NT>, gn_bwd_reg_kernel_drop<NP, 0, NT>, NT, d, r, s, d.ws);
    };
    d.rng ? go(std::true_type()) : go(std::false_type());
}
static void gn_bwd_launch(const mdm_gn_desc& d, const GnPlan& r, hipStream_t s) {
    float* part = r.route == GN_BWD_REDUCE ? d.ws : nullptr;
    gn_resolve(d, [&](auto t, auto drop) {
        typedef decltype(t) T;
        gn_bwd_args<T, decltype(drop)::value>(gn_bwd_kernel<T>, gn_bwd_kernel_drop<T>, 256, d, r, s, part);
    });
    if (part) {
        const int C = d.C0 + d.C1;
        hipLaunchKernelGGL(gn_param_reduce_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, part, d.N, C, d.dgamma, d.dbeta, d.sum_all);
    }
}
static const struct GnRouteRow {
    const char* name;
    void (*launch)(const mdm_gn_desc&, const GnPlan&, hipStream_t);
} kGnRoutes[GN_ROUTES] = {
    {"fwd_reg<1,256>", gn_fwd_reg_launch<1, 256>}, {"fwd_reg<2,256>", gn_fwd_reg_launch<2, 256>}, {"fwd_reg<2,512>", gn_fwd_reg_launch<2, 512>},
    {"fwd_reg<4,512>", gn_fwd_reg_launch<4, 512>}, {"fwd_reg<8,512>", gn_fwd_reg_launch<8, 512>}, {"fwd", gn_fwd_launch},
    {"bwd_reg<1,256>", gn_bwd_reg_launch<1, 256>}, {"bwd_reg<2,256>", gn_bwd_reg_launch<2, 256>}, {"bwd_reg<2,512>", gn_bwd_reg_launch<2, 512>},
    {"bwd_reg<4,512>", gn_bwd_reg_launch<4, 512>}, {"bwd_reg<8,512>", gn_bwd_reg_launch<8, 512>}, {"bwd", gn_bwd_launch},
    {"bwd+reduce", gn_bwd_launch},          // the fp32 backward: the generic kernel, then gn_param_reduce_kernel
};
static thread_local int g_gn_route = -1;

// launches what gn_route names; a refused descriptor launches nothing and leaves no route
static int gn_run(int which, const char* what, const mdm_gn_desc* desc_host, void* stream) {
    g_gn_route = -1;
    MDM_REQUIRE(desc_host != nullptr, "%s: null descriptor", what);
    const mdm_gn_desc& d = *desc_host;
    if (d.rng) {
        MDM_REQUIRE(d.C1 == 0, "%s_dropout: a dropout site has one source (C1=%d)", what, d.C1);
        MDM_REQUIRE(d.ctl, "%s_dropout: null rng / ctl", what);
        MDM_REQUIRE(d.drop_base % 8 == 0, "%s_dropout: base must be a multiple of 8", what);
    }
    GnPlan r;
    if (int rc = gn_route(which, d, &r)) return rc;
    if (which == 1) {
        MDM_REQUIRE(!(d.sum_img || d.sum_all) || d.C1 == 0, "groupnorm_bwd: column sums need a single-source dx");
        MDM_REQUIRE(r.route != GN_BWD_REDUCE || d.ws, "groupnorm_bwd: the fp32 path needs ws (>= 3 * N * C floats) for its fixed-order sums");
    }
    kGnRoutes[r.route].launch(d, r, (hipStream_t)stream);
    const int rc = launch_status(what);
    if (rc == 0) g_gn_route = r.route;
    return rc;
}
extern "C" int mdm_groupnorm_fwd(const mdm_gn_desc* desc_host, void* stream) { return gn_run(0, "groupnorm_fwd", desc_host, stream); }
extern "C" int mdm_groupnorm_bwd(const mdm_gn_desc* desc_host, void* stream) { return gn_run(1, "groupnorm_bwd", desc_host, stream); }
extern "C" const char* mdm_gn_route_of(int which, const mdm_gn_desc* desc_host) {
    GnPlan r;
    return desc_host && gn_route(which, *desc_host, &r) == 0 ? kGnRoutes[r.route].name : nullptr;
}
extern "C" const char* mdm_gn_last_route(void) { return g_gn_route >= 0 ? kGnRoutes[g_gn_route].name : "none"; }
extern "C" int mdm_gn_route_names(const char** out, int cap) {
    for (int i = 0; i < GN_ROUTES && i < cap; ++i)
        if (out) out[i] = kGnRoutes[i].name;
    return GN_ROUTES;
}

extern "C" int mdm_dropout_mask(const uint64_t* rng, uint64_t base, const uint32_t* ctl, int64_t n, uint8_t* keep, void* stream) {
    MDM_REQUIRE(rng && ctl && keep && n > 0 && n < (1ll << 36), "dropout_mask: bad arguments");
    const int64_t vecs = (int64_t)(((base + (uint64_t)n + 7) >> 3) - (base >> 3));
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(cdiv(vecs, 256)), dim3(256), 0, (hipStream_t)stream, rng, base, ctl, n, keep);
    return launch_status("dropout_mask");
}

// floats of `ws` the backward entry points write for this problem (0: none needed).  The C ABI carries no buffer sizes, so a caller
// sizes its workspace with this query instead of with a constant from the header's prose.
extern "C" int64_t mdm_groupnorm_bwd_ws_floats(int dtype, int N, int C) {
    return dtype == MDM_F32 ? (int64_t)3 * N * C : 0;
}

#ifdef MDM_STAMP
extern "C" int mdm_debug_stamps_norm(unsigned long long* out, int reset) {      // out: 4096 * 16 entries
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdm::g_nstamp_buf), 4096 * 16 * 8) != hipSuccess) return -1;
    if (reset) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(mdm::g_nstamp_buf)) != hipSuccess || hipMemset(p, 0, 4096 * 16 * 8) != hipSuccess) return -1;
    }
    return 0;
}
#endif

extern "C" int mdm_softmax_fwd(int dtype, void* S, int rows, int L, void* stream) {
    MDM_REQUIRE(rows > 0 && L > 0, "softmax: bad shape");
    DISPATCH_T(dtype, hipLaunchKernelGGL((softmax_fwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, (T*)S, rows, L));
    return launch_status("softmax_fwd");
}
extern "C" int mdm_softmax_bwd(int dtype, const void* P, void* dP, int rows, int L, void* stream) {
    MDM_REQUIRE(rows > 0 && L > 0, "softmax: bad shape");
    DISPATCH_T(dtype, hipLaunchKernelGGL((softmax_bwd_kernel<T>), dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, (const T*)P, (T*)dP, rows, L));
    return launch_status("softmax_bwd");
}

extern "C" int mdm_timestep_embedding(const float* t, int N, int dim, float* y, void* stream) {
    MDM_REQUIRE(N > 0 && dim >= 4, "timestep_embedding: bad shape");
    hipLaunchKernelGGL(temb_kernel, dim3(cdiv(N * (dim / 2), 256)), dim3(256), 0, (hipStream_t)stream, t, N, dim, 0, 1.f, y);
    return launch_status("timestep_embedding");
}
extern "C" int mdm_timestep_embedding2(const float* t, int N, int dim, int flip_sin_to_cos, float freq_shift, float* y, void* stream) {
    MDM_REQUIRE(N > 0 && dim >= 4, "timestep_embedding: bad shape");
    hipLaunchKernelGGL(temb_kernel, dim3(cdiv(N * (dim / 2), 256)), dim3(256), 0, (hipStream_t)stream, t, N, dim, flip_sin_to_cos,
                       freq_shift, y);
    return launch_status("timestep_embedding");
}
extern "C" int mdm_silu_fwd(const float* x, float* y, int64_t n, void* stream) {
    hipLaunchKernelGGL(silu_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return launch_status("silu_fwd");
}
extern "C" int mdm_silu_bwd(const float* x, const float* dy, float* dx, int acc, int64_t n, void* stream) {
    hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, acc, n);
    return launch_status("silu_bwd");
}

extern "C" int mdm_colsum(int dtype, const void* dY, int N, int P, int C, float* per_img, int ld, int acc_img, float* dbias,
                          void* stream) {
    MDM_REQUIRE(C % 8 == 0 && N > 0 && P > 0, "colsum: bad shape");
    const int imgs = dtype == MDM_F32 ? N : 1;          // fp32 path: fixed summation order over the images (see colsum_kernel)
    dim3 grid(cdiv(C, 64), cdiv(N, imgs));
    DISPATCH_T(dtype, hipLaunchKernelGGL((colsum_kernel<T>), grid, dim3(256), 0, pick_stream(stream), (const T*)dY, P, C, per_img, ld, acc_img, dbias, imgs, N));
    return launch_status("colsum");
}

extern "C" int mdm_sumpool2(int dtype, const void* g, void* dst, int acc, int N, int H, int W, int C, void* stream) {
    MDM_REQUIRE(C % 8 == 0, "sumpool2: C must be a multiple of 8");
    const int64_t tv = (int64_t)N * H * W * (C / 8);
    DISPATCH_T(dtype, hipLaunchKernelGGL((sumpool2_kernel<T>), dim3(stream_grid(tv)), dim3(256), 0, (hipStream_t)stream, (const T*)g, (T*)dst, acc, H, W, C, tv));
    return launch_status("sumpool2");
}

extern "C" int mdm_avgpool2(int dtype, const void* src, void* dst, int acc, int N, int H, int W, int C, void* stream) {
    MDM_REQUIRE(C % 8 == 0, "avgpool2: C must be a multiple of 8");
    MDM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src && dst, "avgpool2: bad shape");
    const int64_t tv = (int64_t)N * H * W * (C / 8);
    DISPATCH_T(dtype, hipLaunchKernelGGL((avgpool2_kernel<T>), dim3(stream_grid(tv)), dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, acc, H, W, C, tv));
    return launch_status("avgpool2");
}
extern "C" int mdm_upsample2(int dtype, const void* src, void* dst, int acc, float scale, int N, int H, int W, int C, void* stream) {
    MDM_REQUIRE(C % 8 == 0, "upsample2: C must be a multiple of 8");
    MDM_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src && dst, "upsample2: bad shape");
    const int64_t tv = (int64_t)N * H * W * (C / 8);
    DISPATCH_T(dtype, hipLaunchKernelGGL((upsample2_kernel<T>), dim3(stream_grid(tv)), dim3(256), 0, (hipStream_t)stream, (const T*)src, (T*)dst, acc, scale, H, W, C, tv));
    return launch_status("upsample2");
}

extern "C" int mdm_add(int dtype, void* dst, const void* src, int64_t n, void* stream) {
    MDM_REQUIRE(n % 8 == 0 && dst && src, "add: n must be a multiple of 8");
    DISPATCH_T(dtype, hipLaunchKernelGGL((add_kernel<T>), dim3(stream_grid(n / 8)), dim3(256), 0, (hipStream_t)stream, (T*)dst, (const T*)dst, (const T*)src, n / 8));
    return launch_status("add");
}
extern "C" int mdm_add3(int dtype, void* dst, const void* x, const void* y, int64_t n, void* stream) {
    MDM_REQUIRE(n % 8 == 0 && dst && x, "add3: n must be a multiple of 8");
    DISPATCH_T(dtype, hipLaunchKernelGGL((add_kernel<T>), dim3(stream_grid(n / 8)), dim3(256), 0, (hipStream_t)stream, (T*)dst, (const T*)x, (const T*)y, n / 8));
    return launch_status("add3");
}

extern "C" int mdm_nchw_to_nhwc(int dtype, const float* x, void* y, int N, int C, int H, int W, int Cp, void* stream) {
    MDM_REQUIRE(Cp >= C && Cp % 8 == 0, "nchw_to_nhwc: bad Cp");
    const int64_t total = (int64_t)N * H * W * Cp;
    DISPATCH_T(dtype, hipLaunchKernelGGL((nchw_to_nhwc_kernel<T>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, (T*)y, C, H * W, Cp, total));
    return launch_status("nchw_to_nhwc");
}
extern "C" int mdm_nhwc_to_nchw(int dtype, const void* x, float* y, int N, int C, int H, int W, int Cp, void* stream) {
    MDM_REQUIRE(Cp >= C, "nhwc_to_nchw: bad Cp");
    const int64_t total = (int64_t)N * C * H * W;
    DISPATCH_T(dtype, hipLaunchKernelGGL((nhwc_to_nchw_kernel<T>), dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)x, y, C, H * W, Cp, total));
    return launch_status("nhwc_to_nchw");
}
