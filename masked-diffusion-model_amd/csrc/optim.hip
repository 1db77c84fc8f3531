// Optimizer pass over flat fp32 buffers: global grad-norm, clip, AdamW / Adam / SGD, EMA and the
// bf16 weight shadow in one read-modify-write sweep (HBM-bound; AdamW and Adam: 16 B read + 12..18 B
// written per parameter, SGD: 8..12 B read + 4..8 B written, + 4 B each way for the EMA, + 2 B for the shadow).
//
// Replaces accelerator.clip_grad_norm_ + torch.optim.{AdamW, Adam, SGD}.step + diffusers EMAModel.step
// (reference trainer_masked_mean_shift.py:163-172, main_train_masked.py:116-141).
#include "common.h"

namespace mdm {

// Deterministic two-stage reduction: data-parallel replicas must derive the SAME clip coefficient from the
// same (all-reduced) gradient, bit for bit, or they drift apart -- so no float atomics here.
constexpr int SQN_BLOCKS = 1024;
__device__ float g_sqnorm_partials[SQN_BLOCKS];

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, int64_t n4, int64_t n) {
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<const float4*>(g)[i];
        a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = n4 * 4; i < n; ++i) a = fmaf(g[i], g[i], a);
    a = wave_sum(a);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) g_sqnorm_partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__global__ __launch_bounds__(256) void sqnorm_final_kernel(float* out, int nblk) {
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) a += g_sqnorm_partials[i];
    a = wave_sum(a);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) *out = (part[0] + part[1]) + (part[2] + part[3]);      // stored: no zeroing launch in front
}

// The one update sweep (mdm_optim_update): clip coefficient, gmul, update, EMA, bf16 shadow.  Bytes per parameter, EMA and shadow
// aside (+8 B and +2 B), and elements per lane and iteration (W):
//   KIND 0  SGD, momentum == 0: no state at all                 8 B read +  4 B written   W = 8
//   KIND 1  SGD with a momentum buffer (s0)                     12 B read +  8 B written   W = 8
//   KIND 2  Adam, coupled (L2) weight decay (s0 = m, s1 = v)    16 B read + 12 B written   W = 8
//   KIND 3  AdamW, decoupled weight decay (s0 = m, s1 = v)      16 B read + 12 B written   W = 1
// W = 8 is two 16-byte loads per stream, all issued up front, two 16-byte stores per fp32 stream and one 16-byte store of the shadow.
// W = 1 is scalar loads and stores, the EMA read only behind the update's stores: the four-stream sweep of the default optimizer
// runs 4 % faster that way than at W = 8, and 5 % slower with the EMA's load up front (profiles/r16_optim_one_kernel.md).
// hp (device, 8 floats):
//   SGD       lr, momentum, buf_decay, g_scale, weight_decay, nesterov (0 | 1), -, ema_decay
//             buf = buf_decay buf + g_scale d: the host sends (0, 1) on the optimizer's first step (torch: buf = d) and (momentum,
//             1 - dampening) afterwards -- the rule lives in the block, not in a kernel argument, so a captured graph replays it
//   Adam[W]   lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, ema_decay
enum { OPT_SGD = 0, OPT_SGD_MOMENTUM = 1, OPT_ADAM = 2, OPT_ADAMW = 3 };

struct OptimConsts {
    float coef, lr, wd, ed, a, b, c, d, e;      // a..e: per kind, see optim_consts
};
template <int KIND>
__device__ __forceinline__ OptimConsts optim_consts(const float* hp, const float* sqnorm, float max_norm, float gmul) {
    OptimConsts k;
    k.coef = gmul;
    if (max_norm > 0.f) {
        float norm = sqrtf(*sqnorm) * gmul;
        float c = max_norm / (norm + 1e-6f);          // torch.nn.utils.clip_grad_norm_
        if (c < 1.f) k.coef *= c;
    }
    k.lr = hp[0]; k.wd = hp[4]; k.ed = hp[7];
    if (KIND >= OPT_ADAM) {
        k.a = hp[1]; k.b = hp[2]; k.c = hp[3];        // beta1, beta2, eps
        k.d = hp[0] / hp[5]; k.e = rsqrtf(hp[6]);     // lr / bias_corr1, 1 / sqrt(bias_corr2)
    } else {
        k.a = hp[1]; k.b = hp[2]; k.c = hp[3]; k.d = hp[5]; k.e = 0.f;   // momentum, buf_decay, g_scale, nesterov
    }
    return k;
}
// one element: p, s0, s1 updated in place (torch's single-tensor SGD / Adam / AdamW, in their order of operations).  Which product
// of a sum of two the compiler fuses is its choice, and it moves with the code around the expression: kinds 0..2 are left to it and
// held to their bits by scripts/optim_parity.py; AdamW's two sums, which it fused the other way round when the EMA's load moved,
// are spelled out as they have always been rounded.
template <int KIND>
__device__ __forceinline__ void optim_elem(const OptimConsts& k, float& p, float g, float& s0, float& s1) {
    float d = g * k.coef;
    if (KIND == OPT_ADAMW) p *= 1.f - k.lr * k.wd;    // decoupled decay: the weight shrinks first, the moments never see it
    else d += k.wd * p;                               // coupled (L2) decay: part of the gradient
    if (KIND == OPT_SGD_MOMENTUM) {
        s0 = k.b * s0 + k.c * d;
        d = k.d != 0.f ? d + k.a * s0 : s0;           // nesterov reads the NEW buffer
    }
    if (KIND >= OPT_ADAM) {
        if (KIND == OPT_ADAM) {
            s0 = k.a * s0 + (1.f - k.a) * d;
            s1 = k.b * s1 + (1.f - k.b) * d * d;
        } else {
            s0 = __fmaf_rn(1.f - k.a, d, k.a * s0);
            s1 = __fmaf_rn(d, (1.f - k.b) * d, k.b * s1);
        }
        float denom = sqrtf(s1) * k.e + k.c;
        p -= k.d * s0 / denom;
    } else {
        p -= k.lr * d;
    }
}
// W consecutive elements of one stream, in registers and to or from memory
__device__ __forceinline__ void loadw(float8& r, const float* p) { r = load8(p); }
__device__ __forceinline__ void loadw(float& r, const float* p) { r = *p; }
__device__ __forceinline__ void storew(float* p, const float8& v) { store8(p, v); }
__device__ __forceinline__ void storew(float* p, float v) { *p = v; }
__device__ __forceinline__ void storew(bf16_t* p, const float8& v) { store8(p, v); }
__device__ __forceinline__ void storew(bf16_t* p, float v) { *p = f2bf(v); }

template <int KIND, typename V>
__device__ __forceinline__ void store_state(float* p, float* s0, float* s1, int64_t o, const V& pv, const V& a, const V& b) {
    storew(p + o, pv);
    if (KIND >= OPT_SGD_MOMENTUM) storew(s0 + o, a);
    if (KIND >= OPT_ADAM) storew(s1 + o, b);
}

template <int KIND, int W>
__global__ __launch_bounds__(256) void optim_update_kernel(float* p, const float* g, float* s0, float* s1, float* ema, bf16_t* shadow,
                                                           int64_t n, const float* hp, const float* sqnorm, float max_norm, float gmul) {
    static_assert(W == 1 || W == 8, "one scalar or two 16-byte words per stream");
    using V = std::conditional_t<W == 8, float8, float>;
    const OptimConsts k = optim_consts<KIND>(hp, sqnorm, max_norm, gmul);
    const float ew = 1.f - k.ed;
    const int64_t nw = n / W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (int64_t)gridDim.x * 256) {
        const int64_t o = i * W;
        V pv, gv, a = {}, b = {}, ev = {};
        loadw(pv, p + o);
        loadw(gv, g + o);
        if (KIND >= OPT_SGD_MOMENTUM) loadw(a, s0 + o);
        if (KIND >= OPT_ADAM) loadw(b, s1 + o);
        if (W > 1 && ema) loadw(ev, ema + o);
        float *pf = reinterpret_cast<float*>(&pv), *af = reinterpret_cast<float*>(&a), *bf = reinterpret_cast<float*>(&b);
        float* ef = reinterpret_cast<float*>(&ev);
        const float* gf = reinterpret_cast<const float*>(&gv);
#pragma unroll
        for (int j = 0; j < W; ++j) optim_elem<KIND>(k, pf[j], gf[j], af[j], bf[j]);
        if (W == 1) {                              // one element per lane: the EMA is read behind the update's stores
            store_state<KIND>(p, s0, s1, o, pv, a, b);
            if (ema) loadw(ev, ema + o);
        }
        if (ema) {
#pragma unroll
            for (int j = 0; j < W; ++j) ef[j] = ef[j] - ew * (ef[j] - pf[j]);
        }
        if (W > 1) store_state<KIND>(p, s0, s1, o, pv, a, b);
        if (ema) storew(ema + o, ev);
        if (shadow) storew(shadow + o, pv);
    }
    // the n % W elements behind the last whole group (the parameter store's sizes are multiples of 8: plain tensors only)
    const int64_t t = nw * W + threadIdx.x;
    if (W > 1 && blockIdx.x == 0 && t < n) {
        float pi = p[t], a = 0.f, b = 0.f;
        if (KIND >= OPT_SGD_MOMENTUM) a = s0[t];
        if (KIND >= OPT_ADAM) b = s1[t];
        optim_elem<KIND>(k, pi, g[t], a, b);
        p[t] = pi;
        if (KIND >= OPT_SGD_MOMENTUM) s0[t] = a;
        if (KIND >= OPT_ADAM) s1[t] = b;
        if (ema) { float e = ema[t]; ema[t] = e - ew * (e - pi); }
        if (shadow) shadow[t] = f2bf(pi);
    }
}

// Transposed bf16 shadow of the conv filters: bf16 [tap][Cout][Cin] (written by the optimizer kernel) -> bf16 [tap][Cin][Cout],
// so the data-gradient contraction reads its weights k-contiguous like the forward does.  One workgroup per 64 x 64 tile of
// one tap of one layer, 16-byte loads and stores on both sides (Cout, Cin are multiples of 8);
// `tiles` = {element offset of the tap matrix, Cout, Cin, row0, col0} x ntiles.
// (The first version moved 2 bytes per lane on 32 x 32 tiles: 62 us for 143 MB; this one is bound by the bytes.)
__global__ __launch_bounds__(256) void transpose_shadow_bf16_kernel(const bf16_t* Pb, bf16_t* PT, const int64_t* tiles, int ntiles) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];
    const int64_t* e = tiles + (int64_t)blockIdx.x * 5;
    const int64_t off = e[0];
    const int Cout = (int)e[1], Cin = (int)e[2], r0 = (int)e[3], c0 = (int)e[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = threadIdx.x + 256 * i, row = q >> 3, cc = (q & 7) * 8;
        const int r = r0 + row, c = c0 + cc;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < Cout && c < Cin) v = *reinterpret_cast<const uint4*>(Pb + off + (int64_t)r * Cin + c);
        *reinterpret_cast<uint4*>(&tile[row][cc]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = threadIdx.x + 256 * i, col = q >> 3, rr = (q & 7) * 8;
        const int c = c0 + col, r = r0 + rr;
        if (c < Cin && r < Cout) {                                   // Cout % 8 == 0: the 8 rows are inside or outside together
            uint4 v;
            v.x = (uint32_t)tile[rr + 0][col] | ((uint32_t)tile[rr + 1][col] << 16);
            v.y = (uint32_t)tile[rr + 2][col] | ((uint32_t)tile[rr + 3][col] << 16);
            v.z = (uint32_t)tile[rr + 4][col] | ((uint32_t)tile[rr + 5][col] << 16);
            v.w = (uint32_t)tile[rr + 6][col] | ((uint32_t)tile[rr + 7][col] << 16);
            *reinterpret_cast<uint4*>(PT + off + (int64_t)c * Cout + r) = v;
        }
    }
}

// One 32-bit word of each half of the split shadow: element xa of a block's first 16 in the low 16 bits, its partner xb of the second
// 16 in the high ones -- `hi` = their bf16 roundings, `lo` = the bf16 roundings of what that left.
__device__ __forceinline__ void split_pair(float xa, float xb, uint32_t& hi, uint32_t& lo) {
    const bf16_t h0 = f2bf(xa), h1 = f2bf(xb);
    hi = (uint32_t)h0 | ((uint32_t)h1 << 16);
    lo = (uint32_t)f2bf(xa - bf2f(h0)) | ((uint32_t)f2bf(xb - bf2f(h1)) << 16);
}

// The split shadow of fp32 filters (mdm_gemm_desc.B_split; conv_halo_body<..., SPLIT>): per 32-element block, chunk g = 8 bf16 hi
// halves of elements {4g..4g+3, 16+4g..16+4g+3} -- dword k = (element 4g+k, element 16+4g+k) --, chunk 4+g = their lo halves in the same
// order.  One thread per (block, g): two 16-byte loads, two stores.
// segs[i] = {element offset, length}; blockIdx.y = segment.
__global__ __launch_bounds__(256) void split_shadow_kernel(const float* P, float* Ps, const int64_t* segs) {
    const int64_t off = segs[2 * blockIdx.y], len = segs[2 * blockIdx.y + 1];
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < len / 8; id += (int64_t)gridDim.x * 256) {
        const int64_t base = off + (id >> 2) * 32 + (id & 3) * 4;
        const float4 a = *reinterpret_cast<const float4*>(P + base), b = *reinterpret_cast<const float4*>(P + base + 16);
        const float xa[4] = {a.x, a.y, a.z, a.w}, xb[4] = {b.x, b.y, b.z, b.w};
        uint32_t h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split_pair(xa[k], xb[k], h[k], l[k]);
        *reinterpret_cast<uint4*>(Ps + base) = make_uint4(h[0], h[1], h[2], h[3]);
        *reinterpret_cast<uint4*>(Ps + base + 16) = make_uint4(l[0], l[1], l[2], l[3]);
    }
}

// The same shadow of the per-tap TRANSPOSED, tap-FLIPPED filters: PsT[off + tap' Cin Cout + ci Cout + co] holds
// P[off + (taps - 1 - tap') Cout Cin + co Cin + ci] in split_shadow_kernel's arrangement over the 32-element blocks of a row of Cout.
// One thread per (tap', ci, block, g): lanes walk ci, so each of its eight 4-byte loads is one coalesced row segment of the
// [Cout][Cin] source (a 16-byte load would need four ci per lane and a transpose in registers; this runs once per optimizer step).
// segs[i] = {element offset, taps, Cout, Cin}; blockIdx.y = filter.
__global__ __launch_bounds__(256) void split_shadow_t_kernel(const float* P, float* PsT, const int64_t* segs) {
    const int64_t off = segs[4 * blockIdx.y], taps = segs[4 * blockIdx.y + 1], co_n = segs[4 * blockIdx.y + 2], ci_n = segs[4 * blockIdx.y + 3];
    const int64_t per_tap = (co_n / 8) * ci_n;                  // (block, g) pairs x ci
    for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < taps * per_tap; id += (int64_t)gridDim.x * 256) {
        const int64_t tp = id / per_tap, rem = id - tp * per_tap, bg = rem / ci_n, ci = rem - bg * ci_n;
        const int64_t co = (bg >> 2) * 32 + (bg & 3) * 4;
        const float* src = P + off + (taps - 1 - tp) * co_n * ci_n + co * ci_n + ci;
        uint32_t h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split_pair(src[k * ci_n], src[(16 + k) * ci_n], h[k], l[k]);
        float* dst = PsT + off + tp * co_n * ci_n + ci * co_n + co;
        *reinterpret_cast<uint4*>(dst) = make_uint4(h[0], h[1], h[2], h[3]);
        *reinterpret_cast<uint4*>(dst + 16) = make_uint4(l[0], l[1], l[2], l[3]);
    }
}

__global__ void cast_bf16_kernel(const float* src, bf16_t* dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = f2bf(src[i]);
}
__global__ void fill_kernel(float* p, float v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
// segs[i] = {element offset, length}; lengths are multiples of 4 and <= 4096, offsets 16-byte aligned: one workgroup each
__global__ __launch_bounds__(256) void fill_segments_kernel(float* base, const int64_t* segs, float v) {
    const int64_t off = segs[2 * blockIdx.x], len = segs[2 * blockIdx.x + 1];
    const float4 v4 = make_float4(v, v, v, v);
    for (int64_t i = 4 * (int64_t)threadIdx.x; i < len; i += 1024) *reinterpret_cast<float4*>(base + off + i) = v4;
}
static inline int ogrid(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
}  // namespace mdm
using namespace mdm;

extern "C" int mdm_sqnorm(const float* g, int64_t n, float* out, void* stream) {
    MDM_REQUIRE(g && out && n > 0, "sqnorm: bad arguments");
    MDM_REQUIRE(((uintptr_t)g & 15) == 0, "sqnorm: buffer must be 16-byte aligned");
    int nb = ogrid(n / 4);
    if (nb > SQN_BLOCKS) nb = SQN_BLOCKS;
    hipLaunchKernelGGL(sqnorm_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, n / 4, n);
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, out, nb);
    return launch_status("sqnorm");
}
extern "C" int mdm_optim_update(int kind, float* p, const float* g, float* buf0, float* buf1, float* ema, void* shadow_bf16, int64_t n,
                                const float* hp, const float* sqnorm, float max_norm, float gmul, void* stream) {
    MDM_REQUIRE(kind >= OPT_SGD && kind <= OPT_ADAMW, "optim_update: kind must be 0 (SGD), 1 (SGD + momentum), 2 (Adam) or 3 (AdamW)");
    MDM_REQUIRE(p && g && hp && n > 0, "optim_update: bad arguments");
    MDM_REQUIRE(kind == OPT_SGD || buf0, "optim_update: this kind needs its first state buffer");
    MDM_REQUIRE(kind < OPT_ADAM || buf1, "optim_update: Adam and AdamW need both state buffers");
    MDM_REQUIRE(max_norm <= 0.f || sqnorm, "optim_update: clipping needs the squared norm");
    MDM_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf0 | (uintptr_t)buf1 | (uintptr_t)ema | (uintptr_t)shadow_bf16) & 15) == 0,
                "optim_update: buffers must be 16-byte aligned");
    const dim3 block(256);
    hipStream_t st = (hipStream_t)stream;
    bf16_t* sh = (bf16_t*)shadow_bf16;
    // the one place a kind gets its width: the grid covers n / W groups, one per lane, up to ogrid's cap
    if (kind == OPT_SGD)
        hipLaunchKernelGGL((optim_update_kernel<OPT_SGD, 8>), dim3(ogrid(n / 8)), block, 0, st, p, g, nullptr, nullptr, ema, sh, n, hp, sqnorm, max_norm, gmul);
    else if (kind == OPT_SGD_MOMENTUM)
        hipLaunchKernelGGL((optim_update_kernel<OPT_SGD_MOMENTUM, 8>), dim3(ogrid(n / 8)), block, 0, st, p, g, buf0, nullptr, ema, sh, n, hp, sqnorm, max_norm, gmul);
    else if (kind == OPT_ADAM)
        hipLaunchKernelGGL((optim_update_kernel<OPT_ADAM, 8>), dim3(ogrid(n / 8)), block, 0, st, p, g, buf0, buf1, ema, sh, n, hp, sqnorm, max_norm, gmul);
    else
        hipLaunchKernelGGL((optim_update_kernel<OPT_ADAMW, 1>), dim3(ogrid(n)), block, 0, st, p, g, buf0, buf1, ema, sh, n, hp, sqnorm, max_norm, gmul);
    return launch_status("optim_update");
}
extern "C" int mdm_transpose_shadow_bf16(const void* Pb, void* PT, const int64_t* tiles, int ntiles, void* stream) {
    MDM_REQUIRE(Pb && PT && tiles && ntiles > 0, "transpose_shadow_bf16: bad arguments");
    hipLaunchKernelGGL(transpose_shadow_bf16_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Pb, (bf16_t*)PT, tiles, ntiles);
    return launch_status("transpose_shadow_bf16");
}
extern "C" int mdm_split_shadow(const float* P, float* Ps, const int64_t* segs, int nseg, void* stream) {
    MDM_REQUIRE(P && Ps && segs && nseg > 0 && nseg <= 65535, "split_shadow: bad arguments");
    MDM_REQUIRE((((uintptr_t)P | (uintptr_t)Ps) & 15) == 0, "split_shadow: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(split_shadow_kernel, dim3(64, (unsigned)nseg), dim3(256), 0, (hipStream_t)stream, P, Ps, segs);
    return launch_status("split_shadow");
}
extern "C" int mdm_split_shadow_t(const float* P, float* PsT, const int64_t* segs, int nseg, void* stream) {
    MDM_REQUIRE(P && PsT && segs && nseg > 0 && nseg <= 65535, "split_shadow_t: bad arguments");
    MDM_REQUIRE((((uintptr_t)P | (uintptr_t)PsT) & 15) == 0, "split_shadow_t: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(split_shadow_t_kernel, dim3(64, (unsigned)nseg), dim3(256), 0, (hipStream_t)stream, P, PsT, segs);
    return launch_status("split_shadow_t");
}
extern "C" int mdm_cast_bf16(const float* src, void* dst, int64_t n, void* stream) {
    MDM_REQUIRE(src && dst && n >= 0, "cast_bf16: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3(ogrid(n)), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
    return launch_status("cast_bf16");
}
extern "C" int mdm_fill_segments_f32(float* base, const int64_t* segs, int nseg, float v, void* stream) {
    MDM_REQUIRE(base && segs && nseg > 0, "fill_segments: bad arguments");
    hipLaunchKernelGGL(fill_segments_kernel, dim3((unsigned)nseg), dim3(256), 0, (hipStream_t)stream, base, segs, v);
    return launch_status("fill_segments");
}
extern "C" int mdm_fill_f32(float* p, float v, int64_t n, void* stream) {
    MDM_REQUIRE(p && n >= 0, "fill: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(fill_kernel, dim3(ogrid(n)), dim3(256), 0, (hipStream_t)stream, p, v, n);
    return launch_status("fill");
}
