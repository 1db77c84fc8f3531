// The four standalone GroupNorm kernels.  norm.hip compiles this text TWICE: GN_DROP 0 gives the kernels as they always were (the
// same tokens, so the same device code: scripts/cmp_device_code.py), GN_DROP 1 their dropout variants gn_*_kernel_drop with three
// more arguments (rng, dbase, ctl: see drop_keep_bits in norm.hip).  A shared __device__ body inlined into two __global__ wrappers
// was tried first: it changed the register allocation of all 19 existing instantiations.
//   GN_K(name)        kernel name            GN_DROP_PARAMS    the extra kernel parameters
//   GN_LOAD_DY(pix)   float8 of dy (dz)      GN_DZ(v)          a value unpacked from the masked packed dy, scaled
template <typename T>
__global__ __launch_bounds__(256) void GN_K(gn_fwd_kernel)(const T* s0, int C0, const T* s1, int C1, int P, int G, int CBLK,
                                                     float eps, const float* gamma, const float* beta, int silu, T* y,
                                                     float* stats GN_DROP_PARAMS) {
#if GN_DROP
    const uint32_t dthr = ctl[0];                                    // 0: eval mode, no Philox work (uniform)
    const float dscale = __uint_as_float(ctl[1]);
#endif
    const int C = C0 + C1, cpg = div_small(C, rcp_small(G));
    const float inv_cpg = rcp_small(cpg);
    const int VB = CBLK >> 3, PL = div_small(256, rcp_small(VB));
    const int img = blockIdx.x, cb = blockIdx.y * CBLK;     // image fastest: the channel blocks of one image (they share 128-B lines) land on one XCD
    const int t = threadIdx.x, lane = div_small(t, rcp_small(VB)), v = t - lane * VB, c = cb + v * 8;
    const int ng = div_small(CBLK, inv_cpg), g0 = div_small(cb, inv_cpg);
    const bool on = t < VB * PL && c < C;
    __shared__ float gsum[2 * 64], gmean[64], grstd[64];
    __shared__ float scratch[16 * (256 + 4)];
    __shared__ float csum[16 * 8];
    const int64_t base = (int64_t)img * P;
    float part[16];                       // [0, 8): sums of (x - K), [8, 16): sums of (x - K)^2, per channel of this lane's vector
#pragma unroll
    for (int k = 0; k < 16; ++k) part[k] = 0.f;
    if (on) {
        float K[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) K[e] = gn_pivot(s0, s1, C0, C1, base, div_small(c + e, inv_cpg), cpg);
        auto add = [&](const float8& x) {
            float xv[8] = F8_TO_ARR(x);
#pragma unroll
            for (int e = 0; e < 8; ++e) { float dlt = xv[e] - K[e]; part[e] += dlt; part[8 + e] = fmaf(dlt, dlt, part[8 + e]); }
        };
        int p = lane;
        for (; p + 3 * PL < P; p += 4 * PL) {          // four independent 16-byte loads in flight per lane
            float8 x0 = load8(src_ptr(s0, s1, C0, C1, base + p, c));
            float8 x1 = load8(src_ptr(s0, s1, C0, C1, base + p + PL, c));
            float8 x2 = load8(src_ptr(s0, s1, C0, C1, base + p + 2 * PL, c));
            float8 x3 = load8(src_ptr(s0, s1, C0, C1, base + p + 3 * PL, c));
            add(x0); add(x1); add(x2); add(x3);
        }
        for (; p < P; p += PL) add(load8(src_ptr(s0, s1, C0, C1, base + p, c)));
    }
    // FIXED summation order (no float atomics: the same input gives the same bits on every box): pixel lanes per channel
    // through block_colsum, then one thread per group walks its channels in order
    block_colsum<16, 256>(part, scratch, csum, t, VB, PL);          // csum[(q*8+e)*VB + v]
    if (t < ng) group_sums<2>(csum, VB, t * cpg, cpg, 8, &gsum[2 * t]);
    __syncthreads();
    if (t < ng && (g0 + t) < G) {
        const float inv_cnt = 1.f / ((float)cpg * (float)P);
        float K = gn_pivot(s0, s1, C0, C1, base, g0 + t, cpg);
        float md = gsum[2 * t] * inv_cnt;
        float var = fmaxf(gsum[2 * t + 1] * inv_cnt - md * md, 0.f);
        float mean = K + md, rstd = rsqrtf(var + eps);
        gmean[t] = mean; grstd[t] = rstd;
        stats[((int64_t)img * G + g0 + t) * 2] = mean;
        stats[((int64_t)img * G + g0 + t) * 2 + 1] = rstd;
    }
    __syncthreads();
    if (on) {
        float m[8], a[8], bt[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int gl = div_small(c + e, inv_cpg) - g0;
            m[e] = gmean[gl]; a[e] = grstd[gl] * gamma[c + e]; bt[e] = beta[c + e];
        }
        auto put = [&](int p, const float8& x) {
            float xv[8] = F8_TO_ARR(x);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = fmaf(xv[e] - m[e], a[e], bt[e]);     // (x - mean) stays exact
                if (silu) o[e] = silu_f(o[e]);
            }
#if GN_DROP
            if (dthr) drop_apply(o, drop_keep_bits(rng, dbase + (uint64_t)((base + p) * C + c), dthr), dscale);
#endif
            float8 r = {make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7])};
            store8(y + (base + p) * C + c, r);
        };
        int p = lane;
        for (; p + 3 * PL < P; p += 4 * PL) {
            float8 x0 = load8(src_ptr(s0, s1, C0, C1, base + p, c));
            float8 x1 = load8(src_ptr(s0, s1, C0, C1, base + p + PL, c));
            float8 x2 = load8(src_ptr(s0, s1, C0, C1, base + p + 2 * PL, c));
            float8 x3 = load8(src_ptr(s0, s1, C0, C1, base + p + 3 * PL, c));
            put(p, x0); put(p + PL, x1); put(p + 2 * PL, x2); put(p + 3 * PL, x3);
        }
        for (; p < P; p += PL) put(p, load8(src_ptr(s0, s1, C0, C1, base + p, c)));
    }
}

// backward: dx = rstd*gamma*g - rstd*(s1 + xhat*s2)/cnt with g = dy * act'(xhat*gamma + beta),
// s1 = sum(g*gamma), s2 = sum(g*gamma*xhat) per (image, group); dgamma += sum g*xhat, dbeta += sum g.
// Every reduction has a FIXED order.  Inside the workgroup: block_colsum + one thread per group.  Across the images:
// `part` != nullptr (the fp32 path) -> this workgroup's per-channel sums go to part[img][{dgamma, dbeta}][C] (plain stores)
// and gn_param_reduce_kernel adds them up image by image behind this launch (it also forms sum_all from sum_img);
// part == nullptr (bf16 large maps) -> one float atomic per channel per image, as the register-cached kernels do.
template <typename T>
__global__ __launch_bounds__(256) void GN_K(gn_bwd_kernel)(const T* s0, int C0, const T* s1, int C1, int P, int G, int CBLK,
                                                     const float* gamma, const float* beta, int silu, const T* dy,
                                                     const float* stats, T* d0, const T* add0, T* d1, const T* add1, const T* add0b,
                                                     float* dgamma, float* dbeta, float* sum_img, int sum_ld, float* sum_all,
                                                     float* part GN_DROP_PARAMS) {
#if GN_DROP
    const uint32_t dthr = ctl[0];                                    // 0: eval mode, no Philox work (uniform)
    const float dscale = __uint_as_float(ctl[1]);
#endif
    const int C = C0 + C1, cpg = div_small(C, rcp_small(G));
    const float inv_cpg = rcp_small(cpg);
    const int VB = CBLK >> 3, PL = div_small(256, rcp_small(VB));
    const int img = blockIdx.x, cb = blockIdx.y * CBLK;     // image fastest: the channel blocks of one image (they share 128-B lines) land on one XCD
    const int t = threadIdx.x, lane = div_small(t, rcp_small(VB)), v = t - lane * VB, c = cb + v * 8;
    const int ng = div_small(CBLK, inv_cpg), g0 = div_small(cb, inv_cpg);
    const bool on = t < VB * PL && c < C;
    __shared__ float gsum[2 * 64];
    __shared__ float scratch[32 * (256 + 4)];
    __shared__ float csum[32 * 8];
    const int64_t base = (int64_t)img * P;
#if GN_DROP
    // dz = dy * keep * scale right behind the load of dy (the forward's mask, drawn again): everything below sees dz
    auto load_dy = [&](int64_t pix) {
        float8 d = load8(dy + pix * C + c);
        if (dthr) drop_apply(d, drop_keep_bits(rng, dbase + (uint64_t)(pix * C + c), dthr), dscale);
        return d;
    };
#endif
    float ga[8], be[8], mean[8], rstd[8];
    float acc[32];                        // per channel of this lane's vector: a1, a2, dgamma, dbeta
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.f;
    if (on) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int grp = div_small(c + e, inv_cpg);
            ga[e] = gamma[c + e]; be[e] = beta[c + e];
            mean[e] = stats[((int64_t)img * G + grp) * 2]; rstd[e] = stats[((int64_t)img * G + grp) * 2 + 1];
        }
        auto add = [&](const float8& x, const float8& d) {
            float xv[8] = F8_TO_ARR(x);
            float dv[8] = F8_TO_ARR(d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float xh = (xv[e] - mean[e]) * rstd[e];
                float gz = dv[e];
                if (silu) gz *= silu_grad_f(fmaf(xh, ga[e], be[e]));
                acc[16 + e] = fmaf(gz, xh, acc[16 + e]); acc[24 + e] += gz;
                float gg = gz * ga[e];
                acc[e] += gg; acc[8 + e] = fmaf(gg, xh, acc[8 + e]);
            }
        };
        int p = lane;
        for (; p + PL < P; p += 2 * PL) {
            float8 x0 = load8(src_ptr(s0, s1, C0, C1, base + p, c));
            float8 e0 = GN_LOAD_DY(base + p);
            float8 x1 = load8(src_ptr(s0, s1, C0, C1, base + p + PL, c));
            float8 e1 = GN_LOAD_DY(base + p + PL);
            add(x0, e0); add(x1, e1);
        }
        for (; p < P; p += PL) add(load8(src_ptr(s0, s1, C0, C1, base + p, c)), GN_LOAD_DY(base + p));
    }
    block_colsum<32, 256>(acc, scratch, csum, t, VB, PL);          // csum[(q*8+e)*VB + v], q = {a1, a2, dgamma, dbeta}
    if (t < ng) group_sums<2>(csum, VB, t * cpg, cpg, 8, &gsum[2 * t]);
    if (t < CBLK && cb + t < C) {            // this workgroup is the only one that holds (image, channel)
        const float dgv = csum[(16 + (t & 7)) * VB + (t >> 3)], dbv = csum[(24 + (t & 7)) * VB + (t >> 3)];
        if (part) {
            part[((int64_t)img * 3) * C + cb + t] = dgv;
            part[((int64_t)img * 3 + 1) * C + cb + t] = dbv;
        } else {
            atomicAdd(&dgamma[cb + t], dgv);
            atomicAdd(&dbeta[cb + t], dbv);
        }
    }
    __syncthreads();
    float k1[8], k2[8], ag[8];
    if (on) {
        const float inv_cnt = 1.f / ((float)cpg * (float)P);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int gl = div_small(c + e, inv_cpg) - g0;
            k1[e] = rstd[e] * gsum[2 * gl] * inv_cnt;
            k2[e] = rstd[e] * gsum[2 * gl + 1] * inv_cnt;
            ag[e] = rstd[e] * ga[e];
        }
    }
    float sx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // column sums of dx (bias / time-embedding gradient of the producer conv)
    if (on) {
        T* dst; const T* addp; int cc, CS;           // addp: a tensor laid out like dst whose values are added (dst itself = accumulate)
        if (c < C0) { dst = d0; addp = add0; cc = c; CS = C0; } else { dst = d1; addp = add1; cc = c - C0; CS = C1; }
        const T* addq = c < C0 ? add0b : nullptr;    // a second addend for source 0 (accumulate AND a residual-branch gradient)
        auto put = [&](int p, const float8& x, const float8& d) {
            float xv[8] = F8_TO_ARR(x);
            float dv[8] = F8_TO_ARR(d);
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float xh = (xv[e] - mean[e]) * rstd[e];
                float gz = dv[e];
                if (silu) gz *= silu_grad_f(fmaf(xh, ga[e], be[e]));
                o[e] = ag[e] * gz - fmaf(xh, k2[e], k1[e]);
                sx[e] += o[e];
            }
            T* q = dst + (base + p) * CS + cc;
            if (addp) {
                float8 old = load8(addp + (base + p) * CS + cc);
                float ov[8] = F8_TO_ARR(old);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += ov[e];
            }
            if (addq) {
                float8 old2 = load8(addq + (base + p) * CS + cc);
                float ov2[8] = F8_TO_ARR(old2);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += ov2[e];
            }
            float8 r = {make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7])};
            store8(q, r);
        };
        int p = lane;
        for (; p + PL < P; p += 2 * PL) {
            float8 x0 = load8(src_ptr(s0, s1, C0, C1, base + p, c));
            float8 e0 = GN_LOAD_DY(base + p);
            float8 x1 = load8(src_ptr(s0, s1, C0, C1, base + p + PL, c));
            float8 e1 = GN_LOAD_DY(base + p + PL);
            put(p, x0, e0); put(p + PL, x1, e1);
        }
        for (; p < P; p += PL) put(p, load8(src_ptr(s0, s1, C0, C1, base + p, c)), GN_LOAD_DY(base + p));
    }
    if (sum_img || sum_all) {               // uniform
        block_colsum<8, 256>(sx, scratch, csum, t, VB, PL);
        if (t < CBLK && cb + t < C) {
            const float r = csum[(t & 7) * VB + (t >> 3)];
            if (sum_img) sum_img[(int64_t)img * sum_ld + cb + t] = r;              // one workgroup owns (image, channel)
            if (part) part[((int64_t)img * 3 + 2) * C + cb + t] = r;              // fixed-order mode: the reduce kernel adds the images up
            else if (sum_all) atomicAdd(&sum_all[cb + t], r);
        }
    }
}

template <int NP, int MODE, int NT = 256, typename T = bf16_t>
__global__ __launch_bounds__(NT) void GN_K(gn_fwd_reg_kernel)(const T* s0, int C0, const T* s1, int C1, int P, int G, int CBLK,
                                                         float eps, const float* gamma, const float* beta, int silu, T* y,
                                                         float* stats, float* ws GN_DROP_PARAMS) {
#if GN_DROP
    const uint32_t dthr = ctl[0];                                    // 0: eval mode, no Philox work (uniform)
    const float dscale = __uint_as_float(ctl[1]);
#endif
    constexpr int CS_PITCH = NT + 4;
    const int C = C0 + C1, cpg = div_small(C, rcp_small(G));
    const float inv_cpg = rcp_small(cpg);
    const int VB = CBLK >> 3, PL = div_small(NT, rcp_small(VB));
    const int img = blockIdx.x, cb = blockIdx.y * CBLK;     // image fastest: the channel blocks of one image (they share 128-B lines) land on one XCD
    const int t = threadIdx.x, lane = div_small(t, rcp_small(VB)), v = t - lane * VB, c = cb + v * 8;
    const int ng = div_small(CBLK, inv_cpg), g0 = div_small(cb, inv_cpg);
    const bool on = t < VB * PL && c < C;
    const int chunks = gridDim.z, chunk = blockIdx.z;
    const int plen = chunks == 1 ? P : (P + chunks - 1) / chunks, pbeg = chunk * plen, pend = min(P, pbeg + plen);
    __shared__ float scratch[16 * CS_PITCH];
    __shared__ float csum[16 * 8];
    __shared__ float gsum[2 * 64], gmean[64], grstd[64], gpiv[64];
    const int64_t base = (int64_t)img * P;
    if (t < 2 * ng) {
        float a = 0.f;
        if (MODE == 2)
            for (int ch = 0; ch < chunks; ++ch) a += ws[(((int64_t)img * chunks + ch) * G + g0 + (t >> 1)) * 2 + (t & 1)];
        gsum[t] = a;
    }
    // one pivot load per group (in flight together with the slice loads below), shared through LDS: every thread
    // loading its 8 pivots itself and the statistics thread loading its pivot AGAIN after the reduction put a second
    // memory round trip on the critical path of a ~3 us kernel
    if (t < ng && g0 + t < G) gpiv[t] = gn_pivot(s0, s1, C0, C1, base, g0 + t, cpg);
    typename RegVec<T>::type cx[NP];
    float part[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) part[k] = 0.f;
    if (on) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int p = pbeg + lane + i * PL;
            cx[i] = p < pend ? RegVec<T>::ld(src_ptr(s0, s1, C0, C1, base + p, c)) : RegVec<T>::zero();
        }
    }
    __syncthreads();
    if (MODE != 2 && on) {
        float K[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) K[e] = gpiv[div_small(c + e, inv_cpg) - g0];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (pbeg + lane + i * PL < pend) {
                float8 x = RegVec<T>::unpack(cx[i]);
                float xv[8] = F8_TO_ARR(x);
#pragma unroll
                for (int e = 0; e < 8; ++e) { float dlt = xv[e] - K[e]; part[e] += dlt; part[8 + e] = fmaf(dlt, dlt, part[8 + e]); }
            }
        }
    }
    if (MODE != 2) {
        block_colsum<16, NT, sizeof(T) == 2>(part, scratch, csum, t, VB, PL);      // csum[(q*8+e)*VB + v]
        // one thread per group walks its channels in order (it was an LDS float atomic per channel: arrival order)
        if (t < ng) {
            float gv[2];
            group_sums<2>(csum, VB, t * cpg, cpg, 8, gv);
            gsum[2 * t] += gv[0]; gsum[2 * t + 1] += gv[1];
        }
    }
    __syncthreads();
    if (MODE == 1) {
        if (t < 2 * ng && g0 + (t >> 1) < G) ws[(((int64_t)img * chunks + chunk) * G + g0 + (t >> 1)) * 2 + (t & 1)] = gsum[t];
        return;
    }
    if (t < ng && (g0 + t) < G) {
        const float inv_cnt = 1.f / ((float)cpg * (float)P);
        float K = gpiv[t];
        float md = gsum[2 * t] * inv_cnt;
        float var = fmaxf(gsum[2 * t + 1] * inv_cnt - md * md, 0.f);
        float mean = K + md, rstd = rsqrtf(var + eps);
        gmean[t] = mean; grstd[t] = rstd;
        if (chunk == 0) {
            stats[((int64_t)img * G + g0 + t) * 2] = mean;
            stats[((int64_t)img * G + g0 + t) * 2 + 1] = rstd;
        }
    }
    __syncthreads();
    if (on) {
        float m[8], a[8], bt[8];
        const float4 g_lo = *reinterpret_cast<const float4*>(gamma + c), g_hi = *reinterpret_cast<const float4*>(gamma + c + 4);
        const float4 b_lo = *reinterpret_cast<const float4*>(beta + c), b_hi = *reinterpret_cast<const float4*>(beta + c + 4);
        const float gv[8] = {g_lo.x, g_lo.y, g_lo.z, g_lo.w, g_hi.x, g_hi.y, g_hi.z, g_hi.w};
        const float bv[8] = {b_lo.x, b_lo.y, b_lo.z, b_lo.w, b_hi.x, b_hi.y, b_hi.z, b_hi.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int gl = div_small(c + e, inv_cpg) - g0;
            m[e] = gmean[gl]; a[e] = grstd[gl] * gv[e]; bt[e] = bv[e];
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int p = pbeg + lane + i * PL;
            if (p < pend) {
                float8 x = RegVec<T>::unpack(cx[i]);
                float xv[8] = F8_TO_ARR(x);
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    o[e] = fmaf(xv[e] - m[e], a[e], bt[e]);
                    if (silu) o[e] = silu_f(o[e]);
                }
#if GN_DROP
                if (dthr) drop_apply(o, drop_keep_bits(rng, dbase + (uint64_t)((base + p) * C + c), dthr), dscale);
#endif
                float8 r = {make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7])};
                store8(y + (base + p) * C + c, r);
            }
        }
    }
}

template <int NP, int MODE, int NT = 256>
__global__ __launch_bounds__(NT) void GN_K(gn_bwd_reg_kernel)(const bf16_t* s0, int C0, const bf16_t* s1, int C1, int P, int G, int CBLK,
                                                         const float* gamma, const float* beta, int silu, const bf16_t* dy,
                                                         const float* stats, bf16_t* d0, const bf16_t* add0, bf16_t* d1, const bf16_t* add1, const bf16_t* add0b,
                                                         float* dgamma, float* dbeta, float* sum_img, int sum_ld, float* sum_all,
                                                         float* ws GN_DROP_PARAMS) {
#if GN_DROP
    // the dropped halves of the packed dy are cleared right behind its load (four ANDs per vector); the scale is one multiply
    // where a value is unpacked (1.0f with thr == 0: exact)
    const uint32_t dthr = ctl[0];
    const float dscale = dthr ? __uint_as_float(ctl[1]) : 1.f;
#endif
    constexpr int CS_PITCH = NT + 4;
    const int C = C0 + C1, cpg = div_small(C, rcp_small(G));
    const float inv_cpg = rcp_small(cpg);
    const int VB = CBLK >> 3, PL = div_small(NT, rcp_small(VB));
    const int img = blockIdx.x, cb = blockIdx.y * CBLK;     // image fastest: the channel blocks of one image (they share 128-B lines) land on one XCD
    const int t = threadIdx.x, lane = div_small(t, rcp_small(VB)), v = t - lane * VB, c = cb + v * 8;
    const int ng = div_small(CBLK, inv_cpg), g0 = div_small(cb, inv_cpg);
    const bool on = t < VB * PL && c < C;
    const int chunks = gridDim.z, chunk = blockIdx.z;
    const int plen = chunks == 1 ? P : (P + chunks - 1) / chunks, pbeg = chunk * plen, pend = min(P, pbeg + plen);
    __shared__ float scratch[16 * CS_PITCH];
    __shared__ float csum[32 * 8];
    __shared__ float gsum[2 * 64], sgam[64];
    MDM_T(const unsigned long long ts0 = nstamp_now();)
    if (t >= 128 && t < 128 + CBLK && cb + t - 128 < C) sgam[t - 128] = gamma[cb + t - 128];     // for the group sums behind the column sums
    if (t < 2 * ng) {
        float a = 0.f;
        if (MODE == 2)
            for (int ch = 0; ch < chunks; ++ch) a += ws[(((int64_t)img * chunks + ch) * G + g0 + (t >> 1)) * 2 + (t & 1)];
        gsum[t] = a;
    }
    const int64_t base = (int64_t)img * P;
    uint4 cx[NP], cd[NP];
    // the tensors ADDED to dx (accumulated gradient / residual branch) are fetched with x and dy, not behind the reduction:
    // a second exposed memory round trip on a kernel that is one round trip + a reduction long
    constexpr bool PRE_ADD = NP <= 4;
    uint4 cadd[PRE_ADD ? NP : 1], caddq[PRE_ADD ? NP : 1];
    // single-launch mode with a small slice: dy * silu'(..) is kept in fp32 registers for the apply pass instead of being
    // recomputed (exp + rcp per element: the large-map kernels are VALU-bound, 1 wave per SIMD)
    constexpr bool CACHE = MODE == 0 && NP <= 8;
    float gzc[CACHE ? NP : 1][8];
    float ga[8], be[8], mean[8], rstd[8], nmr[8], za[8], zb[8];
    float part[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) part[k] = 0.f;
    MDM_T(unsigned long long ts1 = 0;)
    if (on) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int p = pbeg + lane + i * PL;
            bool ok = p < pend;
            cx[i] = ok ? *reinterpret_cast<const uint4*>(src_ptr(s0, s1, C0, C1, base + p, c)) : make_uint4(0, 0, 0, 0);
            cd[i] = ok ? *reinterpret_cast<const uint4*>(dy + (base + p) * C + c) : make_uint4(0, 0, 0, 0);
#if GN_DROP
            if (dthr && ok) {
                const uint4 k = drop_keep_bits(rng, dbase + (uint64_t)((base + p) * C + c), dthr);
                cd[i].x &= k.x; cd[i].y &= k.y; cd[i].z &= k.z; cd[i].w &= k.w;
            }
#endif
            if (PRE_ADD) {
                const bf16_t* ap = c < C0 ? add0 : add1;
                const int cc2 = c < C0 ? c : c - C0, CS2 = c < C0 ? C0 : C1;
                cadd[i] = (ok && ap) ? *reinterpret_cast<const uint4*>(ap + (base + p) * CS2 + cc2) : make_uint4(0, 0, 0, 0);
                caddq[i] = (ok && add0b && c < C0) ? *reinterpret_cast<const uint4*>(add0b + (base + p) * C0 + c) : make_uint4(0, 0, 0, 0);
            }
        }
        {
            const float4 g_lo = *reinterpret_cast<const float4*>(gamma + c), g_hi = *reinterpret_cast<const float4*>(gamma + c + 4);
            const float4 b_lo = *reinterpret_cast<const float4*>(beta + c), b_hi = *reinterpret_cast<const float4*>(beta + c + 4);
            ga[0] = g_lo.x; ga[1] = g_lo.y; ga[2] = g_lo.z; ga[3] = g_lo.w; ga[4] = g_hi.x; ga[5] = g_hi.y; ga[6] = g_hi.z; ga[7] = g_hi.w;
            be[0] = b_lo.x; be[1] = b_lo.y; be[2] = b_lo.z; be[3] = b_lo.w; be[4] = b_hi.x; be[5] = b_hi.y; be[6] = b_hi.z; be[7] = b_hi.w;
            // 8 consecutive channels touch at most 8/cpg + 1 groups; load each group's pair once
            const int gA = div_small(c, inv_cpg);
            float2 st_prev = *reinterpret_cast<const float2*>(stats + ((int64_t)img * G + gA) * 2);
            int g_prev = gA;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int grp = div_small(c + e, inv_cpg);
                if (grp != g_prev) { st_prev = *reinterpret_cast<const float2*>(stats + ((int64_t)img * G + grp) * 2); g_prev = grp; }
                mean[e] = st_prev.x; rstd[e] = st_prev.y;
            }
        }
        MDM_T(ts1 = nstamp_now();)
        // (round 4: these kernels are VALU-bound -- ~60 vector instructions per element at two waves per SIMD, finding 48.  The
        // normalisation and the affine map are one fma each from per-channel constants, and only TWO sums are kept per channel:
        // sum(gz xh) = dgamma and sum(gz) = dbeta; the group sums of gz gamma and gz gamma xh are gamma-weighted sums of those
        // two over the group's channels, taken once behind the column sums: 16 quantities through block_colsum instead of 32.)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            nmr[e] = -mean[e] * rstd[e];                     // xh = fma(x, rstd, nmr)
            za[e] = rstd[e] * ga[e]; zb[e] = fmaf(nmr[e], ga[e], be[e]);      // gamma xh + beta = fma(x, za, zb)
        }
        if (MODE != 2) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (pbeg + lane + i * PL < pend) {
                float8 x = unpack8(cx[i]), d = unpack8(cd[i]);
                float xv[8] = F8_TO_ARR(x);
                float dv[8] = F8_TO_ARR(d);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float xh = fmaf(xv[e], rstd[e], nmr[e]);
                    float gz = GN_DZ(dv[e]);
                    if (silu) gz *= silu_grad_f(fmaf(xv[e], za[e], zb[e]));
                    if (CACHE) gzc[CACHE ? i : 0][e] = gz;
                    part[e] = fmaf(gz, xh, part[e]); part[8 + e] += gz;                      // dgamma, dbeta
                }
            }
        }
        }
    }
    if (MODE != 2) {
        block_colsum<16, NT>(part, scratch, csum, t, VB, PL);      // csum[(q*8+e)*VB + v], q = {dgamma, dbeta}
        if (t < CBLK && cb + t < C) {            // across images: one float atomic per (image, channel) (bf16 path)
            const int vv = t >> 3, e = t & 7;
            atomicAdd(&dgamma[cb + t], csum[e * VB + vv]);
            atomicAdd(&dbeta[cb + t], csum[(8 + e) * VB + vv]);
        }
        if (t >= 64 && t < 64 + ng) {            // inside the workgroup: fixed order (a second wave, next to the atomics above)
            const int gi = t - 64;
            float a1 = 0.f, a2 = 0.f;            // sum over the group's channels of gamma dbeta / gamma dgamma, in channel order
            for (int lc = gi * cpg; lc < (gi + 1) * cpg; ++lc) {
                const float gm = sgam[lc];
                a1 = fmaf(gm, csum[(8 + (lc & 7)) * VB + (lc >> 3)], a1);
                a2 = fmaf(gm, csum[(lc & 7) * VB + (lc >> 3)], a2);
            }
            gsum[2 * gi] += a1; gsum[2 * gi + 1] += a2;
        }
    }
    MDM_T(const unsigned long long ts2 = nstamp_now();)
    __syncthreads();
    if (MODE == 1) {
        if (t < 2 * ng && g0 + (t >> 1) < G) ws[(((int64_t)img * chunks + chunk) * G + g0 + (t >> 1)) * 2 + (t & 1)] = gsum[t];
        if (sum_img && chunk == 0 && t < CBLK && cb + t < C) sum_img[(int64_t)img * sum_ld + cb + t] = 0.f;
        return;
    }
    MDM_T(const unsigned long long ts3 = nstamp_now(); const unsigned long long ts4 = ts3;)
    float k1[8], k2[8], ag[8];              // dx = ag gz - (k2 xh + k1) = fma(ag, gz, -fma(x, k2 rstd, k2 nmr + k1))
    if (on) {
        const float inv_cnt = 1.f / ((float)cpg * (float)P);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int gl = div_small(c + e, inv_cpg) - g0;
            const float q1 = rstd[e] * gsum[2 * gl] * inv_cnt, q2 = rstd[e] * gsum[2 * gl + 1] * inv_cnt;
            k1[e] = fmaf(q2, nmr[e], q1);
            k2[e] = q2 * rstd[e];
            ag[e] = za[e];
        }
    }
    float sx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
        bf16_t* dst; const bf16_t* addp; int cc, CS;
        if (c < C0) { dst = d0; addp = add0; cc = c; CS = C0; } else { dst = d1; addp = add1; cc = c - C0; CS = C1; }
        const bf16_t* addq = c < C0 ? add0b : nullptr;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int p = pbeg + lane + i * PL;
            if (p < pend) {
                float8 x = unpack8(cx[i]), d = unpack8(cd[i]);
                float xv[8] = F8_TO_ARR(x);
                float dv[8] = F8_TO_ARR(d);
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float gz;
                    if (CACHE) gz = gzc[CACHE ? i : 0][e];
                    else { gz = GN_DZ(dv[e]); if (silu) gz *= silu_grad_f(fmaf(xv[e], za[e], zb[e])); }
                    o[e] = fmaf(ag[e], gz, -fmaf(xv[e], k2[e], k1[e]));
                    sx[e] += o[e];
                }
                bf16_t* q = dst + (base + p) * CS + cc;
                if (addp) {
                    float8 old = PRE_ADD ? unpack8(cadd[PRE_ADD ? i : 0]) : load8(addp + (base + p) * CS + cc);
                    float ov[8] = F8_TO_ARR(old);
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] += ov[e];
                }
                if (addq) {
                    float8 old2 = PRE_ADD ? unpack8(caddq[PRE_ADD ? i : 0]) : load8(addq + (base + p) * CS + cc);
                    float ov2[8] = F8_TO_ARR(old2);
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] += ov2[e];
                }
                float8 r = {make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7])};
                store8(q, r);
            }
        }
    }
    if (sum_img || sum_all) {            // uniform
        block_colsum<8, NT>(sx, scratch, csum, t, VB, PL);
        if (t < CBLK && cb + t < C) {
            const float r = csum[(t & 7) * VB + (t >> 3)];
            if (sum_img) {
                if (MODE == 0) sum_img[(int64_t)img * sum_ld + cb + t] = r;         // single writer
                else atomicAdd(&sum_img[(int64_t)img * sum_ld + cb + t], r);        // zeroed by the MODE 1 launch
            }
            if (sum_all) atomicAdd(&sum_all[cb + t], r);
        }
    }
#ifdef MDM_STAMP
    {
        const unsigned long long ts5 = nstamp_now();
        const unsigned widx = (blockIdx.y * gridDim.x + blockIdx.x) * 4 + (t >> 6);
        if ((t & 63) == 0 && widx < 4096) {
            unsigned long long* r = g_nstamp_buf + widx * 16;
            r[0] = 1; r[1] = ts1 - ts0; r[2] = ts2 - ts1; r[3] = ts3 - ts2; r[4] = ts4 - ts3; r[5] = ts5 - ts4; r[6] = ts0; r[7] = ts5;
        }
    }
#endif
}
