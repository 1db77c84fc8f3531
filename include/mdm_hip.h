/*
 * mdm_hip.h -- C ABI of libmdm_hip.so: the MI355X (gfx950) kernels under the
 * masked-diffusion train step and reverse sampler.
 *
 * The reference (hytae1993/masked-diffusion-model) has no FFI: its hot path is
 * Python calling ATen ops.  Each entry point below replaces the ATen call sites
 * named in its comment (file:line relative to /root/reference/code).  The Python
 * host in masked-diffusion-model_amd/mdm binds these with ctypes and keeps the
 * reference's Scheduler / Sampler / Trainer / model(x,t).sample surface.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless the
 *     name ends in _host.  The caller owns all buffers (incl. workspaces).
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered,
 *     nothing synchronises, nothing allocates -> every call is graph-capturable.
 *   - return 0 on success, negative on error; mdm_last_error() gives the
 *     thread-local message.  Nothing throws across the ABI.
 *   - dtype: MDM_F32 = 0 (exact-fp32 VALU contraction path, used for parity),
 *            MDM_BF16 = 1 (bf16 storage, MFMA 16x16x32 contractions, fp32 accumulate).
 *   - activations are NHWC with the channel count a multiple of 8; images enter
 *     and leave as NCHW fp32 exactly like the reference's tensors.
 */
#ifndef MDM_HIP_H
#define MDM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDM_F32 0
#define MDM_BF16 1

const char* mdm_last_error(void);
int mdm_version(void);
/* number of visible HIP devices, or negative */
int mdm_device_count(void);

/* ------------------------------------------------------------------------- *
 * Contractions.  One descriptor drives the three MFMA/VALU contraction
 * kernels; it replaces F.conv2d (unet6.py:232-235) forward, its autograd
 * dgrad/wgrad, F.linear (unet6.py:170-171), the 1x1 convs and the two einsums
 * of AttentionBlock.qkv (unet6.py:316-324) plus their backward products.
 *
 * layout 0 (NT): D[m][n] = sum_k A[m][k] * B[n][k]      A rows gathered if conv
 * layout 1 (NN): D[m][n] = sum_k A[m][k] * B[k][n]      A rows gathered if conv
 * layout 2 (TN): D[m][n] = sum_k A[k][m] * B[k][n]      B rows gathered if conv
 *
 * conv != 0 turns the gathered operand into an implicit im2col over NHWC
 * sources: row index = (img, oy, ox) over OH x OW, reduction index k = tap*Ck+c
 * (layouts 0/1) or row index k = pixel with the tap taken from the grid
 * (layout 2, weight gradient).  Two sources give the channel concat of
 * unet6.py:501 without materialising it; ups=1 reads the source through a
 * nearest x2 upsample (unet6.py:472); stride/pad_t/pad_l cover SamePad2d +
 * stride-2 (unet6.py:257-272, 438-440); transposed=1 is the data-gradient form.
 * ------------------------------------------------------------------------- */
typedef struct mdm_gemm_desc {
    int32_t dtype;              /* MDM_F32 | MDM_BF16: element type of A, B, sources, resid and (unless out_f32) D */
    int32_t layout;             /* 0 NT, 1 NN, 2 TN */
    int32_t M, N, K;
    int32_t batch;              /* >= 1; blockIdx.z when conv == 0 */
    int64_t sA, sB, sD, sR;     /* batch strides in elements */
    const void* A; int32_t lda;
    int32_t f32_split;          /* dtype MDM_F32, layout 0: 1 = the register-staged fp32 kernel may multiply as bf16 hi / lo pairs (see B_split) */
    const void* B; int32_t ldb; int32_t _p1;
    /* implicit-GEMM gather */
    int32_t conv;
    int32_t OH, OW;             /* row space of the gathered operand */
    int32_t IH, IW;             /* logical source extent (after the virtual upsample) */
    int32_t KH, KW, stride, pad_t, pad_l, transposed, ups;
    int32_t C0, C1;             /* channels taken from src0 / src1 */
    int32_t Ck;                 /* reduction channels per tap (layouts 0/1) */
    const void* src0; const void* src1;
    int32_t ld0, ld1;           /* pixel pitch of each source in elements */
    int64_t wtap;               /* weight offset per tap in elements (layouts 0/1) */
    /* epilogue */
    void* D0; void* D1;         /* columns [0,N0) -> D0, [N0,N) -> D1 */
    int32_t ldd0, ldd1, N0;
    int32_t out_f32;            /* D is fp32 regardless of dtype */
    float alpha;
    int32_t acc0, acc1;         /* D += instead of D = */
    const float* bias;          /* [N] or NULL */
    const float* rowvec;        /* [M / rows_per_img][rv_ld] fp32 or NULL (time-embedding add, unet6.py:359) */
    int32_t rv_ld, rows_per_img;
    const void* resid;          /* [M][ldr] or NULL (residual add, unet6.py:333,362) */
    int32_t ldr;
    int32_t splitk;             /* reduction split over grid z (0 = choose; conv layouts 0/1 never split) */
    int64_t dtap;               /* layout 2 + conv: D0 offset per tap */
    /* split-K workspace (optional).  With it, every split writes its fp32 partial tile with plain
     * stores into ws[split][tap|batch][M][N] and a second kernel sums the splits into D0 -- float
     * atomics from dozens of workgroups into one tile serialise at the memory side AND sum in arrival
     * order.  Without it (or when D0 is not a dense [tap|batch][M][N] block) the reduction is not
     * split: there is no atomic fallback, results do not depend on scheduling. */
    void* ws; int64_t ws_bytes;
    /* layout 2, bf16: if set, dbias[m] += sum_k A[k][m] (the bias gradient of a convolution is the column
     * sum of dY, which the weight-gradient kernel already holds as MFMA fragments: one extra MFMA against
     * a ones-fragment per k-step in the tap-0 / first-column workgroups, fp32 atomics at the end). */
    float* dbias;
    /* Fused GroupNorm backward (unet6.py:291-293 backward) in the epilogue of the DATA GRADIENT of the conv that
     * consumes the normalised tensor, on the whole-image tiles of the 4x4 / 8x8 maps (mdm_gemm_can_fuse_gn_bwd says
     * whether this descriptor qualifies): the contraction result is d(z), z = silu?(GroupNorm(x)); instead of storing
     * it, the epilogue reads x, stats (mean, rstd per image and group), gamma, beta and writes dx into D0 (acc0 honoured),
     * adds dgamma / dbeta, and optionally the column sums of dx (gnb_sum_img[n * gnb_sum_ld + c] = sum_p dx,
     * gnb_sum_all[c] += sum_{n,p} dx) like sum_img / sum_all of mdm_gn_desc.  gnb_add (with acc0 == 0): a tensor laid out like D0
     * whose values are added to dx (the gradient arriving over the residual branch, unet6.py:362).  NULL gnb_x = plain epilogue. */
    const void* gnb_x; const float* gnb_stats; const float* gnb_gamma; const float* gnb_beta;
    float* gnb_dgamma; float* gnb_dbeta; float* gnb_sum_img; float* gnb_sum_all;
    int32_t gnb_G, gnb_silu, gnb_sum_ld, _p3;
    const void* gnb_add;
    /* Fused GroupNorm FORWARD in the epilogue of the conv that PRODUCES the tensor, same tiles (mdm_gemm_can_fuse_gn_fwd):
     * after the usual epilogue has stored y (bf16), the workgroup normalises the values it just rounded:
     * gnf_out = silu?(GroupNorm_G(y) * gamma + beta) (bf16, same shape as y), gnf_stats[n][g] = (mean, rstd).
     * NULL gnf_out = plain epilogue. */
    void* gnf_out; const float* gnf_gamma; const float* gnf_beta; float* gnf_stats;
    int32_t gnf_G, gnf_silu; float gnf_eps; int32_t _p4;
    /* dtype MDM_F32, optional: the filters of B once more, written by mdm_split_shadow (same offsets and leading dimension as B).
     * With it, a 3x3 stride-1 forward convolution that qualifies for the halo kernel multiplies on the bf16 matrix pipe with fp32
     * storage and fp32 accumulation: every operand x = hi + lo (hi = bf16(x), lo = bf16(x - hi)), a product = hi*hi + hi*lo + lo*hi
     * -- relative error <= ~2^-16 per product instead of 2^-24, at a fifth of the matrix time of the exact path.  Descriptors that do
     * not qualify ignore it and run the exact fp32 path on B.  NULL = exact fp32 everywhere (the parity path).
     * (NaN operands stay NaN; an infinite operand becomes NaN -- Inf - bf16(Inf) is NaN -- where the exact path would give +-Inf.) */
    const void* B_split;
} mdm_gemm_desc;

int mdm_gemm(const mdm_gemm_desc* desc_host, void* stream);
/* Two INDEPENDENT contractions (neither reads what the other writes), in one launch where the pair is a 3x3 halo convolution
 * `a` and a 1x1 convolution `b` of the shapes a ResidualBlock produces (conv1 next to the skip projection, unet6.py:350-362;
 * conv2's data gradient next to the skip projection's): the workgroups of `b` follow those of `a` in the same grid.
 * Every other pair runs as mdm_gemm(a) then mdm_gemm(b): the results are the same either way. */
int mdm_gemm_pair(const mdm_gemm_desc* a_host, const mdm_gemm_desc* b_host, void* stream);
/* What mdm_gemm would choose for this descriptor given unlimited workspace: the split count and the
 * workspace bytes it needs (0 when it would not use partial slabs).  No launch. */
int mdm_gemm_plan(const mdm_gemm_desc* desc_host, int* splitk_out, int64_t* ws_bytes_out);
/* 1 if mdm_gemm would run this descriptor (a bf16 3x3 data gradient through the transposed filters) on the whole-image
 * halo tiles AND groups of G channels are whole inside a 64-channel tile, i.e. the gnb_* epilogue may be used; else 0. */
int mdm_gemm_can_fuse_gn_bwd(const mdm_gemm_desc* desc_host, int G);
/* the same question for the gnf_* epilogue of a bf16 3x3 forward convolution */
int mdm_gemm_can_fuse_gn_fwd(const mdm_gemm_desc* desc_host, int G);
/* Route record (tests): the kernel and second stage ("+tapsplit" epilogue, "+splitk" reduce) the last mdm_gemm, mdm_gemm_pair
 * ("pair:two launches" when it ran two mdm_gemm) or mdm_wgrad_group_launch call on THIS host thread launched, e.g.
 * "halo<256,6,NSB,64,f32,split>", "lin2<64,64>+tapsplit"; "none" before the first call or when validation failed.  Host-side only. */
const char* mdm_gemm_last_route(void);
/* The name mdm_gemm_last_route would give after mdm_gemm(desc) / mdm_gemm_pair(a, b) -- the descriptor's own ws / ws_bytes decide
 * the split, as in a launch -- without launching: host arithmetic only, the pointers are never dereferenced, no device is
 * touched and the record of the last launch stays as it is.  "none" (and mdm_last_error) when the descriptor is refused. */
const char* mdm_gemm_route_of(const mdm_gemm_desc* desc_host);
const char* mdm_gemm_pair_route_of(const mdm_gemm_desc* a_host, const mdm_gemm_desc* b_host);
/* The first launch mdm_gemm(desc) would make, without making it.  out[0] workgroups (grid.x), out[1] grid.z, out[2] threads per
   workgroup, out[3] dynamic LDS bytes, out[4], out[5] the route's output tile (0, 0: the grid is not a tiling of the output).
   0, or -1 with mdm_last_error set exactly where mdm_gemm refuses.  Host arithmetic; pointers are not dereferenced. */
int mdm_gemm_launch_of(const mdm_gemm_desc* desc, int32_t out[6]);
/* The fused launch of mdm_gemm_pair(a, b); 1 and zeros for "pair:two launches" (ask mdm_gemm_launch_of about each). */
int mdm_gemm_pair_launch_of(const mdm_gemm_desc* a, const mdm_gemm_desc* b, int32_t out[6]);
/* every route name mdm_gemm_last_route can return: fills up to `cap` of them into out (may be NULL), returns how many there are */
int mdm_gemm_route_names(const char** out, int cap);

/* ------------------------------------------------------------------------- *
 * A GROUP of weight gradients in ONE launch (autograd's conv2d weight gradient, unet6.py:232-235).
 * The weight gradient of a convolution only READS dY and the layer input; both stay in memory until the end of
 * the backward pass, so the host may collect the (layout 2, conv) descriptors of a whole stretch of the backward
 * and run them together: every contraction is cut into work items (output tile x filter tap x k-range), the items of
 * all layers are sorted longest first and launched as one flat grid, followed by ONE launch that sums the split-K
 * partial slabs of the layers that were split.  The group fills the chip, so a layer needs only the k-splits that
 * balance asks for (descriptor.splitk > 0 is honoured, 0 = the per-layer rule of mdm_gemm).
 *   mdm_wgrad_group_accepts   1 if the descriptor can be a member (bf16, layout 2, conv, dense fp32 [tap][M][N] output,
 *                             geometry of the linear-gather kernel), else 0 (run it through mdm_gemm instead).
 *   mdm_wgrad_group_create    resolves the n HOST descriptors (operands must already be the final device pointers;
 *                             a descriptor with splitk > 1 needs its own ws slice), builds the item table and copies
 *                             both into dev_buf (device memory owned by the caller, kept alive as long as the handle).
 *                             *need_bytes_out = bytes dev_buf must hold; with dev_buf == NULL or too small nothing is
 *                             built (*handle_out = NULL, return 0): call once to size, once to build.  Synchronous
 *                             (hipMemcpy): call it outside stream capture.
 *   mdm_wgrad_group_launch    the launches of the group, stream-ordered and capturable.  D0 = (acc0 ? D0 : 0) + dW.
 *   mdm_wgrad_group_destroy   frees the host-side handle (not dev_buf).
 * Nine-tap form.  3x3 stride-1 members (maps 8 / 16 / 32 / 64 wide, overwrite form) whose group gives every CU a share
 * of >= MDM_TAPS_MIN_SHARE (default 48) 64-pixel slabs run all nine taps in one pass over dY and the input (wgrad_taps_body):
 * the group is then ONE persistent launch of one workgroup per CU walking its column of the item table -- equal contiguous
 * shares of the (tile, slab) space, the remaining per-tap items in the same queues -- plus the split-K sum of per-tap layers
 * and tile_parts_reduce_kernel, which adds the fp32 partial slots of the tiles a share boundary cut.  The slots live in
 * dev_buf too (they are part of *need_bytes_out: ~80 MB for the whole cfg2 backward), descriptor.splitk / ws of such a member
 * are ignored.  Same results as the per-tap form up to fp32 summation order.  Environment: MDM_WGRAD_TAPS=0 keeps every layer
 * on the per-tap kernels; MDM_TAPS_DEBUG=1 prints the schedule of each group; MDM_WGRAD_RESERVE_CUS=r builds the persistent nine-tap
 * launch for CUs - r workgroups (data-parallel runs: room for the collective's kernels beside it).
 *
 * dev_buf, in this order, every section but the last padded to a multiple of 256 bytes:
 *   1. descriptors   n x mdm_gemm_desc, resolved (splitk = 1 on nine-tap members)
 *   2. flat items    per-tap form only: [entry][8 queues] item words, workgroup b of the flat grid takes word b
 *   3. taps table    merged form only: [round][queue] item words, queue = one workgroup per CU (less the reserve)
 *   4. part tiles    one 48-byte record per nine-tap tile that was cut: {float* dst; int64 dtap; int32 N, m0, n0, first_slot,
 *                    parts, rows, cols, pad}
 *   5. slots         nslots x [9][128][64] fp32 partial sums of the parts of the cut tiles
 * A group has either section 2 (form 0, "wgrad_group") or sections 3-5 (form 1, "wgrad_taps_group"), never both.
 * The item word is four int32 {x, y, z, w}:
 *   x  descriptor index, -1 = padding
 *   w  kind: 0 = 64x64, 1 = 128x128, 2 = 256x128 per-tap tile, 3 = nine-tap tile
 *   per-tap (w < 3):  y = item index inside the descriptor, below tiles x taps x splitk;  z = tiles (of that kind) per tap and k-split
 *   nine-tap (w = 3): y = tile | (slot + 1) << 12 (tile < 4096; slot + 1 = 0: uncut, the tile is stored straight into D0; slot + 1 < 2^19,
 *                     a plan that needs more is refused);  z = k0 | k1 << 16: the 64-pixel slabs [k0, k1) of the reduction
 *
 *   mdm_wgrad_group_schedule  the table mdm_wgrad_group_create would upload for these descriptors on a device of n_cu CUs
 *                             (n_cu is the queue count of the merged form as it stands: MDM_WGRAD_RESERVE_CUS is not applied
 *                             to it, the other environment variables are read as in create).  Host arithmetic only: no
 *                             device is asked, pointers are never dereferenced, mdm_gemm_last_route stays as it is.
 *                             One row of eight int32 per table entry, padding included, in table order:
 *                               [0] queue   entry index % 8 (form 0) or % n_cu (form 1)
 *                               [1] round   entry index / 8 (form 0) or / n_cu (form 1)
 *                               [2] desc    descriptor index; -1 = padding, and [3..7] are then 0
 *                               [3] kind    w of the item word
 *                               [4] tile_or_item   per-tap: the item index (y);  nine-tap: the tile
 *                               [5] k0      per-tap: tiles per tap and k-split (z);  nine-tap: first slab
 *                               [6] k1      per-tap: 0;  nine-tap: one past the last slab
 *                               [7] slot    per-tap: 0;  nine-tap: slot + 1 of the item word (0 = uncut)
 *                             rows_out == NULL (the size query) only fills *n_rows_out, *need_bytes_out (create's) and
 *                             *form_out (0 per-tap, 1 merged); otherwise cap_rows >= *n_rows_out rows of space are required.
 * ------------------------------------------------------------------------- */
int mdm_wgrad_group_accepts(const mdm_gemm_desc* desc_host);
int mdm_wgrad_group_create(const mdm_gemm_desc* descs_host, int n, void* dev_buf, int64_t dev_bytes,
                           int64_t* need_bytes_out, void** handle_out);
int mdm_wgrad_group_schedule(const mdm_gemm_desc* descs_host, int n, int n_cu, int32_t* rows_out, int64_t cap_rows,
                             int64_t* n_rows_out, int64_t* need_bytes_out, int32_t* form_out);
int mdm_wgrad_group_launch(void* handle, void* stream);
int mdm_wgrad_group_destroy(void* handle);

/* ------------------------------------------------------------------------- *
 * fp32 weight gradient with SPLIT products (autograd's conv2d weight gradient, unet6.py:232-235 backward, for fp32 training:
 * UNet(dtype=F32, f32_products="split", grad_products="split")).  Same descriptor as a mdm_gemm weight gradient: dtype MDM_F32,
 * layout 2, conv, out_f32, D0 = dW[tap][M = Cout][N = Cin] (+)= sum_pixels dY[p][m] x[gather(p, tap)][n] -- any geometry the gather
 * takes (3x3 stride 1 / 2, folded x2 upsample, 1x1, one or two sources).  Both operands are fp32 activations, split in registers on
 * their way into LDS (x = hi + lo, hi = bf16(x), lo = bf16(x - hi)); a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16
 * with fp32 accumulation (~2^-16 relative per product instead of 2^-24).  The reduction over the pixels is split over grid z when
 * `ws` can hold the partial slabs ([split][tap][M][N] fp32, dense destination required: ldd0 == N, dtap == M N): plain stores, then
 * one launch sums them in split order -- no float atomics, the same bits on every run.  descriptor.splitk > 0 is honoured, 0 = choose.
 * Plain epilogue only: no bias / dbias / rowvec / resid / D1, alpha 1 (the bias gradient stays on mdm_colsum).
 *   mdm_conv_wgrad_split_plan   the split count and workspace bytes it would use for this descriptor.  No launch.
 *   mdm_wgrad_split_last_route  route record (tests): "wgrad_split<128>", "wgrad_split<64>", either with "+splitk", or "none"
 *                               (before the first call or when validation failed).  Host-side, this thread.
 * Replaces nothing upstream (a faster form of the same contraction mdm_gemm runs exactly).
 * ------------------------------------------------------------------------- */
int mdm_conv_wgrad_split(const mdm_gemm_desc* desc_host, void* stream);
int mdm_conv_wgrad_split_plan(const mdm_gemm_desc* desc_host, int* splitk_out, int64_t* ws_bytes_out);
const char* mdm_wgrad_split_last_route(void);

/* ------------------------------------------------------------------------- *
 * GroupNorm(32, eps) [+ SiLU]  (unet6.py:291-293, 358, 360, 330, 505)
 * x = concat(src0[C0], src1[C1]) along channels, NHWC, P = H*W pixels per image.  One descriptor drives both directions; it is
 * read on the host at call time and its fields become kernel arguments by value (nothing on the device sees the struct).  A
 * zeroed descriptor is a plain GroupNorm with nothing optional: every field a call does not use stays 0 / NULL.
 * One kernel per call (the fp32 backward: two); inside a workgroup every sum has a fixed order.
 * ------------------------------------------------------------------------- */
typedef struct mdm_gn_desc {
    const void* src0; const void* src1; /* the sources (dtype); src1 may be NULL with C1 == 0 */
    const float* gamma; const float* beta; /* [C0 + C1] */
    float* stats;               /* [N][G][2] fp32 (mean, rstd): written by the forward, read by the backward */
    float* ws;                  /* fp32 backward: REQUIRED, >= mdm_groupnorm_bwd_ws_floats() floats -- per-image partial sums that a
                                 * second launch adds in image order: the same bits on every run.  Elsewhere unused, may be NULL */
    /* forward */
    void* y;                    /* [N][P][C0 + C1] (dtype) = silu?(GroupNorm_G(x) * gamma + beta) */
    /* backward: dx goes to dst0 / dst1 (channel split like the sources); dgamma / dbeta are ACCUMULATED (bf16: one fp32 atomic per
     * channel per image; fp32: no atomics, see ws) */
    const void* dy;             /* [N][P][C0 + C1] (dtype) */
    void* dst0;                 /* [N][P][C0]: dst0 = add0 + add0b + dx */
    const void* add0;           /* NULL = none; a tensor laid out like dst0.  dst0 itself gives the accumulating form dst0 += dx; another
                                 * tensor adds the gradient that arrives over a residual branch (x + block(x), unet6.py:333, 362) WITHOUT
                                 * modifying that tensor, which a later (grouped) weight gradient still reads */
    const void* add0b;          /* NULL = none; a SECOND tensor laid out like dst0 that is added too -- an activation with two forward
                                 * consumers and a residual join receives dst0 (accumulate) + the residual branch's dY + dx in one pass */
    void* dst1;                 /* [N][P][C1]: dst1 = add1 + dx; may be NULL with C1 == 0 */
    const void* add1;           /* NULL = none; like add0 */
    float* dgamma; float* dbeta; /* [C0 + C1] fp32, += */
    /* column sums of the dx it writes (the complete gradient of a conv output); one source only (C1 == 0); either may be NULL */
    float* sum_img;             /* sum_img[n * sum_ld + c] = sum_p dx (the time-embedding gradient, unet6.py:359) */
    float* sum_all;             /* sum_all[c] += sum_{n,p} dx (that conv's bias gradient) */
    /* Dropout on the GroupNorm output, fused into the same kernels (nn.Dropout between silu(norm2(.)) and conv2 of a ResidualBlock,
     * unet6.py:354, 360): y = silu?(GN(x)) * keep * scale in the forward, dz = dy * keep * scale right behind the load of dy in the
     * backward -- no extra pass over memory, no stored mask.  rng == NULL: no dropout (drop_base and ctl are ignored).  Otherwise one
     * source only (C1 == 0), ctl != NULL and drop_base % 8 == 0.  Element e = (n*P + p)*C + c has the global index g = drop_base + e
     * (drop_base: the caller's running element count of the dropout sites before this one); its random word is the 16-bit lane g & 7 of
     * Philox4x32-10(key = rng[0], counter = {g >> 3, rng[1] * 8 + 5}) (lane j = half j & 1 of 32-bit word j >> 1, low half first).
     * An element is kept iff its lane >= thr, kept values are multiplied by scale (thr = clamp(round(rate * 65536), 0, 65535),
     * scale = 65536 / (65536 - thr)), dropped ones are exact zeros; thr == 0 (eval mode: {0, 1.0f}) draws nothing and gives the bits
     * of a descriptor without rng. */
    const uint64_t* rng;        /* {seed, offset} as for mdm_rng_advance: forward and backward of one step must see the same offset */
    uint64_t drop_base;
    const uint32_t* ctl;        /* {uint32 thr, float scale} in device memory */
    int32_t dtype;              /* MDM_F32 | MDM_BF16: element type of the sources, y, dy, dst and add tensors */
    int32_t N, P, G;            /* images, pixels per image, groups */
    int32_t C0, C1;             /* channels taken from src0 / src1 (multiples of 8) */
    int32_t silu;               /* != 0: SiLU behind the normalisation */
    int32_t sum_ld;             /* row pitch of sum_img in floats */
    float eps;                  /* forward only */
    int32_t _pad;
} mdm_gn_desc;

/* reads src0, src1, gamma, beta; writes y and stats */
int mdm_groupnorm_fwd(const mdm_gn_desc* desc_host, void* stream);
/* reads src0, src1, gamma, beta, stats, dy and the add tensors; writes dst0, dst1, sum_img and adds to dgamma, dbeta, sum_all */
int mdm_groupnorm_bwd(const mdm_gn_desc* desc_host, void* stream);
/* Which kernel runs (tests): the choice is one pure host function of (direction, dtype, N, P, G, C0 + C1), and these three ask it
 * without any device work.  Storage type and dropout are not part of a name.
 *   mdm_gn_route_of     which = 0 forward, 1 backward -> "fwd_reg<4,512>" (register-cached, <vectors per lane, threads>), "fwd",
 *                       "bwd_reg<2,256>", "bwd", "bwd+reduce" (the fp32 backward: two launches), ...; NULL, with the message in
 *                       mdm_last_error, for a shape or dtype the entry points refuse.  What they require of the pointers (ws, ctl,
 *                       one source under rng or the column sums) is not asked here.
 *   mdm_gn_last_route   what the last mdm_groupnorm_fwd / mdm_groupnorm_bwd call of this thread launched; "none" before the first
 *                       call and after a refused one
 *   mdm_gn_route_names  every name the two can return: fills up to `cap` of them into out (may be NULL), returns how many */
const char* mdm_gn_route_of(int which, const mdm_gn_desc* desc_host);
const char* mdm_gn_last_route(void);
int mdm_gn_route_names(const char** out, int cap);

/* floats mdm_groupnorm_bwd writes into `ws` for an [N][P][C] problem of this dtype (0: `ws` may be NULL): the entry point cannot check
 * a size it is not given. */
int64_t mdm_groupnorm_bwd_ws_floats(int dtype, int N, int C);

/* keep[i] = 1 / 0 for the n consecutive elements from global index `base` on (any base): the mask a descriptor with this rng / ctl
 * applies, for tests and debugging. */
int mdm_dropout_mask(const uint64_t* rng, uint64_t base, const uint32_t* ctl, int64_t n, uint8_t* keep, void* stream);

/* ------------------------------------------------------------------------- *
 * Fused single-head attention of AttentionBlock.qkv (unet6.py:316-324): o = softmax(q k^T * scale) v over L tokens,
 * qkv = [N][L][3C] (q | k | v) as project_in writes it (NHWC), o = [N][L][C]; bf16, C in {32, 64, 128, 256},
 * L % 16 == 0 (mdm_attn_supported).  One forward launch (online softmax over 64-key tiles, the scores never reach
 * memory), lse[N][L] = log-sum-exp of the scaled scores per query (fp32) is kept for the backward.
 * Backward: two launches -- dQ (also writes delta[N][L] = sum_d dO*O) and dK/dV -- recomputing P from q, k, lse;
 * dqkv = [N][L][3C] is written completely (dq | dk | dv), nothing is accumulated.
 * Replaces both einsums, the softmax and `.contiguous()` of unet6.py:319-324 and their autograd backward.
 * ------------------------------------------------------------------------- */
int mdm_attn_supported(int dtype, int L, int C);
/* Which of the fused kernels runs (tests): the kernel choice is one pure host function of (direction, dtype, L, C), and these
 * three ask it without any device work.
 *   mdm_attn_route_of     which = 0 forward, 1 backward -> "fwd<128>", "fwd_dma<256>", "bwd<32>", "bwd_dma<64>", ...;
 *                         NULL for a request mdm_attn_fwd / mdm_attn_bwd would refuse (the backward needs L <= 4096)
 *   mdm_attn_last_route   what the last mdm_attn_fwd / mdm_attn_bwd call of this thread launched; "none" before the first call
 *                         and after a refused one
 *   mdm_attn_route_names  every name the two can return: fills up to `cap` of them into out (may be NULL), returns how many */
const char* mdm_attn_route_of(int which, int dtype, int L, int C);
const char* mdm_attn_last_route(void);
int mdm_attn_route_names(const char** out, int cap);
/* Exact-fp32 forward of the same attention for short sequences (L in {16, 32, 48, 64}, C in {64, 128, 256}: the 8x8 / 4x4 attention
 * blocks on the fp32 path): one launch on v_mfma_f32_16x16x4_f32 instead of two batched contractions and a softmax launch.  It also
 * writes the probabilities S[N][L][L] (fp32) -- what the unfused fp32 backward (softmax_bwd + three contractions) reads. */
int mdm_attn_f32_small_supported(int L, int C);
int mdm_attn_f32_small_fwd(const float* qkv, float* o, float* S, int N, int L, int C, float scale, void* stream);
int mdm_attn_fwd(int dtype, const void* qkv, void* o, float* lse, int N, int L, int C, float scale, void* stream);
int mdm_attn_bwd(int dtype, const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv,
                 int N, int L, int C, float scale, void* stream);

/* The same attention with MANY SMALL heads on separate q, k, v, o tensors [N][L][C], head h = channels [h D, (h+1) D),
 * D = C / heads in {8, 16, 32}, any L, bf16 or fp32: diffusers' attention blocks inside UNet2DModel (attention_head_dim = 8;
 * reference utils/model.py:24-32 builds them).  lse / delta are [N][heads][L] fp32.  dq, dk, dv are written completely. */
int mdm_attn_mh_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int N, int L, int C,
                    int heads, float scale, void* stream);
int mdm_attn_mh_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                    float* delta, void* dq, void* dk, void* dv, int N, int L, int C, int heads, float scale, void* stream);

/* row softmax of S[rows][L] in place (unet6.py:320-322), and its backward
 * dS = P * (dP - sum_j dP*P) written over dP. */
int mdm_softmax_fwd(int dtype, void* S, int rows, int L, void* stream);
int mdm_softmax_bwd(int dtype, const void* P, void* dP, int rows, int L, void* stream);

/* y[N][dim] = [sin(t*f) | cos(t*f)], f_i = exp(-i*ln(1e4)/(dim/2-1))  (unet6.py:18-34); fp32 */
int mdm_timestep_embedding(const float* t, int N, int dim, float* y, void* stream);
/* general form: flip_sin_to_cos puts the cosines first, the exponent is -i ln(1e4) / (dim/2 - freq_shift)
 * (diffusers `Timesteps(flip_sin_to_cos=True, downscale_freq_shift=0)` as UNet2DModel builds it; (0, 1) = the call above) */
int mdm_timestep_embedding2(const float* t, int N, int dim, int flip_sin_to_cos, float freq_shift, float* y, void* stream);
/* fp32 SiLU on small [n] vectors (unet6.py:397, 359) and its backward (dx = dy * silu'(x), acc adds) */
int mdm_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int mdm_silu_bwd(const float* x, const float* dy, float* dx, int acc, int64_t n, void* stream);

/* The linear layers of the time-embedding path (unet6.py:395-399 `embed`, unet6.py:350 the per-block projections, all in one
 * [sum Cout][temb] matrix) and their data gradients: fp32 contractions whose row count M is the batch.  M <= 128,
 * N % 16 == 0, K % (64 * splits) == 0 (mdm_skinny_supported); larger batches go through mdm_gemm.
 *   fwd: y[M][N] = x[M][K] W[N][K]^T + bias; act_out (may be NULL) = silu(y).  With x == NULL the input is the sinusoidal
 *        embedding of t[M] (dimension K, as mdm_timestep_embedding2), also stored to emb_out[M][K] when that is not NULL.
 *   bwd: dx[M][N] = dy[M][K] W[K][N] (* silu'(pre[M][N]) when pre != NULL); with splits > 1 the reduction is cut into
 *        `splits` ranges whose fp32 partial results go to slabs[splits][M][N] (pre and dx unused) for mdm_silu_bwd_sum.
 *   mdm_silu_bwd_sum: dx[n] = (sum_s slabs[s][n]) * silu'(pre[n]) (pre may be NULL: plain sum).
 * Which instantiation runs (host arithmetic, one rule for the query and both launchers; no device is touched):
 *   mdm_skinny_route_of     which = 0 forward, 1 backward; has_t != 0: the input is the embedding of t (forward only) ->
 *                           "nt<MB,NB>", "nt<MB,1,temb>", "nn<MB,1>": MB = 2 (M <= 32) | 8 sixteen-row blocks, NB sixteen-column
 *                           blocks per workgroup (2 for a forward from a matrix with N >= 2048, N % 32 == 0; else 1: the grid is
 *                           N / (16 NB) workgroups, times `splits` in the backward).  NULL for a shape the entry points refuse
 *                           (the split count and the pointers are not asked here: mdm_skinny_supported, the entry points).
 *   mdm_skinny_last_route   what the last mdm_skinny_linear_fwd / _bwd call of this thread launched; "none" before the first
 *                           call and after a refused one
 *   mdm_skinny_route_names  every name the two can return: fills up to `cap` of them into out (may be NULL), returns how many */
const char* mdm_skinny_route_of(int which, int M, int N, int K, int has_t);
const char* mdm_skinny_last_route(void);
int mdm_skinny_route_names(const char** out, int cap);
int mdm_skinny_supported(int M, int N, int K, int splits);
int mdm_skinny_linear_fwd(const float* x, int ldx, const float* t, int flip_sin_to_cos, float freq_shift, float* emb_out,
                          const float* W, int ldw, const float* bias, int M, int N, int K, float* y, int ldy, float* act_out,
                          void* stream);
int mdm_skinny_linear_bwd(const float* dy, int lddy, const float* W, int ldw, int M, int N, int K, int splits, const float* pre,
                          float* dx, float* slabs, void* stream);
int mdm_silu_bwd_sum(const float* pre, const float* slabs, int nslab, int64_t n, float* dx, void* stream);

/* column sums of dY[N][P][C] (NHWC): per_img[n*ld + c] (= or +=) sum_p, and dbias[c] += sum_{n,p}.
 * Either output may be NULL.  Backward of the bias add (unet6.py:233) and of the
 * time-embedding broadcast add (unet6.py:359). */
int mdm_colsum(int dtype, const void* dY, int N, int P, int C, float* per_img, int ld, int acc_img,
               float* dbias, void* stream);

/* 2x2 sum-pool of g[N][2H][2W][C] into dst[N][H][W][C] (backward of nn.Upsample(2,'nearest'), unet6.py:472) */
int mdm_sumpool2(int dtype, const void* g, void* dst, int acc, int N, int H, int W, int C, void* stream);

/* resample_with_conv=False (unet6.py:441-442, 472-475): the parameter-free resampling.  NHWC, C % 8 == 0, fp32 arithmetic,
 * one rounding to storage, no atomics.
 *   mdm_avgpool2   H, W = OUTPUT extents, src[N][2H][2W][C]: dst[n,h,w,c] = (acc ? dst : 0) + 0.25 (((a + b) + c) + d) over the
 *                  2x2 block, taps in mdm_sumpool2's order.  Forward of nn.AvgPool2d(2) (unet6.py:441-442).
 *   mdm_upsample2  H, W = SOURCE extents, dst[N][2H][2W][C]: dst[n,y,x,c] = (acc ? dst : 0) + scale * src[n,y/2,x/2,c].  Forward of
 *                  nn.Upsample(scale_factor=2, mode="nearest") (unet6.py:472-475; scale 1, acc 0) and backward of the average pool
 *                  (scale 0.25).  The backward of the bare upsample is mdm_sumpool2. */
int mdm_avgpool2(int dtype, const void* src, void* dst, int acc, int N, int H, int W, int C, void* stream);
int mdm_upsample2(int dtype, const void* src, void* dst, int acc, float scale, int N, int H, int W, int C, void* stream);

/* dst += src over n elements of `dtype` (n % 8 == 0): joins two gradient contributions of one activation */
int mdm_add(int dtype, void* dst, const void* src, int64_t n, void* stream);
/* dst = x + y (y == NULL: dst = x) */
int mdm_add3(int dtype, void* dst, const void* x, const void* y, int64_t n, void* stream);

/* layout converters: NCHW fp32 <-> NHWC dtype with the channel count padded to Cp (pad = 0) */
int mdm_nchw_to_nhwc(int dtype, const float* x, void* y, int N, int C, int H, int W, int Cp, void* stream);
int mdm_nhwc_to_nchw(int dtype, const void* x, float* y, int N, int C, int H, int W, int Cp, void* stream);

/* ------------------------------------------------------------------------- *
 * Scheduler kernels (NCHW fp32, like the reference tensors)
 * ------------------------------------------------------------------------- */
/* On-device draw of the per-sample step (trainer_masked_mean_shift.py:109-112,
 * scheduler.py:88-100, 780-794): idx ~ U{0..n_used-1}; t = used[idx]; amount = table[t-1];
 * weight = wtab[idx] (or 1); out2 = table2[t-1] for a second schedule table (the shift ratio; both may be NULL);
 * zero_out[0] = zero_out[1] = 0 (may be NULL: the two-word loss accumulator mdm_loss_fwd_bwd adds to -- this is the first
 * launch of a step).
 * Philox4x32-10 keyed by rng[0]=seed, rng[1]=offset (device memory). */
int mdm_draw_timesteps(const uint64_t* rng, const int32_t* used, int n_used, const double* table,
                       const float* wtab, int N, float* t_out, double* amount_out, float* weight_out,
                       int32_t* idx_out, const double* table2, double* out2, int64_t* zero_out, void* stream);

/* Thresholding mask + fill + degrade (scheduler.py:286-323 == 438-477 == 572-598).
 *   u: [N][Cm*HW] uniforms (replay mode) or NULL (device Philox, stream id `rng_stream`);
 *   mask_in: existing [N][C][HW] keep-mask to use instead of drawing (degrade_with_mask), or NULL;
 *   amount: [N] double ratios (thresholding) ; Cm = 1 ('1-channel') or C ('3-channel');
 *   fill_mode: 0 constant `fill_const`, 1 degraded_area image-wise, 2 degraded_area channel-wise,
 *              3 non_degraded_area (NaN -> 0);
 * outputs (any may be NULL): x_t, mask [N][C][HW] fp32, mean_pixel [N][C]. */
int mdm_degrade(const float* x0, const float* u, const float* mask_in, const double* amount, int amount_stride,
                const uint64_t* rng, int rng_stream, int N, int C, int HW, int Cm, int fill_mode, float fill_const,
                float* x_t, float* mask, float* mean_pixel, void* stream);

/* 'indexing' mode on device (scheduler.py:279-284): keep-mask [N][C][HW] with EXACTLY count[n] zeroed pixels
 * per image (the count smallest of HW Philox keys; same distribution as randperm(HW)[:count], different
 * stream).  The replay mode ships the host's randperm-built mask through mdm_degrade(mask_in=...). */
int mdm_index_mask(const double* count, int count_stride, const uint64_t* rng, int rng_stream, int N, int C, int HW,
                   float* mask, void* stream);

/* Shift (scheduler.py:612-732) + perturb_shift (:757-766):  s = z * ratio,  x_in = x_t + s.
 *   z: [N][zc][zhw] draws (replay) or NULL (device Philox normal(mean,1) / uniform(-1,1) per `kind`);
 *   kind: 0 non_shift, 1 '1-d_constant' (zc=1,zhw=1,uniform), 2 '3-d_constant' (zc=3,zhw=1,uniform),
 *         3 'noise_reduction' (zc=1,zhw=HW,normal), 4 'noise_with_perturbation' (zc=3,zhw=HW,normal),
 *         5 'noise_std_reduction' (zc=3,zhw=HW; s = N(noise_mean, ratio_n); a replayed z IS the shift);
 *   ratio: [N] double; per_column != 0 reproduces the reference's N==W broadcast (ratio indexed by column w);
 *   outputs: s [N][C][HW] (may be NULL), x_in fp32 NCHW (may be NULL), x_in_nhwc (dtype, Cp channels; may be NULL: only the
 *   C real channels of every pixel are written -- the caller provides the pad channels zeroed once, they never change). */
int mdm_shift(const float* x_t, const float* z, const double* ratio, const uint64_t* rng, int rng_stream,
              int kind, float noise_mean, int per_column, int N, int C, int H, int W,
              float* s, float* x_in, int dtype, void* x_in_nhwc, int Cp, void* stream);
/* x_nhwc[pix][C .. Cp) = 0 for npix pixels: what a caller that did not get its buffer from a zeroing allocator runs ONCE
 * before the first mdm_shift on it (mdm_shift leaves the pad channels alone; the first convolution multiplies them by zero
 * weights, so garbage there -- a NaN -- would poison its output and its weight gradient). */
int mdm_zero_pad_channels(int dtype, void* x_nhwc, int64_t npix, int C, int Cp, void* stream);

/* Fused x0-space loss + its gradient (trainer_masked_mean_shift.py:142-159, trainer_masked.py:126-140):
 *   r = (x_in + pred) - s - x0 ;  loss += sum(w_n * r^2) / numel ;  dpred = 2 w_n r / numel * gscale
 * pred, dpred: NHWC dtype with Cp channels (pad channels of dpred are written 0). s, w may be NULL.
 * loss_q40: TWO int64 words the caller zeroes before a step (mdm_draw_timesteps does).  [0] += the loss in Q23.40 fixed
 * point (loss = (double)loss_q40[0] * 2^-40): the workgroups' partial sums meet through INTEGER atomics, which commute, so
 * the value is bit-identical from run to run (a float atomic sums in arrival order).  [1] counts partials that were not
 * finite or >= 2^22: non-zero means the loss is not representable (report NaN). */
int mdm_loss_fwd_bwd(int dtype, const void* pred, const float* x_in, const float* s, const float* x0,
                     const float* w, int N, int C, int H, int W, int Cp, float gscale,
                     void* dpred, int64_t* loss_q40, void* stream);

/* mdm_loss_fwd_bwd plus the sums behind the four per-step means the reference logs next to the loss
 * (trainer_masked_mean_shift.py:176-179; trainer_masked.py:161-162 are two of them):
 *   mon_q40[0] += mean((x_in + pred) - s)   inverse_reconstruct_train_mean  (x_in + pred when s is NULL)
 *   mon_q40[1] += mean(x_in + pred)         reconstruct_train_mean
 *   mon_q40[2] += mean(x_in)                shifted_degrade_img_mean
 *   mon_q40[3] += mean(x_t)                 degraded_train_mean            (x_t: the degraded image, NCHW fp32)
 * each in fp32 registers in the reference's order, summed thread -> wave -> workgroup like the loss and added as
 * (partial / numel) in the same Q23.40 fixed point through integer atomics: bit-identical from run to run.
 * mon_q40[4] counts partials that were not finite or >= 2^22; mon_q40[5] is reserved and stays 0.  mon_q40 is SIX int64
 * words, zero before the step (mdm_monitor_commit leaves them so).  dpred and loss_q40 come out bit-identical to
 * mdm_loss_fwd_bwd on the same arguments. */
int mdm_loss_fwd_bwd_mon(int dtype, const void* pred, const float* x_in, const float* s, const float* x0,
                         const float* w, int N, int C, int H, int W, int Cp, float gscale,
                         void* dpred, int64_t* loss_q40, const float* x_t, int64_t* mon_q40, void* stream);
/* Last launch of a monitored step: writes row (ctr[0] mod cap) of ring[cap][8] --
 *   loss, the four means above in that order, sqrt(*gnorm_sq), mon_q40[4] (the flag count), 0
 * -- then ++ctr[0] and mon_q40[0..5] = 0.  This is what trainer_masked_mean_shift.py:175-179 computes with five
 * `.mean()` calls and :193 / :321-334 read with a host sync per value; here the host reads rows when it wants them.
 * The loss is (double)loss_q40[0] * 2^-40 rounded to fp32, NaN when loss_q40[1] != 0 (loss_q40 is only read).  gnorm_sq: the
 * squared gradient norm the optimizer kernel clipped with, or NULL (a micro-step without an update): the column is NaN.
 * The row index lives in device memory, so a captured step replays with no host work (as mdm_sampler_step_params).
 * ctr[0] counts modulo 2^32. */
int mdm_monitor_commit(const int64_t* loss_q40, int64_t* mon_q40, const float* gnorm_sq, int32_t* ctr, float* ring,
                       int cap, void* stream);

/* Reverse-step pieces (sampler.py:146-152, 199-216):
 *   x0_hat = (x_in + pred) - s                                              (mdm_sampler_x0)
 *   x_t   <- x_t + (d_next - d_t)  [momentum]  |  x_t <- d_next  [base]     (mdm_sampler_update) */
int mdm_sampler_x0(int dtype, const void* pred_nhwc, int Cp, const float* x_in, const float* s,
                   int N, int C, int H, int W, float* pred_nchw, float* shifted0, float* x0_hat, void* stream);
/* rng = {seed, offset} (uint64 x2, device): ++offset in stream order.  Every step / graph replay starts with it (the
 * kernels key Philox by (seed, offset, stream id, element)). */
int mdm_rng_advance(uint64_t* rng, void* stream);
/* Device-side per-step parameters (so that one reverse step is one hipGraph replayed T times): with step = *step_ctr,
 * i = T-1-step, t = timesteps[i], t_next = t-1 (t when i == 0) writes time_out[n] = t, ratio_out[n] = ratio_tab[t-1]
 * (optional), amt_t[n] = amount_tab[t-1], amt_next[n] = amount_tab[t_next-1], then ++*step_ctr and ++rng[1]
 * (sampler.py:137-170; the Philox offset bump of the host path). */
int mdm_sampler_step_params(const int32_t* timesteps, int T, int32_t* step_ctr, const double* ratio_tab,
                            const double* amount_tab, int n, float* time_out, double* ratio_out, double* amt_t,
                            double* amt_next, uint64_t* rng, void* stream);
int mdm_sampler_update(const float* d_t, const float* d_next, float* x_t, float* diff, int momentum,
                       int64_t n, void* stream);

/* ------------------------------------------------------------------------- *
 * Evaluation caller (the step after the sampler; tester.py:57-223, sampler.py:487-526): the similarity matrix of
 * generated images against data images is ONE fp32 contraction (mdm_gemm, layout 0) over unit-length rows.
 *   mdm_normalize01  y = (x - min) / (max - min) per image [N][E], NaN -> 0       (utils/datautils.py:211-222); min and max
 *                    hand a NaN pixel on like torch's amin / amax: an image that holds one comes out all 0, as a constant image does
 *   mdm_unit_rows    y[r] = x[r] / max(||x[r]||, eps) over [R][D]                  (F.cosine_similarity's normalisation)
 *   mdm_col_argmax   per column of S[M][B]: largest value and the first row holding it (score.max(dim=0), tester.py:198), in
 *                    torch's order: a NaN beats every number (the first NaN row), an all -inf column gives (-inf, 0); the index is
 *                    below M always; val may be NULL
 * ------------------------------------------------------------------------- */
int mdm_normalize01(const float* x, float* y, int N, int E, void* stream);
int mdm_unit_rows(const float* x, float* y, int R, int D, float eps, void* stream);
int mdm_col_argmax(const float* S, int M, int B, float* val, int64_t* idx, void* stream);

/* ------------------------------------------------------------------------- *
 * Optimizer: global-norm clip + SGD / Adam / AdamW + EMA + bf16 weight shadow in one pass over flat fp32 buffers.  Replaces
 * accelerator.clip_grad_norm_ + torch.optim.{SGD, Adam, AdamW}.step + EMAModel.step (trainer_masked_mean_shift.py:163-172;
 * `--optim sgd | adam | adamw`, main_train_masked.py:134-141, 375).
 *   mdm_sqnorm stores sum(g^2) to *out (two-stage, fixed summation order: bit-identical on every rank).
 *   mdm_optim_update: coef = gmul min(1, max_norm / (sqrt(*sqnorm) gmul + 1e-6)) -- gmul alone when max_norm <= 0, and *sqnorm is
 *   then not read -- (gmul = 1/world for the DP mean), then per element, in torch's order of operations:
 *     kind  optimizer           buf0, buf1            update
 *     0     SGD, momentum == 0  NULL, NULL            d = coef g + wd p;  p -= lr d
 *     1     SGD with momentum   momentum buffer, NULL d as above;  buf = buf_decay buf + g_scale d;
 *                                                     p -= lr (nesterov ? d + momentum buf : buf)
 *     2     Adam                exp_avg, exp_avg_sq   d as above (COUPLED decay: it enters both moments);
 *                                                     m = beta1 m + (1 - beta1) d;  v = beta2 v + (1 - beta2) d d;
 *                                                     p -= (lr / bias_corr1) m / (sqrt(v) / sqrt(bias_corr2) + eps)
 *     3     AdamW               exp_avg, exp_avg_sq   p *= 1 - lr wd (DECOUPLED decay);  d = coef g;  then m, v and p as kind 2
 *   then ema -= (1 - ema_decay)(ema - p) and shadow = bf16(p), each where its pointer is not NULL.
 *   hp (device, 8 floats)  kinds 0, 1:  lr, momentum, buf_decay, g_scale, weight_decay, nesterov (0 | 1), unused, ema_decay --
 *                                       (buf_decay, g_scale) = (0, 1) on the optimizer's first step (torch: buf = d), (momentum,
 *                                       1 - dampening) afterwards: the block is device memory, so a captured graph follows the rule
 *                          kinds 2, 3:  lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, ema_decay
 *   every buffer 16-byte aligned; any n (kinds 0..2 take 8 elements per lane and handle the n % 8 behind them, kind 3 takes one).
 * ------------------------------------------------------------------------- */
int mdm_sqnorm(const float* g, int64_t n, float* out, void* stream);
int mdm_optim_update(int kind, float* p, const float* g, float* buf0, float* buf1, float* ema, void* shadow_bf16,
                     int64_t n, const float* hp, const float* sqnorm, float max_norm, float gmul, void* stream);
/* dst[i] = bf16(src[i]), round to nearest even, NaN stays NaN; n == 0 returns 0 without a launch (so does mdm_fill_f32) */
int mdm_cast_bf16(const float* src, void* dst, int64_t n, void* stream);
/* Transposed bf16 shadow of the conv filters for the data-gradient pass, from the bf16 shadow Pb the optimizer kernel writes:
 * for every 64x64 tile listed in `tiles` (device, int64 x5 per tile: element offset of one tap's [Cout][Cin] matrix, Cout,
 * Cin, row0, col0; Cout % 8 == Cin % 8 == 0) write PT[off + c*Cout + r] = Pb[off + r*Cin + c]. */
int mdm_transpose_shadow_bf16(const void* Pb, void* PT, const int64_t* tiles, int ntiles, void* stream);
/* The B_split shadow of fp32 filters (mdm_gemm_desc.B_split): for each of the `nseg` segments (off, len) of the device table `segs`
 * (element offsets into P / Ps; off % 4 == 0, len % 32 == 0; a segment is a run of filter rows whose length is a multiple of 32),
 * every 32-element block b of the segment becomes 128 bytes at the same offset of Ps: 16-byte chunk g (g = 0..3) = the bf16 hi halves
 * of elements {4g..4g+3, 16+4g..16+4g+3} of the block -- 32-bit word k of the chunk = (element 4g+k in the low half, element 16+4g+k in
 * the high half) --, chunk 4+g = their bf16 lo halves in the same order (hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even):
 * the arrangement the split kernels make of their input rows in LDS.  Replaces nothing upstream: it is
 * how the fp32 `F.conv2d` of unet6.py:232-235 reaches the bf16 MFMA pipe at ~fp32 accuracy. */
int mdm_split_shadow(const float* P, float* Ps, const int64_t* segs, int nseg, void* stream);
/* The B_split shadow of the data gradient: for each filter segs[i] = {element offset, taps, Cout, Cin} (device, int64 x4; Cout % 32 == 0,
 * offset % 4 == 0) of a [tap][Cout][Cin] filter in P, PsT[off + tap' Cin Cout + ci Cout + co] = P[off + (taps-1-tap') Cout Cin + co Cin + ci]
 * -- taps flipped, each tap transposed to [Cin][Cout] -- in mdm_split_shadow's hi / lo arrangement over the 32-element blocks of every
 * row of Cout.  With it the data gradient of a 3x3 stride-1 pad-1 or a 1x1 convolution is a plain FORWARD convolution of dY
 * (layout 0, transposed = 0, Ck = Cout, N = Cin, B = B_split = this view) and runs on the split forward routes of mdm_gemm.
 * Replaces nothing upstream: it is how autograd's conv2d data gradient (unet6.py:232-235 backward) reaches the bf16 MFMA pipe. */
int mdm_split_shadow_t(const float* P, float* PsT, const int64_t* segs, int nseg, void* stream);
int mdm_fill_f32(float* p, float v, int64_t n, void* stream);
/* base[off .. off + len) = v for nseg segments segs[i] = {off, len} (device, int64 pairs; len % 4 == 0, len <= 4096, off % 4 == 0):
 * the per-step zeroing of the ACCUMULATED gradient slots only (biases, GroupNorm scales: `optimizer.zero_grad()` at
 * trainer_masked_shift.py:137 -- the weight gradients overwrite their slots, mdm_wgrad_group_*) */
int mdm_fill_segments_f32(float* base, const int64_t* segs, int nseg, float v, void* stream);

/* ------------------------------------------------------------------------- *
 * hipGraph capture of a launch sequence issued on `stream` (the whole train step
 * or one reverse step is ~10^3 short kernels: replay removes the host launch cost).
 * ------------------------------------------------------------------------- */
int mdm_graph_begin(void* stream);
int mdm_graph_end(void* stream, void** graph_exec_out);
int mdm_graph_launch(void* graph_exec, void* stream);
int mdm_graph_destroy(void* graph_exec);

/* HIP events on a caller-supplied stream (bench.py times kernels on the launch stream) */
int mdm_event_create(void** ev);
int mdm_event_record(void* ev, void* stream);
int mdm_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out);   /* synchronises on ev_stop */
int mdm_event_destroy(void* ev);
int mdm_stream_sync(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_HIP_H */
