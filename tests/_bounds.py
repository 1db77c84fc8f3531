"""Error bounds for the contraction kernels (csrc/gemm.hip) against an fp64 reference of the same operation.

The reference is computed in fp64 from the exact stored operand values (bf16 upcasts exactly), epilogue included: alpha,
bias, rowvec (row pitch rv_ld, image = row // rows_per_img), resid and, where the destination accumulates, its prior value.
`mag` is the same computation on absolute values.  Per element, a correct kernel satisfies

    |y - ref| <= u_out |ref| + (1 + u_out) gamma mag,    gamma = (K_terms + 8) 2^-23  (+ 2^-15 on split-product routes)

u_out = 2^-8 for a bf16 store, 2^-24 for fp32: fp32 accumulation in any order (split-K, atomics, faithfully rounded adds),
then one rounding of the store.  The split-product routes multiply hi / lo bf16 pairs, ~2^-16 relative per product
(include/mdm_hip.h, B_split).  The bound does not depend on the data, so it never fails on a correct kernel; a missing tap,
K-chunk, row, image or epilogue term moves an element by about mag / K_terms or more and fails it.

Every output and input lives inside guard bands of a fixed NaN bit pattern (`Buf`): a write past either end changes the
bands, a read past either end that reaches a result turns it into NaN.

Attention (csrc/attn.hip) and the row softmax (csrc/norm.hip)
--------------------------------------------------------------
o = softmax(q k^T scale) v over L keys, head width C.  All references are fp64 functions of exactly the stored inputs.  With

    g  = (C + 8) 2^-23       fp32 accumulation of the C products of one score (or of dO . v, dO . o), any order
    gL = (L + 8) 2^-23       fp32 accumulation over the L keys (or queries) of a second product
    u  = 2^-8 | 2^-24        one rounding of a bf16 | fp32 store
    eps = 2^-20              the fast exponential: v_exp_f32 is good to 2^-23 relative, its argument x log2(e) and the result's
                             use carry two more roundings; 8x head room.  The rounding of the argument itself, 2^-24 |s - m|, is
                             below g smag because |s| <= smag and g >= 40 * 2^-23
    smag_ij = scale sum_d |q_id| |k_jd|

forward.  The computed score is s_ij + d_ij with |d_ij| <= g smag_ij, so exp(.) of it is off by that much RELATIVELY, in the
numerator term j and -- at most max_j of it -- in the denominator: 2 (g max_j smag_ij + eps).  The bf16 kernels round the
unnormalised p_ij once to bf16 before the second product (2^-8 relative per term: bf16 keeps 8 significant bits, so round to
nearest is off by up to 2^-8 of the value -- 2^-9 is only the mean, and an output element that one probability near 1 dominates,
as the peaked draws make them, attains the worst case: with 2^-9 the CPU emulation of a correct kernel left the dv bound); the sums over keys add gL (numerator: L
roundings of half an ulp; denominator: 16 per lane, two shuffles and one add per 64-key tile; each rescale of a tile step
multiplies numerator and denominator by the same alpha).  Hence, per query row i,

    eta_i = [2^-8] + 2 (g max_j smag_ij + eps) + gL,        |o - P v| <= u |P v| + (1 + u) eta_i (P |v|)
    |lse - logsumexp(s)| <= g max_j smag_ij + eps + gL + 2^-23 |lse|

([..]: kernels that round P to bf16 only.)  attn_mh_kernel rescales at every KEY, not every tile: numerator and denominator each
take two roundings per key (2 gL in all for o), and every rise of the running max multiplies what was summed so far by a fresh
fast exponential, so eps counts once per rise of the row's running max in key order (`rises_i`, from the fp64 scores, + 1).
The probabilities attn_f32_small leaves behind: |S_ij - P_ij| <= u P_ij + (1 + u) (g (smag_ij + max_j smag_ij) + 2 eps + gL) P_ij.

backward, as a function of its five inputs (qkv, o, dO, lse, scale) -- the o and lse handed to the kernel are the quantities
of the reference, whatever produced them: P = exp(s - lse), delta = sum_d dO o, dP = dO v^T, dS = P (dP - delta) scale, and
mdS = P (|dO| |v|^T + sum_d |dO| |o|) scale.

    ep_ij = g smag_ij + eps + 2^-23 |lse_i|                         relative error of the recomputed P_ij
    eS_ij = ([2^-8] + ep_ij + g + 2^-22) mdS_ij                     dS: its bf16 rounding, P, the two C-term sums, three roundings
    eP_ij = ([2^-8] + ep_ij) P_ij
    dq: (1 + gL) eS |k| + gL mdS |k|      dk: the same with eS^T, mdS^T, |q|      dv: (1 + gL) eP^T |dO| + gL P^T |dO|
    each wrapped as u |ref| + (1 + u) (...);          |delta - sum dO o| <= g sum |dO| |o|

row softmax in place: |y - P| <= u P + (1 + u) (2^-23 |x_ij - max_i| + 2 eps + gL) P (no score error: the inputs are exact; the
argument's rounding is kept because a single probability, unlike a weighted sum of them, has nothing to hide it in); backward
ref = P (g - sum P g), mag = P (|g| + sum P |g|), eta = gL + 2^-22.

A CPU emulation of the fused kernels' arithmetic (fp32 scores, 64-key online softmax, P and dS rounded to bf16, fp32 second
product, bf16 store; tests/test_bounds_cpu.py) stays inside these bounds, and each planted fault there leaves them.  The bounds
are derived, never fitted to what a GPU returned.

rel-L2 bar of the bf16 outputs: `attn_emulate_bf16` is the storage precision alone -- fp64 arithmetic with exactly the bf16
roundings above.  A kernel's rel-L2 against fp64 may be at most REL_L2_MARGIN = 1.5 times the emulation's on the same inputs:
the emulation does not depend on the tile order, while truncating P or the output instead of rounding lands at 1.7 - 2.0 times.

GroupNorm (csrc/gn_kernels.inc, the fused epilogues of csrc/gemm.hip)
----------------------------------------------------------------------
x [N][P][C], G groups of cpg = C / G channels, n = cpg P elements per (image, group).  References are fp64 functions of exactly the
stored inputs (bf16 upcasts exactly; eps is the fp32 value the descriptor carries).  u = 2^-8 | 2^-24 as above.

forward, scheme "pivot" (the standalone kernels): K = the group's first element; the sums of d = x - K and d^2 are taken in fp32 in
any order.  With g = (n + 8) 2^-23 (any-order fp32 summation of n terms: (n - 1) 2^-24 to first order, twice that taken), D1 =
mean |d|, D2 = mean d^2, md = mean d:

    e_md   = g D1                                                      the computed mean of d
    e_mean = e_md + 2^-23 |mean|                                       K + md rounded, the product with 1 / n rounded
    e_var  = (g + 2^-22) D2 + 2 |md| e_md + e_md^2 + 2^-23 (D2 + md^2)  d rounded (2^-23 on its square) and the square's fma; md^2
                                                                       from the computed md; the products, the difference
    w = var + eps,  e_var < w / 2 asserted (the rows are chosen so that it holds)
    e_r    = e_var / (2 (w - e_var)) + EPS_RSQ                         RELATIVE error of rstd = rsqrtf(w)

EPS_RSQ = 4 x 2^-23: four times the accuracy of rsqrtf.  What a ROCm installation itself states is only the mapping: its HIP header
lib/llvm/lib/clang/<version>/include/__clang_hip_math.h defines rsqrtf(x) as __ocml_rsqrt_f32(x); no header or document it ships
gives the accuracy.  The figure, 1 ULP, is quoted from AMD's PUBLIC documentation -- the OCML document of the ROCm device libraries
("rsqrt", float) and the math API table of the HIP documentation -- and one ulp of an fp32 value is at most 2^-23 of it.  Derived
from that figure, not fitted.  A constant group has D1 = D2 = md = 0, hence e_var = 0: its mean must be K (the tests ask for K's bits)
and its rstd rsqrtf(eps); the tests hold the latter to the bits of fp32(1 / sqrt(eps)) or of a neighbour, which is what 1 ULP
allows.

    z = (x - mean) rstd gamma_c + beta_c
    |dz| <= |rstd gamma_c| e_mean + |x - mean| |rstd gamma_c| (e_r + 2^-22) + 2^-24 |z|
            (x - mean^ rounded, rstd gamma rounded, their product inside or in front of an fma: 1.5 x 2^-23 < 2^-22; the fma's own
             rounding is the last term)
    silu(z) = z rcp(1 + __expf(-z)):  |dsilu| <= 1.1 |dz| + (EPS_EXP + 2^-23 |z| + 2^-22) |silu(z)|     (1.1 >= sup |silu'|; the
            exponential's argument rounding is 2^-24 |z| absolute = relative on exp, the add, the reciprocal, the product)
    store:  u |ref| + (1 + u) (the above)
    dropout: ref keep scale with one more 2^-24 |ref| for the product; a dropped element has ref = bound = 0: exactly zero.

scheme "two_pass" (the fused forward epilogues: the mean of the bf16-rounded y, then centred squares): A1 = mean |y|,

    e_mean = g A1 + 2^-23 |mean|                        nothing is subtracted before the first sum: it scales with |y|, not D1
    mean (y - mean^)^2 = var + (mean - mean^)^2 <= V = var + e_mean^2       exactly
    e_var  = e_mean^2 + (g + 2^-22 + 2^-23) V + 2^-24 w  the centred value rounded (2^-23 on its square), the square, the sum, the
                                                        product with 1 / n; the sum with eps

and everything after w as above.

backward, as a function of (x, dy, mean, rstd, gamma, beta): the statistics handed to the kernel are fp32-rounded fp64 values --
inputs of the reference, so no backward bound depends on a forward kernel.  With r = rstd, xh = (x - mean) r, z = xh gamma + beta,
sigma = 1 / (1 + exp(-z)):

    e_xh = 2^-23 (|x| + |mean|) r                      both (x - mean) r and fma(x, r, -mean r)
    e_z  = 2^-22 ((|x| + |mean|) r |gamma| + |beta|)
    e_sg = EPS_EXP + 2^-23 |z| + 2^-22                 relative error of sigma
    silu'(z) = sigma (1 + z (1 - sigma)):  |dsilu'| <= (e_sg + 2^-22) (1 + 2 |z|) sigma + 0.5 e_z      ABSOLUTE: silu' crosses zero;
                                                       0.5 >= sup |silu''|
    gz = dy silu'(z),  e_gz = |dy| e_silu' + 2^-24 |gz|  (+ dy_err |silu'| where dy itself was computed; + 2^-24 |gz| with dropout,
                                                       where dy is dy keep scale)
    dbeta  = sum_{n,p} gz:      gNP sum |gz| + sum e_gz,                           gNP = (N P + 8) 2^-23
    dgamma = sum_{n,p} gz xh:   gNP sum |gz xh| + sum (e_gz |xh| + |gz| e_xh)
    A1 = sum_group gz gamma, A2 = sum_group gz gamma xh:   (n + cpg + 8) 2^-23 on their |.| sums (gn_bwd_reg_kernel forms them as
                                                       gamma-weighted sums over the group's channels of the column sums), plus the
                                                       propagated e_gz, e_xh
    dx  = r (gamma gz - (A1 + xh A2) / n),   mag = the same on absolute values
    e_dx = r (|gamma| e_gz + (e_A1 + |xh| e_A2 + e_xh |A2|) / n) + 2^-21 mag + 2^-22 (|x| + |mean|) r^2 |A2| / n
                                                       (the last term: k1 = fma(q2, -mean r, q1) of gn_bwd_reg_kernel, whose two
                                                       parts cancel against x k2)
    stored = dx + adds:  + 2^-23 (|dx| + sum |add|), wrapped with u
    sum_img[n][c] = sum_p dx (in front of the adds and of the store's rounding):  (P + 8) 2^-23 sum_p mag + sum_p e_dx
    sum_all, dgamma, dbeta accumulate onto a prior value: + (N + 8) 2^-23 (|prior| + the |.| sum) for the N additions.
A group's dx sums to zero, so the column sums are held against magnitudes, never relatively.

A CPU emulation of each kernel's arithmetic in fp32 (tests/test_bounds_cpu.py: pivot sums in two orders, the two-pass forward, both
backward forms, the adds, one store rounding) stays inside these bounds on every row the GPU tests use, and each planted fault
leaves them.  rel-L2 bar of the bf16 y and dx: REL_L2_MARGIN times the rel-L2 of rne_bf16(ref), as for attention.

The time-embedding path (csrc/temb.hip) and the helper kernels at the end of csrc/norm.hip
-------------------------------------------------------------------------------------------
All fp32; every reference is an fp64 function of exactly the stored inputs.

skinny forward, y = x W^T + b:  `check` with k_terms = K + 1, store "f32", mag = |x| |W|^T + |b| (four wave partials, their sum in
LDS order, the bias: fp32 additions in some order).  act_out is held against silu of the y THE KERNEL STORED (the register value it
applied silu to), not of the reference:

    |act - silu(y)| <= u |silu(y)| + (1 + u) (EPS_EXP + 2^-23 |y| + 2^-22) |silu(y)|         (the silu term above, u = 2^-24)

so an act_out taken from another element or from the sum before the bias is off by the full difference, not by the error of y.

embedding (emb_out of the skinny kernel, temb_kernel):  e[n][j | half + j] = sin | cos (a), a = t_n exp(-j c), c = ln(1e4) / (half -
shift), in fp32 as  a^ = t * expf(-(float)j * (logf(10000.f) / ((float)half - shift))).  logf, expf, sinf and cosf are
__ocml_{log,exp,sin,cos}_f32 (__clang_hip_math.h), which AMD's public tables -- the OCML document of the ROCm device libraries
and the math API table of the HIP documentation, the sources EPS_RSQ quotes -- give as 1 ULP (logf, expf) and 2 ULP at most (sinf,
cosf over the full range).  EPS_LIBM = 4 x 2^-23 takes four times one ulp (<= 2^-23 relative) for logf and expf; E_TRIG = 4 x 2 x
2^-24 = 2^-21 ABSOLUTE takes four times two ulps of a value below 1 (2^-24 each; of the value 1 itself: four ulps).  (float)half - shift is
exact.  c^ = c (1 + d), |d| <= EPS_LIBM + 2^-24 (logf, the division); the exponent -(float)j c^ takes one more 2^-24, and |j c| <=
ln(1e4) because j <= half - shift: its ABSOLUTE error is at most ln(1e4) (EPS_LIBM + 2^-23), which is relative on the exponential;
expf adds EPS_LIBM, the product with t 2^-24:

    e_a = exp(ln(1e4) (EPS_LIBM + 2^-23)) (1 + EPS_LIBM) (1 + 2^-24) - 1            (6.0e-6: 51 x 2^-23)
    |e - ref| <= |a| e_a + E_TRIG                                                   sin, cos are 1-Lipschitz

At j = 0 the exponent is -0.0, expf gives exactly 1 and a^ = t exactly: that column is held to E_TRIG alone, at t up to 1000.  The
pad column of an odd dim (temb_kernel) is exactly +0.

TEMB layer (x == NULL): y is held against the emb_out the kernel stored -- the register tile it multiplied -- so the contraction
bound is the plain one.  Without emb_out the reference is the fp64 embedding and the bound grows by (embedding bound) |W|^T.

skinny backward, dx = dy W.  Slab s of a split launch is held against the fp64 partial sum over k in [s K / splits, (s + 1) K /
splits) with k_terms = K / splits.  silu'(p) = sigma (1 + p (1 - sigma)) as in the GroupNorm section with an exact argument:

    e_silu' = (EPS_EXP + 2^-23 |p| + 2^-22 + 2^-22) (1 + 2 |p|) sigma                ABSOLUTE
    unsplit with pre:   |silu'| (u |acc| + (1 + u) gamma mag) + mag e_silu',   gamma = (K + 8) 2^-23
    silu_bwd_sum of the slabs HANDED to it:  ref = (sum_s slab_s) silu'(pre),
        u |ref| + (1 + u) ((nslab + 8) 2^-23 sum |slab| |silu'| + sum |slab| e_silu');     pre == NULL: silu' = 1, e_silu' = 0

silu_fwd: the silu term, wrapped with u.  silu_bwd: dx = dy silu'(x): u |ref| + (1 + u) |dy| e_silu' (e_silu' carries 2^-22 for the
two products); acc = 1 adds 2^-24 (|prior| + |g|) for the addition.

colsum of dY [N][P][C] (bf16 upcasts exactly):  per_img[n][c] = sum_p: (P + 8) 2^-23 sum_p |dY| (32 pixel-lane partials, then their
32-term sum), + 2^-24 (|prior| + sum_p |dY|) when acc_img = 1.  dbias[c] = prior + sum_{n,p}: (N P + 8) 2^-23 (|prior| + sum |dY|).
fp32: one writer per channel and a fixed order, two runs give the same bits.  bf16: the images meet through float atomics -- bound
only.

add, add3, sumpool2 with acc = 1, the layout converters: bit exact.  add3(x, y) has the bits of (x.float() + y.float()).to(storage),
add3(x, NULL) and the converters move bits unchanged, pad channels C .. Cp - 1 are +0, sumpool2 with acc = 1 is ((a + b) + c) + d in
fp32, + prior, one rounding (as test_avgpool2's accumulate case).

A CPU emulation in fp32 (tests/_temb_rows.py: four wave partials over k summed w0 + w1 + w2 + w3, slabs summed in order, silu and
silu' in fp32, the embedding in fp32 numpy, colsum as 32 pixel-lane partials and their 32-term sum) stays inside these bounds on
every row, and each planted fault leaves them (tests/test_bounds_cpu.py).

The store kernels (csrc/optim.hip apart from optim_update_kernel), the loss and sampler kernels (the value side of csrc/sched.hip)
and the evaluation kernels (csrc/eval.hip)
-----------------------------------------------------------------------------------------------------------------------------------
All fp32 arithmetic; u = 2^-24.  The library is built without any fast-math flag (csrc/Makefile: -O3 and nothing that relaxes
floating point), so +, -, * are IEEE, sqrtf and / are correctly rounded, and the compiler contracts a product into an fma only where
one expression holds a product AND a sum of it.  Three kernels sum; everything else is held BIT FOR BIT.

mdm_sqnorm, ref = sum g^2 in fp64.  Every term is non-negative, so each rounding on the way from a term to the result is at most u of
a partial sum that is itself at most ref: the error is (depth) u ref, whatever n is.  The depth, from sqnorm_kernel /
sqnorm_final_kernel and the launcher (n4 = n / 4 float4, nb = min(1024, max(1, ceil(n4 / 256))) workgroups of 256):

    T = ceil(n4 / (256 nb)) float4 per thread: 4 T chained fmaf (one rounding each, the square is not rounded)
    <= 3 tail elements on thread 0 of workgroup 0, 6 shuffle adds, 2 adds over the four wave partials              (11)
    second stage: ceil(nb / 256) <= 4 chained adds per lane, 6 shuffle adds, 2 adds                                (12)

    |y - ref| <= (4 T + 32) 2^-24 ref              (depth 4 T + 23 as found; the other 9 u cover every second-order term)

A row that is zero but for one 3.0 must give exactly 9.0: 9 + 0 is exact at every node.  That is the row that shows a MISSING
element; among a million random terms one float4 is at the edge of the bound.

mdm_loss_fwd_bwd.  r = ((x_in + pred) - s) - x0 is two or three IEEE additions of stored values (pred upcasts exactly), no product
next to them: the same expression in numpy fp32 has the kernel's bits (`loss_residual32`).  dpred = 2.f * wn * r * inv_numel *
gscale, left to right, inv_numel = 1.f / ((float)N * (float)C * (float)HW): products and one correctly rounded division, no sum, so
nothing can contract -- bit for bit the numpy fp32 expression, rounded once (RNE) to a bf16 destination; the pad channels C .. Cp - 1
are +0.  The loss word: ref = fp64 mean of w_n r32^2.  A term passes wn * r (1 rounding), the thread's chain of fmaf over its C T
terms (T = ceil(N HW / (256 grid)) pixels per thread, grid = min(256, ceil(N HW / 256)) workgroups), 6 shuffle adds and 2 adds, the
product with inv_numel (1) and inv_numel's own three roundings: C T + 13, all terms non-negative.  Each workgroup then rounds its
partial once to Q23.40, half a unit = 2^-41, and the integer adds are exact:

    |loss - ref| <= (C T + 16) 2^-24 ref + grid 2^-41;      the flag word is 0

mdm_unit_rows, ref = x / max(||x||, eps) in fp64 with eps the fp32 value the call carries.  The sum of squares S has depth d =
ceil(D / 256) + 8 (the lane's fmaf chain, 6 shuffle adds, 2 adds), non-negative terms: relative d u.  sqrtf halves that and rounds
once (d / 2 + 1) u; max(., eps) is 1-Lipschitz (and exact), so the figure holds on either side of eps and across it; inv = 1.f / max
is correctly rounded (+ u); y = x * inv (+ u):

    |y - ref| <= (d / 2 + 4) 2^-24 |ref|           (d / 2 + 3 to first order; the fourth u covers the second-order terms, d <= 200)

A zero row is exactly +0 (0 * (1 / eps)); a row with ||x|| < eps is x / eps under the same bound.

Bit for bit, and why:
    mdm_normalize01     (x - lo) / (hi - lo), then NaN -> 0: one subtraction, one correctly rounded division, and min / max, which do
                        not round: torch fp32 nan_to_num((x - amin) / (amax - amin), nan=0) on the CPU.  A NaN pixel makes amin and
                        amax NaN and the whole image 0; a constant image is 0 / 0 -> 0.
    mdm_col_argmax      comparisons only: torch.max(dim=0), values and indices: the first row among equals, a NaN beats every number
                        (the first NaN row), an all -inf column gives (-inf, 0); the index is below M always.
    mdm_sampler_x0      sh0 = x_in + pred, x0_hat = sh0 - s: one addition each; pred_nchw moves bits.  Pad channels of pred are
                        never read.
    mdm_sampler_update  diff = d_next - d_t; x_t + diff (two additions, no product) or the bits of d_next.
    mdm_cast_bf16       v_cvt_pk_bf16_f32, round to nearest even, NaN stays NaN: torch's .to(bfloat16).
    mdm_transpose_shadow_bf16, mdm_split_shadow, mdm_split_shadow_t
                        move bits / round to bf16 twice (hi = bf16(x), lo = bf16(x - hi): x - hi is exact in fp32): the layouts the
                        kernel comments give, restated below (`transpose_want`, `split_want`, `split_t_want`).
    the two fills       the fill value's bits (-0.0 stays -0.0).

A CPU emulation in numpy fp32 (tests/_store_rows.py: the sqnorm tree with per-thread chains, waves and both stages in the kernel's
order, the loss tree, unit_rows; fmaf(a, a, c) as the fp64 a a + c rounded to fp32) stays inside these bounds on every row, and each
planted fault is rejected by at least one row (tests/test_store_rows_cpu.py).
"""
import torch
import torch.nn.functional as F

U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
SPLIT_PRODUCT = 2.0 ** -15
EPS_EXP = 2.0 ** -20          # fast exponential (module docstring)
REL_L2_MARGIN = 1.5           # kernel rel-L2 <= this x the rel-L2 of the storage-precision emulation
EPS_RSQ = 4 * 2.0 ** -23       # rsqrtf: 4 x its documented 1 ULP (module docstring)
# guard pattern: a quiet NaN with a payload no kernel produces
_PAT = {torch.float32: (torch.int32, 0x7FC0A5A5), torch.bfloat16: (torch.int16, 0x7FE5)}


class Buf:
    """A tensor `.t` of `shape` inside [guard | data | guard] of one allocation.  Guards hold the NaN pattern and are at least
    `min_guard_rows` rows of `row` elements and at least 64 KiB.  fill: "nan" (the pattern), or a tensor of values."""

    def __init__(self, shape, dtype, device, fill="nan", row=None, min_guard_rows=256):
        self.shape, self.dtype = tuple(shape), dtype
        n = 1
        for s in self.shape:
            n *= s
        row = row if row is not None else (self.shape[-1] if len(self.shape) > 1 else 1)
        esz = torch.finfo(dtype).bits // 8
        self.g = max(min_guard_rows * row, 65536 // esz)
        self.n = n
        self.raw = torch.empty(2 * self.g + n, dtype=dtype, device=device)
        ity, pat = _PAT[dtype]
        self.ity, self.pat = ity, pat
        self.raw.view(ity).fill_(pat)
        self.t = self.raw[self.g:self.g + n].view(self.shape)
        if not isinstance(fill, str):
            self.t.copy_(fill.to(dtype).reshape(self.shape))

    def guards_intact(self):
        iv = self.raw.view(self.ity)
        return bool((iv[:self.g] == self.pat).all()) and bool((iv[self.g + self.n:] == self.pat).all())

    def first_bad_guard(self):
        iv = self.raw.view(self.ity).cpu()
        lo = (iv[:self.g] != self.pat).nonzero()
        hi = (iv[self.g + self.n:] != self.pat).nonzero()
        return (int(lo[-1]) - self.g if len(lo) else None, int(hi[0]) + self.n if len(hi) else None)


def rne_bf16(x64):
    """fp64 -> bf16 with round-to-nearest-even through fp32 (fp32 first is exact enough: the fp32 rounding is far below a bf16 ulp
    except at exact ties, which random data does not hit)."""
    return x64.float().to(torch.bfloat16)


def trunc_bf16(x64):
    """fp64 -> bf16 by dropping the low 16 bits of the fp32 value (round toward zero): a planted fault."""
    i = x64.float().view(torch.int32) & ~0xFFFF
    return i.view(torch.float32).to(torch.bfloat16)


def _finite64(name, y):
    y64 = y.detach().cpu().double()
    if not bool(torch.isfinite(y64).all()):
        bad = (~torch.isfinite(y64)).nonzero()[:4].tolist()
        raise AssertionError(f"{name}: non-finite output at {bad} ({int((~torch.isfinite(y64)).sum())} elements)")
    return y64


def violations(y, ref, bound):
    """Boolean mask of the elements of `y` outside |y - ref| <= bound (non-finite elements count as outside)."""
    y64 = y.detach().cpu().double()
    return ~((y64 - ref.double()).abs() <= bound.double())


def check_bound(name, y, ref, bound, rows=None):
    """`check` with a precomputed per-element `bound` tensor (same shape as ref): NaN / Inf anywhere in y fails, then every
    element of y (or y[rows]) must satisfy |y - ref| <= bound.  Returns (largest err / bound, rel-L2)."""
    y64 = _finite64(name, y)
    if rows is not None:
        y64 = y64[rows]
    ref, bound = ref.double(), bound.double()
    assert y64.shape == ref.shape == bound.shape, (name, y64.shape, ref.shape, bound.shape)
    err = (y64 - ref).abs()
    over = err > bound
    if bool(over.any()):
        idx = over.nonzero()[:4].tolist()
        ex = [(i, float(y64[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
        raise AssertionError(f"{name}: {int(over.sum())} elements outside the bound, e.g. (index, y, ref, bound) {ex}")
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    rel = float((y64 - ref).norm() / (ref.norm() + 1e-300))
    return ratio, rel


def check(name, y, ref, mag, k_terms, store, split=False, rows=None):
    """Per-element hard bound and tensor rel-L2 of output `y` (any device, any float dtype) against the fp64 `ref` / `mag`
    (same shape as y, or as y[rows] when `rows` selects a subset of the leading dimension).  NaN / Inf anywhere in y fails.
    Returns (largest err / bound, rel-L2)."""
    ref, mag = ref.double(), mag.double()
    assert ref.shape == mag.shape, (name, ref.shape, mag.shape)
    u = U_BF16 if store == "bf16" else U_F32
    gamma = (k_terms + 8) * 2.0 ** -23 + (SPLIT_PRODUCT if split else 0.0)
    return check_bound(name, y, ref, u * ref.abs() + (1 + u) * gamma * mag, rows=rows)


# ------------------------------------------------------------------ fp64 references (CPU)
def _nchw(x):
    return x.double().cpu().permute(0, 3, 1, 2)


def _w4(wt, KH, KW):
    """w[tap][Cout][Cin] -> [Cout][Cin][KH][KW]"""
    T, Co, Ci = wt.shape
    return wt.double().cpu().reshape(KH, KW, Co, Ci).permute(2, 3, 0, 1)


def _conv(xv, w4, pads, stride):
    pt, pl, pb, pr = pads
    return F.conv2d(F.pad(xv, (pl, pr, pt, pb)), w4, stride=stride)


def conv_fwd_ref(x0, x1, wt, KH, KW, stride, pads, ups, imgs=None):
    """(acc, mag) of the convolution only, [n][OH][OW][Cout] fp64; x0/x1 NHWC (x1 may be None), imgs = subset of images."""
    xs = [x0] + ([x1] if x1 is not None else [])
    x = torch.cat([_nchw(t if imgs is None else t[imgs]) for t in xs], 1)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w4 = _w4(wt, KH, KW)
    acc = _conv(x, w4, pads, stride)
    mag = _conv(x.abs(), w4.abs(), pads, stride)
    return acc.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def conv_dgrad_ref(dy, wt, VH, VW, C, KH, KW, stride, pads, imgs=None):
    """(acc, mag) of the data gradient on the (virtual) input map [n][VH][VW][C]; dy NHWC, wt[tap][Cout][Cin]."""
    dyv = _nchw(dy if imgs is None else dy[imgs])
    w4 = _w4(wt, KH, KW)

    def vjp(g, w):
        x = torch.zeros(g.shape[0], C, VH, VW, dtype=torch.float64, requires_grad=True)
        out = _conv(x, w, pads, stride)
        return torch.autograd.grad(out, x, g)[0]
    return vjp(dyv, w4).permute(0, 2, 3, 1), vjp(dyv.abs(), w4.abs()).permute(0, 2, 3, 1)


def conv_wgrad_ref(dy, x0, x1, KH, KW, stride, pads, ups):
    """(acc, mag) of the weight gradient [tap][Cout][Cin] fp64 over all images, and the bias gradient (sum, sum|.|) [Cout]."""
    xs = [x0] + ([x1] if x1 is not None else [])
    x = torch.cat([_nchw(t) for t in xs], 1)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    dyv = _nchw(dy)
    Co, Ci = dyv.shape[1], x.shape[1]

    def vjp(g, xx):
        w = torch.zeros(Co, Ci, KH, KW, dtype=torch.float64, requires_grad=True)
        out = _conv(xx, w, pads, stride)
        return torch.autograd.grad(out, w, g)[0].permute(2, 3, 0, 1).reshape(KH * KW, Co, Ci)
    db = dyv.sum((0, 2, 3)), dyv.abs().sum((0, 2, 3))
    return vjp(dyv, x), vjp(dyv.abs(), x.abs()), db


def epilogue_ref(acc, mag, alpha=1.0, bias=None, rowvec=None, rv_ld=0, rv_off=0, rows_per_img=1, resid=None, prior=None,
                 img0=None):
    """acc / mag [M][N] fp64 -> (ref, mag) of the stored value: alpha acc + bias[n] + rowvec[rv_off + img * rv_ld + n] + resid + prior.
    img0: image index of each row block when the rows are a subset (default: row // rows_per_img)."""
    M, N = acc.shape
    ref, mg = alpha * acc, abs(alpha) * mag
    if bias is not None:
        b = bias.double().cpu()[:N]
        ref, mg = ref + b, mg + b.abs()
    if rowvec is not None:
        img = (torch.arange(M) // rows_per_img) if img0 is None else img0
        rv = rowvec.double().cpu().reshape(-1)
        idx = rv_off + img[:, None] * rv_ld + torch.arange(N)[None, :]
        r = rv[idx]
        ref, mg = ref + r, mg + r.abs()
    for extra in (resid, prior):
        if extra is not None:
            e = extra.double().cpu().reshape(M, N)
            ref, mg = ref + e, mg + e.abs()
    return ref, mg


# ------------------------------------------------------------------ attention and row softmax (module docstring)
def _u(store):
    return U_BF16 if store == "bf16" else U_F32


def _wrap(ref, m, u):
    return ref, u * ref.abs() + (1 + u) * m


def attn_fwd_ref(q, k, v, scale, store, p_bf16, per_key=False, want_P=False, chunk=1024):
    """q, k, v [B][L][D] (any float dtype: the stored values) -> dict of (ref, bound) pairs "o" [B][L][D], "lse" [B][L] and, with
    want_P, "P" [B][L][L].  store: "bf16" | "f32" of o (and P); p_bf16: the kernel rounds P to bf16 before the second product;
    per_key: it rescales at every key (attn_mh_kernel).  Queries are walked in chunks to bound the memory."""
    q, k, v = (t.detach().cpu().double() for t in (q, k, v))
    B, L, D = q.shape
    u, g, gL = _u(store), (D + 8) * 2.0 ** -23, (L + 8) * 2.0 ** -23
    o, ob, ls, lb, Ps, Pb = [], [], [], [], [], []
    for i0 in range(0, L, chunk):
        qs = q[:, i0:i0 + chunk]
        s = qs @ k.transpose(1, 2) * scale
        smag = qs.abs() @ k.abs().transpose(1, 2) * abs(scale)
        smax = smag.max(-1).values
        lse = torch.logsumexp(s, -1)
        P = torch.exp(s - lse[..., None])
        eps = torch.full_like(lse, EPS_EXP)
        if per_key:
            eps = eps * (1 + (s[..., 1:] > s.cummax(-1).values[..., :-1]).sum(-1) + 1)
        sums = (2 if per_key else 1) * gL
        eta = (U_BF16 if p_bf16 else 0.0) + 2 * (g * smax + eps) + sums
        r, b = _wrap(P @ v, eta[..., None] * (P @ v.abs()), u)
        o.append(r); ob.append(b)
        ls.append(lse); lb.append(g * smax + eps + gL + 2.0 ** -23 * lse.abs())
        if want_P:
            r, b = _wrap(P, (g * (smag + smax[..., None]) + 2 * eps[..., None] + gL) * P, u)
            Ps.append(r); Pb.append(b)
    out = {"o": (torch.cat(o, 1), torch.cat(ob, 1)), "lse": (torch.cat(ls, 1), torch.cat(lb, 1))}
    if want_P:
        out["P"] = (torch.cat(Ps, 1), torch.cat(Pb, 1))
    return out


def attn_bwd_ref(q, k, v, o, do, lse, scale, store, round_bf16, chunk=1024):
    """The backward as a function of its inputs (q, k, v, o, dO [B][L][D], lse [B][L], as stored) -> dict of (ref, bound) pairs
    "dq", "dk", "dv" [B][L][D] and "delta" [B][L].  round_bf16: the kernel rounds P and dS to bf16 before the second products."""
    q, k, v, o, do, lse = (t.detach().cpu().double() for t in (q, k, v, o, do, lse))
    B, L, D = q.shape
    u, g, gL = _u(store), (D + 8) * 2.0 ** -23, (L + 8) * 2.0 ** -23
    r9 = U_BF16 if round_bf16 else 0.0
    delta, dmag = (do * o).sum(-1), (do.abs() * o.abs()).sum(-1)
    z = lambda: torch.zeros(B, L, D, dtype=torch.float64)
    dq, dqm, dk, dkm, dv, dvm = [], [], z(), z(), z(), z()
    ka, va = k.abs(), v.abs()
    for i0 in range(0, L, chunk):
        sl = slice(i0, i0 + chunk)
        qs, gs = q[:, sl], do[:, sl]
        s = qs @ k.transpose(1, 2) * scale
        smag = qs.abs() @ ka.transpose(1, 2) * abs(scale)
        P = torch.exp(s - lse[:, sl, None])
        dS = P * (gs @ v.transpose(1, 2) - delta[:, sl, None]) * scale
        mdS = P * (gs.abs() @ va.transpose(1, 2) + dmag[:, sl, None]) * abs(scale)
        ep = g * smag + EPS_EXP + 2.0 ** -23 * lse[:, sl, None].abs()
        eS = (r9 + ep + g + 2.0 ** -22) * mdS
        eP = (r9 + ep) * P
        dq.append(dS @ k); dqm.append((1 + gL) * (eS @ ka) + gL * (mdS @ ka))
        dk += dS.transpose(1, 2) @ qs; dkm += (1 + gL) * (eS.transpose(1, 2) @ qs.abs()) + gL * (mdS.transpose(1, 2) @ qs.abs())
        dv += P.transpose(1, 2) @ gs; dvm += (1 + gL) * (eP.transpose(1, 2) @ gs.abs()) + gL * (P.transpose(1, 2) @ gs.abs())
    return {"dq": _wrap(torch.cat(dq, 1), torch.cat(dqm, 1), u), "dk": _wrap(dk, dkm, u), "dv": _wrap(dv, dvm, u),
            "delta": (delta, g * dmag)}


def attn_emulate_bf16(q, k, v, do, scale, o=None, lse=None, chunk=1024):
    """The storage precision of the fused bf16 kernels and nothing else: fp64 arithmetic with the unnormalised P rounded to bf16
    before P v, P and dS rounded to bf16 before the backward's second products, and every output rounded to bf16.  The backward
    (when `o` and `lse` are given) is the same function of (qkv, o, dO, lse) as attn_bwd_ref.  -> dict of fp64 tensors."""
    r = lambda x: rne_bf16(x).double()
    q, k, v, do = (t.detach().cpu().double() for t in (q, k, v, do))
    B, L, D = q.shape
    out = {}
    oo = []
    bwd = o is not None
    if bwd:
        o, lse = o.detach().cpu().double(), lse.detach().cpu().double()
        delta = (do * o).sum(-1)
        dq, dk, dv = [], torch.zeros_like(q), torch.zeros_like(q)
    for i0 in range(0, L, chunk):
        sl = slice(i0, i0 + chunk)
        s = q[:, sl] @ k.transpose(1, 2) * scale
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        oo.append(r((r(p) @ v) / p.sum(-1, keepdim=True)))
        if bwd:
            P = torch.exp(s - lse[:, sl, None])
            dS = r(P * (do[:, sl] @ v.transpose(1, 2) - delta[:, sl, None]) * scale)
            dq.append(r(dS @ k))
            dk += dS.transpose(1, 2) @ q[:, sl]
            dv += r(P).transpose(1, 2) @ do[:, sl]
    out["o"] = torch.cat(oo, 1)
    if bwd:
        out.update(dq=torch.cat(dq, 1), dk=r(dk), dv=r(dv))
    return out


def softmax_fwd_ref(x, store):
    """x [rows][L] as stored -> (P, bound) of the in-place row softmax."""
    x = x.detach().cpu().double()
    L = x.shape[-1]
    mx = x.max(-1, keepdim=True).values
    P = torch.softmax(x, -1)
    eta = 2.0 ** -23 * (x - mx).abs() + 2 * EPS_EXP + (L + 8) * 2.0 ** -23
    return _wrap(P, eta * P, _u(store))


def softmax_bwd_ref(P, g, store):
    """P, g [rows][L] as stored -> (ref, bound) of dS = P (g - sum_j P g) written over g."""
    P, g = P.detach().cpu().double(), g.detach().cpu().double()
    L = P.shape[-1]
    ref = P * (g - (P * g).sum(-1, keepdim=True))
    mag = P.abs() * (g.abs() + (P.abs() * g.abs()).sum(-1, keepdim=True))
    return _wrap(ref, ((L + 8) * 2.0 ** -23 + 2.0 ** -22) * mag, _u(store))


def attn_draw(N, L, C, kind, seed):
    """Inputs of the fused-attention tests, pre-rounded to bf16: qkv [N][L][3C], dO [N][L][C] ~ N(0, 1).
    "flat": q, k ~ N(0, 1), every key carries weight.  "peaked": amplitude 1.5, key L - 3 of image 0 scaled x6 and key L / 2 x4:
    the running max rises in the last and in a middle key tile while the accumulator is non-zero.  v gets +0.5 on both, so that
    a missing or doubled key moves the output."""
    g = torch.Generator().manual_seed(seed)
    amp = {"flat": 1.0, "peaked": 1.5}[kind]
    qkv = torch.randn(N, L, 3 * C, generator=g) * amp
    qkv[..., 2 * C:] += 0.5
    qkv = qkv.to(torch.bfloat16).float()
    if kind == "peaked":
        qkv[0, L - 3, C:2 * C] *= 6.0
        qkv[0, L // 2, C:2 * C] *= 4.0
    do = torch.randn(N, L, C, generator=g)
    return qkv.to(torch.bfloat16), do.to(torch.bfloat16)


def attn_fused_refs(qkv, do, scale, emulate=True):
    """Everything a test of the fused bf16 kernels compares with: the forward's (ref, bound) pairs, the o (fp64 -> bf16) and lse
    (fp64 -> fp32) the backward is GIVEN, the backward's pairs as a function of those, and the storage-precision emulation."""
    C = do.shape[-1]
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    R = attn_fwd_ref(q, k, v, scale, "bf16", p_bf16=True)
    R["o_in"], R["lse_in"] = rne_bf16(R["o"][0]), R["lse"][0].float()
    R.update(attn_bwd_ref(q, k, v, R["o_in"], do, R["lse_in"], scale, "bf16", round_bf16=True))
    if emulate:
        R["emu"] = attn_emulate_bf16(q, k, v, do, scale, R["o_in"], R["lse_in"])
    return R


# ------------------------------------------------------------------ GroupNorm (module docstring)
def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def _per_elem(t, cpg):
    """[N][G] -> [N][1][C]"""
    return t.repeat_interleave(cpg, 1)[:, None, :]


def gn_fwd_ref(x, gamma, beta, G, eps, silu, store, scheme="pivot", keep=None, scale=1.0):
    """x [N][P][C] as stored, gamma / beta [C] -> {"y": (ref, bound) [N][P][C], "stats": (ref, bound) [N][G][2]} with stats[..., 0] the
    mean and stats[..., 1] rstd, each under its own bound.  scheme: "pivot" (csrc/gn_kernels.inc) | "two_pass" (the fused forward
    epilogues).  keep (bool [N][P][C]) / scale: the host-predicted dropout mask and the fp32 scale."""
    x, gamma, beta = _f64(x), _f64(gamma), _f64(beta)
    N, P, C = x.shape
    cpg = C // G
    n = cpg * P
    eps = float(torch.tensor(eps, dtype=torch.float32))
    xg = x.reshape(N, P, G, cpg)
    g = (n + 8) * 2.0 ** -23
    if scheme == "pivot":
        K = xg[:, :1, :, :1]
        d = xg - K
        D1, D2, md = d.abs().mean((1, 3)), (d * d).mean((1, 3)), d.mean((1, 3))
        mean, var = K[:, 0, :, 0] + md, D2 - md * md
        e_md = g * D1
        e_mean = e_md + 2.0 ** -23 * mean.abs()
        e_var = (g + 2.0 ** -22) * D2 + 2 * md.abs() * e_md + e_md ** 2 + 2.0 ** -23 * (D2 + md * md)
        w = var + eps
    else:
        assert scheme == "two_pass", scheme
        mean = xg.mean((1, 3))
        var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
        e_mean = g * xg.abs().mean((1, 3)) + 2.0 ** -23 * mean.abs()
        w = var + eps
        e_var = e_mean ** 2 + (g + 2.0 ** -22 + 2.0 ** -23) * (var + e_mean ** 2) + 2.0 ** -24 * w
    assert bool((e_var < w / 2).all()), "gn_fwd_ref: the variance bound reaches var + eps on this draw: choose another row"
    rstd = w.rsqrt()
    e_r = e_var / (2 * (w - e_var)) + EPS_RSQ
    m_e, r_e, em_e, er_e = (_per_elem(t, cpg) for t in (mean, rstd, e_mean, e_r))
    a = r_e * gamma
    z = (x - m_e) * a + beta
    e = a.abs() * em_e + (x - m_e).abs() * a.abs() * (er_e + 2.0 ** -22) + 2.0 ** -24 * z.abs()
    y = z
    if silu:
        y = z * torch.sigmoid(z)
        e = 1.1 * e + (EPS_EXP + 2.0 ** -23 * z.abs() + 2.0 ** -22) * y.abs()
    if keep is not None:
        ks = torch.as_tensor(keep).reshape(N, P, C).double() * float(torch.tensor(scale, dtype=torch.float32))
        y, e = y * ks, (e + 2.0 ** -24 * y.abs()) * ks
    return {"y": _wrap(y, e, _u(store)), "stats": (torch.stack((mean, rstd), 2), torch.stack((e_mean, rstd * e_r), 2))}


def gn_bwd_ref(x, dy, mean, rstd, gamma, beta, G, silu, store, adds=(), dy_err=None, N_all=None, keep=None, scale=1.0,
               prior=None):
    """The backward as a function of its inputs: x, dy [N][P][C] as stored, mean / rstd [N][G] as HANDED to the kernel, `adds` the
    tensors [N][P][C] added to dx in front of the store, dy_err the absolute error of a dy that was itself computed, N_all the number
    of images the per-channel sums run over when x holds a subset of them, keep / scale the dropout mask of dy, prior =
    dict(dgamma=, dbeta=, sum_all=) the values accumulated onto.  -> (ref, bound) pairs "dx" (the stored value, adds included),
    "dgamma", "dbeta" [C], "sum_img" [N][C], "sum_all" [C]; "dx_only" = (dx, mag) in front of the adds."""
    x, dy, mean, rstd, gamma, beta = (_f64(t) for t in (x, dy, mean, rstd, gamma, beta))
    N, P, C = x.shape
    cpg = C // G
    n = cpg * P
    u = _u(store)
    m, r = _per_elem(mean, cpg), _per_elem(rstd, cpg)
    e_gz_extra = 0.0
    if keep is not None:
        dy = dy * torch.as_tensor(keep).reshape(N, P, C).double() * float(torch.tensor(scale, dtype=torch.float32))
        e_gz_extra = 2.0 ** -24
    xh = (x - m) * r
    e_xh = 2.0 ** -23 * (x.abs() + m.abs()) * r
    z = xh * gamma + beta
    if silu:
        sg = torch.sigmoid(z)
        gp = sg * (1 + z * (1 - sg))
        e_z = 2.0 ** -22 * ((x.abs() + m.abs()) * r * gamma.abs() + beta.abs())
        e_gp = (EPS_EXP + 2.0 ** -23 * z.abs() + 2.0 ** -22 + 2.0 ** -22) * (1 + 2 * z.abs()) * sg + 0.5 * e_z
    else:
        gp, e_gp = torch.ones_like(z), torch.zeros_like(z)
    gz = dy * gp
    e_gz = dy.abs() * e_gp + (2.0 ** -24 + e_gz_extra) * gz.abs()
    if dy_err is not None:
        e_gz = e_gz + _f64(dy_err) * gp.abs()
    prior = prior or {}
    pr = lambda k: _f64(prior[k]) if prior.get(k) is not None else torch.zeros(C, dtype=torch.float64)
    Nn = N if N_all is None else N_all
    gNP, gN = (Nn * P + 8) * 2.0 ** -23, (Nn + 8) * 2.0 ** -23
    out = {}
    for name, t, et in (("dbeta", gz, e_gz), ("dgamma", gz * xh, e_gz * xh.abs() + gz.abs() * e_xh)):
        s, sa = t.sum((0, 1)), t.abs().sum((0, 1))
        out[name] = (pr(name) + s, gNP * sa + et.sum((0, 1)) + gN * (pr(name).abs() + sa))
    gs = lambda t: _per_elem(t.reshape(N, P, G, cpg).sum((1, 3)), cpg)
    gg = gz * gamma
    A1, A2, M1, M2 = gs(gg), gs(gg * xh), gs(gg.abs()), gs((gg * xh).abs())
    gn = (n + cpg + 8) * 2.0 ** -23
    e_A1 = gn * M1 + gs(e_gz * gamma.abs())
    e_A2 = gn * M2 + gs(e_gz * (gamma * xh).abs() + gg.abs() * e_xh)
    dx = r * (gg - (A1 + xh * A2) / n)
    mag = r * (gg.abs() + (A1.abs() + xh.abs() * A2.abs()) / n)
    e_dx = (r * (gamma.abs() * e_gz + (e_A1 + xh.abs() * e_A2 + e_xh * A2.abs()) / n) + 2.0 ** -21 * mag
            + 2.0 ** -22 * (x.abs() + m.abs()) * r * r * A2.abs() / n)
    adds = [_f64(a) for a in adds]
    stored, amag = dx + sum(adds), dx.abs() + sum(a.abs() for a in adds)
    out["dx"] = _wrap(stored, e_dx + (2.0 ** -23 * amag if adds else 0.0), u)
    out["dx_only"] = (dx, mag)
    b_img = (P + 8) * 2.0 ** -23 * mag.sum(1) + e_dx.sum(1)
    out["sum_img"] = (dx.sum(1), b_img)
    out["sum_all"] = (pr("sum_all") + dx.sum((0, 1)), b_img.sum(0) + gN * (pr("sum_all").abs() + mag.sum((0, 1))))
    return out


def gn_stats_in(x, G, eps):
    """The statistics a backward test hands to the kernel: fp64 (two-pass) mean and rstd of the stored x, rounded to fp32.
    -> [N][G][2] fp32"""
    x = _f64(x)
    N, P, C = x.shape
    xg = x.reshape(N, P, G, C // G)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    return torch.stack((mean, (var + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()), 2).float()


def gn_draw(N, P, C, kind, seed, direction="fwd", G=32, dtype="bf16"):
    """Inputs of the GroupNorm tests as fp32 tensors already rounded to `dtype`: (x, dy) [N][P][C].
    "plain": x ~ 1.5 N(0, 1) + 0.3, dy ~ N(0, 1).  "spiked": pixels 1, P / 2 and P - 1 of every channel scaled by 40 -- in x for a
    forward row, in dy for a backward row: one element missing from a sum of 4096 plain terms moves it by about as much as the
    summation bound allows, a missing spike by 75 times that.  "offset": x = 1000 + 0.01 N(0, 1) (fp32 only): the forward's pivot; the
    backward's bounds are loose here and no fault-detection claim is made for it.  "constant": as plain, but group G - 1 of image
    N - 1 is the constant 0.75."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, P, C, generator=g) * 1.5 + 0.3
    dy = torch.randn(N, P, C, generator=g)
    if kind == "offset":
        assert dtype == "f32"
        x = 1000.0 + 0.01 * (x - 0.3) / 1.5
    elif kind == "spiked":
        (x if direction == "fwd" else dy)[:, [1, P // 2, P - 1]] *= 40.0
    elif kind == "constant":
        x[N - 1, :, (G - 1) * (C // G):] = 0.75
    else:
        assert kind == "plain", kind
    if dtype == "bf16":
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    return x, dy


def rel_l2_bar(ref):
    """REL_L2_MARGIN x the rel-L2 of rne_bf16(ref): the bar of a bf16 output (module docstring)."""
    ref = ref.double()
    return REL_L2_MARGIN * float((rne_bf16(ref).double() - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------ time-embedding path and helper kernels (module docstring)
LN1E4 = 9.210340371976184            # ln(1e4)
EPS_LIBM = 4 * 2.0 ** -23            # logf, expf: 4 x 1 ULP, relative
E_TRIG = 2.0 ** -21                  # sinf, cosf: 4 x 2 ULP of a value below 1, absolute
E_ARG = float(torch.tensor(LN1E4 * (EPS_LIBM + 2.0 ** -23), dtype=torch.float64).exp()) * (1 + EPS_LIBM) * (1 + 2.0 ** -24) - 1


def temb_ref(t, dim, flip, shift):
    """t [M] as stored -> (ref, bound) [M][dim] of the sinusoidal embedding: [sin | cos] (flip = 0) or [cos | sin] of
    t exp(-j ln(1e4) / (dim // 2 - shift)); the pad column of an odd dim is 0 with bound 0."""
    t = _f64(t).reshape(-1)
    half = dim // 2
    a = t[:, None] * torch.exp(-torch.arange(half, dtype=torch.float64) * (LN1E4 / (half - float(shift))))[None]
    e = a.abs() * E_ARG + E_TRIG
    e[:, 0] = E_TRIG
    s, c = torch.sin(a), torch.cos(a)
    parts, bounds = ([c, s] if flip else [s, c]), [e, e]
    if dim & 1:
        z = torch.zeros(t.shape[0], 1, dtype=torch.float64)
        parts, bounds = parts + [z], bounds + [z]
    return torch.cat(parts, 1), torch.cat(bounds, 1)


def linear_ref(x, W, bias=None):
    """(ref, mag) of x W^T + bias: x [M][K], W [N][K], bias [N] as stored"""
    x, W = _f64(x), _f64(W)
    ref, mag = x @ W.t(), x.abs() @ W.abs().t()
    if bias is not None:
        ref, mag = ref + _f64(bias), mag + _f64(bias).abs()
    return ref, mag


def silu_ref(y):
    """(silu(y), bound) of the fp32 v / (1 + expf(-v)) of the stored y"""
    y = _f64(y)
    s = y * torch.sigmoid(y)
    return _wrap(s, (EPS_EXP + 2.0 ** -23 * y.abs() + 2.0 ** -22) * s.abs(), U_F32)


def silu_grad_ref(p):
    """(silu'(p), its ABSOLUTE error bound) of the fp32 sigma (1 + p (1 - sigma)); p None: (1, 0)"""
    if p is None:
        return 1.0, 0.0
    p = _f64(p)
    sg = torch.sigmoid(p)
    return sg * (1 + p * (1 - sg)), (EPS_EXP + 2.0 ** -23 * p.abs() + 2.0 ** -22 + 2.0 ** -22) * (1 + 2 * p.abs()) * sg


def skinny_bwd_ref(dy, W, splits, pre=None):
    """dy [M][K], W [K][N] as stored -> (ref, bound) of slabs [splits][M][N] (splits > 1: the partial sums over the k ranges) or of
    dx [M][N] = dy W silu'(pre) (splits == 1)."""
    dy, W = _f64(dy), _f64(W)
    K = dy.shape[1]
    ks = K // splits
    g = (ks + 8) * 2.0 ** -23
    acc = torch.stack([dy[:, s * ks:(s + 1) * ks] @ W[s * ks:(s + 1) * ks] for s in range(splits)])
    mag = torch.stack([dy[:, s * ks:(s + 1) * ks].abs() @ W[s * ks:(s + 1) * ks].abs() for s in range(splits)])
    cb = U_F32 * acc.abs() + (1 + U_F32) * g * mag
    if splits > 1:
        assert pre is None
        return acc, cb
    gp, e_gp = silu_grad_ref(pre)
    if pre is None:
        return acc[0], cb[0]
    return acc[0] * gp, gp.abs() * cb[0] + mag[0] * e_gp


def silu_bwd_sum_ref(slabs, pre=None):
    """slabs [nslab][...] as HANDED to the kernel, pre [...] or None -> (ref, bound) of (sum_s slab_s) silu'(pre)"""
    slabs = _f64(slabs)
    nslab = slabs.shape[0]
    gp, e_gp = silu_grad_ref(None if pre is None else _f64(pre).reshape(slabs.shape[1:]))
    sa = slabs.abs().sum(0)
    gpa = gp.abs() if pre is not None else 1.0
    return _wrap(slabs.sum(0) * gp, (nslab + 8) * 2.0 ** -23 * sa * gpa + sa * e_gp, U_F32)


def silu_bwd_ref(x, dy, prior=None):
    """(ref, bound) of dx = (prior +) dy silu'(x)"""
    gp, e_gp = silu_grad_ref(x)
    dy = _f64(dy)
    g, b = _wrap(dy * gp, dy.abs() * e_gp, U_F32)
    if prior is not None:
        pr = _f64(prior)
        g, b = pr + g, b + 2.0 ** -24 * (pr.abs() + g.abs())
    return g, b


def colsum_ref(dY, prior_img=None, prior_bias=None):
    """dY [N][P][C] as stored -> {"per_img": (ref, bound) [N][C], "dbias": (ref, bound) [C]}; prior_img: the values per_img
    accumulates onto (acc_img = 1), prior_bias: what dbias held."""
    d = _f64(dY)
    N, P, C = d.shape
    s, sa = d.sum(1), d.abs().sum(1)
    r, b = s, (P + 8) * 2.0 ** -23 * sa
    if prior_img is not None:
        pi = _f64(prior_img)
        r, b = pi + s, b + 2.0 ** -24 * (pi.abs() + sa)
    pb = _f64(prior_bias) if prior_bias is not None else torch.zeros(C, dtype=torch.float64)
    return {"per_img": (r, b), "dbias": (pb + s.sum(0), (N * P + 8) * 2.0 ** -23 * (pb.abs() + sa.sum(0)))}


# ------------------------------------------------------------------ store, loss, sampler and evaluation kernels (module docstring)
def sqnorm_geom(n):
    """the launch of mdm_sqnorm restated: (n4 float4 of the body, nb workgroups, T float4 per thread at most)"""
    n4 = n // 4
    nb = min(1024, max(1, -(-n4 // 256)))
    return n4, nb, -(-n4 // (nb * 256))


def sqnorm_ref(g):
    """g [n] as stored -> (sum g^2 in fp64, bound): python floats"""
    g = _f64(g).reshape(-1)
    ref = float((g * g).sum())
    return ref, (4 * sqnorm_geom(g.numel())[2] + 32) * 2.0 ** -24 * ref


def loss_geom(N, HW):
    """(grid, T): workgroups of the loss launch and the pixels one thread walks at most"""
    npix = N * HW
    grid = min(256, max(1, -(-npix // 256)))
    return grid, -(-npix // (grid * 256))


def loss_residual32(pred, x_in, s, x0, C):
    """r = ((x_in + pred) - s) - x0 in fp32, in that order: pred NHWC [N][H][W][Cp] as stored, the rest NCHW fp32 -> [N][C][H][W] fp32.
    Additions of stored values only: the kernel's bits."""
    pv = pred.detach().cpu().float()[..., :C].permute(0, 3, 1, 2).contiguous()
    r = x_in.detach().cpu().float() + pv
    if s is not None:
        r = r - s.detach().cpu().float()
    return r - x0.detach().cpu().float()


def loss_ref(r32, w):
    """r32 [N][C][H][W] (loss_residual32), w [N] or None -> (fp64 mean of w_n r^2, bound): python floats"""
    N, C, H, W = r32.shape
    t = r32.double() ** 2
    if w is not None:
        t = t * _f64(w).reshape(N, 1, 1, 1)
    ref = float(t.mean())
    grid, T = loss_geom(N, H * W)
    return ref, (C * T + 16) * 2.0 ** -24 * ref + grid * 2.0 ** -41


def dpred_want(r32, w, Cp, gscale, dtype):
    """2.f * wn * r * inv_numel * gscale left to right in numpy fp32, pad channels +0, one rounding to `dtype` -> NHWC [N][H][W][Cp]"""
    import numpy as np
    f32 = np.float32
    N, C, H, W = r32.shape
    inv_numel = f32(1.0) / (f32(N) * f32(C) * f32(H * W))
    wn = (np.ones(N, f32) if w is None else w.detach().cpu().numpy().astype(f32)).reshape(N, 1, 1, 1)
    g = f32(2.0) * wn * r32.numpy() * inv_numel * f32(gscale)
    assert g.dtype == f32
    out = torch.zeros(N, H, W, Cp, dtype=torch.float32)
    out[..., :C] = torch.from_numpy(g).permute(0, 2, 3, 1)
    return out.to(dtype)


def unit_rows_ref(x, eps):
    """x [R][D] as stored, eps as passed -> (x / max(||x||, fp32(eps)), bound) fp64"""
    x = _f64(x)
    D = x.shape[1]
    e = float(torch.tensor(eps, dtype=torch.float32))
    ref = x / x.norm(dim=1, keepdim=True).clamp_min(e)
    d = -(-D // 256) + 8
    return ref, (d / 2 + 4) * 2.0 ** -24 * ref.abs()


def normalize01_want(x):
    """torch fp32 on the CPU: nan_to_num((x - amin) / (amax - amin), nan=0) per image, x [N][E]"""
    x = x.detach().cpu().float()
    lo, hi = x.amin(1, keepdim=True), x.amax(1, keepdim=True)
    return torch.nan_to_num((x - lo) / (hi - lo), nan=0.0)


def col_argmax_want(S):
    """torch.max(dim=0) of the stored S [M][B] -> (values, indices)"""
    m = S.detach().cpu().float().max(dim=0)
    return m.values, m.indices


def sampler_x0_want(pred, x_in, s, C):
    """-> (pred_nchw, shifted0, x0_hat) fp32 NCHW: pred NHWC [N][H][W][Cp] as stored"""
    pv = pred.detach().cpu().float()[..., :C].permute(0, 3, 1, 2).contiguous()
    sh0 = x_in.detach().cpu().float() + pv
    return pv, sh0, (sh0 - s.detach().cpu().float() if s is not None else sh0)


def sampler_update_want(d_t, d_next, x_t, momentum):
    """-> (diff, new x_t)"""
    diff = d_next - d_t
    return diff, (x_t + diff if momentum else d_next.clone())


def transpose_want(Pb, filters):
    """Pb: int16 bits [n] (CPU); filters [(off, taps, Cout, Cin)] -> {off: bits [taps][Cin][Cout]}: PT[off + tap Cout Cin + c Cout + r]
    = Pb[off + tap Cout Cin + r Cin + c]"""
    return {off: Pb[off:off + t * co * ci].view(t, co, ci).transpose(1, 2).contiguous() for off, t, co, ci in filters}


def _split_halves(x):
    """x fp32 [..., 32 k] -> int16 bits of the same shape viewed as [..., 64 k] halves: per 32-element block, 32-bit word j (j < 16) =
    (hi of element j, hi of element 16 + j), word 16 + j = the lo halves of the same pair; hi = bf16(x), lo = bf16(x - hi)"""
    b = x.reshape(*x.shape[:-1], -1, 2, 16)                     # [.., block, half, j]
    hi = b.to(torch.bfloat16)
    lo = (b - hi.float()).to(torch.bfloat16)
    pair = lambda h: h.view(torch.int16).transpose(-1, -2)      # [.., block, j, half]: element j low, element 16 + j high
    return torch.stack((pair(hi), pair(lo)), -3).reshape(*x.shape[:-1], -1)


def split_want(P, segs):
    """P fp32 [n] (CPU), segs [(off, len)] -> {off: int16 bits [2 len]} of mdm_split_shadow's arrangement"""
    return {off: _split_halves(P[off:off + ln]) for off, ln in segs}


def split_t_want(P, filters):
    """filters [(off, taps, Cout, Cin)] -> {off: int16 bits [2 taps Cin Cout]}: taps flipped, each tap transposed to [Cin][Cout], every
    row of Cout in mdm_split_shadow's arrangement"""
    out = {}
    for off, t, co, ci in filters:
        wt = P[off:off + t * co * ci].view(t, co, ci).flip(0).transpose(1, 2).contiguous()
        out[off] = _split_halves(wt).reshape(-1)
    return out
