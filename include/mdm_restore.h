/* mdm_restore.h -- the restoration-sampler ABI of libmdm_hip.so: super-resolution and colourisation by projecting every reverse
 * step onto a measurement of group means.
 *
 * A ninth header of the same library, bound next to the others (mdm/_lib.py: RESTORE_PROTOS / RESTORE_EXPORTS).  Same conventions:
 * every pointer is a DEVICE pointer, every function returns 0 or non-zero with the text in mdm_last_error, a refused call launches
 * nothing and writes nothing, the stream is the last parameter, nothing here allocates or synchronises.  Images are fp32 NCHW,
 * contiguous.
 *
 * Upstream has no counterpart.  The method is stated here and restated for the tests in tests/_restore_ref.py.
 *
 * GROUPS.  k in {1, 2, 4, 8} (square blocks; H and W multiples of k) and gray in {0, 1} partition the elements of an image: element
 * (n, c, y, x) lies in group (n, gray ? 0 : c, y / k, x / k), a group has |g| = k k (gray ? C : 1) elements, and the measurement y
 * is [N][gray ? 1 : C][H / k][W / k], one mean per group.  |g| == 1 (k = 1 without gray) constrains nothing and is refused.
 *
 * GROUP SUM, in fp32, the same order in every kernel, on every route, for every N, grid and pointer alignment.  A group is cut into
 * STRIPS of min(k, 4) columns (one strip for k <= 4, a left and a right one for k = 8).  A strip's sum starts at +0 and takes
 * the strip's elements by sequential adds: channels in order (gray; else the one channel), within a channel rows top to bottom,
 * within a row columns left to right.  The group's sum is the strip's sum (k <= 4) or left + right (k = 8).  The mean is
 * sum / (float)|g|, a correctly rounded division.  No atomics: two launches give the same bits.
 */
#ifndef MDM_RESTORE_H
#define MDM_RESTORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mdm_sampler_x0 of mdm_hip.h plus the orthogonal projection onto { x : the mean of every group of x is y }.  Per element
 * i = (n, c, p), pv = pred[n][p][c] read as fp32:
 *     pred_nchw[i] = pv,  shifted0[i] = x_in[i] + pv,  x = s ? shifted0[i] - s[i] : shifted0[i]      (what mdm_sampler_x0 writes)
 *     x0_hat[i]    = x + (y[g(i)] - m[g(i)]),   m[g] the mean of x over group g as stated above       (two fp32 operations)
 * A NaN in x or in y reaches exactly the elements of its own group.
 *   pred_nhwc  [N][H][W][Cp] of `dtype` (0 = float, 1 = bf16)
 *   s          NULL or [N][C][H][W]
 *   y          [N][gray ? 1 : C][H / k][W / k]
 *   pred_nchw, shifted0   NULL or [N][C][H][W]: the UNPROJECTED values
 * The 16-byte route holds a strip in registers between its sum and its stores (one lane per strip, two neighbouring lanes for
 * k = 8); it runs when x_in, s and the outputs are 16-byte aligned and
 *     k = 1:  H W is a multiple of 4, y is 16-byte aligned;       k > 1:  W is a multiple of 4 (every row starts 16-byte aligned);
 *     gray:   C <= 4.
 * Everything else takes the scalar route: one lane per group, which forms the sum and then forms x again for the stores.  Both
 * routes run 256-thread workgroups, at most 2048 of them, with a grid stride.
 * Refused: pred_nhwc, x_in, y or x0_hat NULL; N, C, H, W <= 0; C > 8; Cp < C; dtype outside {0, 1}; k outside {1, 2, 4, 8}; H or W
 * not a multiple of k; gray outside {0, 1}; |g| == 1. */
int mdm_restore_x0(int dtype, const void* pred_nhwc, int Cp, const float* x_in, const float* s, const float* y, int k, int gray, int N,
                   int C, int H, int W, float* pred_nchw, float* shifted0, float* x0_hat, void* stream);

/* The measurement of an image: y[g] = the mean of x [N][C][H][W] over group g, the sum and the division as stated above.  Routes
 * and grid as mdm_restore_x0, for any C (nothing is held): the 16-byte route runs when x is 16-byte aligned and, k = 1, H W is a
 * multiple of 4 and y is 16-byte aligned, or, k > 1, W is a multiple of 4.
 * Refused: x or y NULL; N, C, H, W <= 0; C > 8; k outside {1, 2, 4, 8}; H or W not a multiple of k; gray outside {0, 1}; |g| == 1. */
int mdm_restore_measure(const float* x, int k, int gray, int N, int C, int H, int W, float* y, void* stream);

/* What a run can start from and be read against, one workgroup per image:
 *     mu[n][c]      = the fp32 mean of y [n][c] over its blocks (per_channel != 0 and gray == 0), else the one mean over all of
 *                     y [n], the same value for every c
 *     expand[i]     = y[g(i)]: y broadcast over its groups (nearest upsampling, the grey value copied to every channel)
 *   mu NULL or [N][C];  expand NULL or [N][C][H][W]
 * With both outputs NULL nothing is launched.  The sums are fp32 in a fixed order (thread t of 256 adds elements t, t + 256, ... of
 * a channel of y in order, the 64 lanes of a wave by butterfly, the four waves as (0 + 1) + (2 + 3), channels in order; divided
 * by the number of values as a float): the same bits on every run and for every alignment.  expand is stored by 16 bytes when W is
 * a multiple of 4 and expand is 16-byte aligned.
 * Refused: y NULL; N, C, H, W <= 0; C > 8; k outside {1, 2, 4, 8}; H or W not a multiple of k; gray outside {0, 1}; |g| == 1. */
int mdm_restore_start(const float* y, int k, int gray, int per_channel, int N, int C, int H, int W, float* mu, float* expand,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_RESTORE_H */
