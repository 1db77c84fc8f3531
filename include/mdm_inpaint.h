/* mdm_inpaint.h -- the inpainting-sampler ABI of libmdm_hip.so: what the reverse loop needs to complete partly given images and the
 * mean-shift loop's entry points cannot express.
 *
 * A seventh header of the same library, bound next to the others (mdm/_lib.py: INPAINT_PROTOS / INPAINT_EXPORTS).  Same conventions:
 * every pointer is a DEVICE pointer, every function returns 0 or non-zero with the text in mdm_last_error, a refused call launches
 * nothing and writes nothing, the stream is the last parameter, nothing here allocates or synchronises.  Images are fp32 NCHW,
 * contiguous.
 *
 * Upstream has no counterpart: its sampler cannot be told which pixels are given.  The method is stated here and restated for the
 * tests in tests/_inpaint_ref.py.  A pixel of channel c is GIVEN where keep[n][keep_C == 1 ? 0 : c][p] != 0 (so -0 is not given and
 * NaN is given); keep is [N][keep_C][H][W] with keep_C 1 or C.
 */
#ifndef MDM_INPAINT_H
#define MDM_INPAINT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mdm_sampler_x0 of mdm_hip.h plus the projection onto the data.  Per element i = (n, c, p), pv = pred[n][p][c] read as fp32:
 *     pred_nchw[i] = pv,  shifted0[i] = x_in[i] + pv,  x = s ? shifted0[i] - s[i] : shifted0[i]      (what mdm_sampler_x0 writes)
 *     x0_hat[i]    = given ? known[i] : x                                                            (a select: no arithmetic on known)
 *   pred_nhwc  [N][H][W][Cp] of `dtype` (0 = float, 1 = bf16)
 *   s          NULL or [N][C][H][W]
 *   pred_nchw, shifted0   NULL or [N][C][H][W]: the UNPROJECTED values
 * 16-byte loads and stores of the NCHW operands run when H W is a multiple of 4 and x_in, s, known, keep and the outputs are 16-byte
 * aligned.
 * Refused: pred_nhwc, x_in, known, keep or x0_hat NULL; N, C, H, W <= 0; C > 8; Cp < C; keep_C outside {1, C}; dtype outside {0, 1}. */
int mdm_inpaint_x0(int dtype, const void* pred_nhwc, int Cp, const float* x_in, const float* s, const float* known, const float* keep,
                   int keep_C, int N, int C, int H, int W, float* pred_nchw, float* shifted0, float* x0_hat, void* stream);

/* The start image of an inpainting run and the size of its hole, one workgroup per image.
 *     mu[n][c]      = the fp32 mean of the given values: over all channels of image n, the same value for every c (per_channel == 0),
 *                     or over channel c (per_channel != 0); fallback[n][c] where nothing of that image (that channel) is given
 *     x_start[i]    = given ? known[i] : mu[n][c]
 *     unknown[n]    = the number of pixels p with at least one channel not given
 *   fallback  [N][C] float;  x_start NULL or [N][C][HW];  mu NULL or [N][C];  unknown NULL or [N] int32
 * With all three outputs NULL nothing is launched.  The sums are fp32 in a fixed order (a thread's elements in order, the 64 lanes of
 * a wave by butterfly, the four waves as (0 + 1) + (2 + 3), channels in order): the same bits on every run.  16-byte accesses run
 * when HW is a multiple of 4 and known, keep and x_start are 16-byte aligned.
 * Refused: known, keep or fallback NULL; N, C, HW <= 0; C > 8; keep_C outside {1, C}. */
int mdm_inpaint_start(const float* known, const float* keep, int keep_C, const float* fallback, int per_channel, int N, int C, int HW,
                      float* x_start, float* mu, int32_t* unknown, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_INPAINT_H */
