/* mdm_interp.h -- the interpolation-sampler ABI of libmdm_hip.so: what the latent-interpolation reverse loop needs and the
 * mean-shift loop's entry points cannot express.
 *
 * A fourth header of the same library.  include/mdm_hip.h stays the statement of the training / sampling ABI, include/mdm_vis.h of the
 * presentation ABI and include/mdm_data.h of the data ABI; what is declared here is bound next to them (mdm/_lib.py: INTERP_PROTOS /
 * INTERP_EXPORTS).  Same conventions: every pointer is a DEVICE pointer, every function returns 0 or non-zero with the text in
 * mdm_last_error, a refused call launches nothing and writes nothing, the stream is the last parameter, nothing here allocates or
 * synchronises.  Images are fp32 NCHW, contiguous, like the reference's tensors.
 *
 * Replaces upstream's Scheduler.get_schedule_shift_time_interpolation (scheduler.py:735-754) with perturb_shift (:757-766), the mask
 * draw of Scheduler.degrade_interpolation_sampling (:553-557) and the momentum write of Sampler._sample_interpolation
 * (sampler.py:326-333).  The masked fills themselves are mdm_degrade(mask_in = ...) of mdm_hip.h.
 */
#ifndef MDM_INTERP_H
#define MDM_INTERP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The clamped constant shift of one reverse step and the shifted input of the net.  Per sample n (ratio is fp64, one entry per sample:
 * the schedule's ratio at t - 1 gathered by the caller or by mdm_sampler_step_params):
 *     sv   = (float)((double)shift * ratio[n])
 *     s_n  = (float)clamp((double)sv, -(double)mu[n] - ratio[n], -(double)mu[n] + ratio[n])      (torch.clamp: a NaN bound or value gives NaN)
 *     s[n][c][p] = s_n,  x_in[n][c][p] = x_t[n][c][p] + s_n                                      (one fp32 rounding)
 *   s, x_in    NULL or [N][C][H][W] float
 *   x_in_nhwc  NULL or [N][H][W][Cp] of `dtype` (0 = float, 1 = bf16: x_in rounded to nearest even): the C real channels of every pixel
 *              are written, the Cp - C pad channels are left as they are.
 * With all three outputs NULL nothing is launched.  16-byte loads and stores run when H W is a multiple of 4 and x_t, s and x_in are
 * 16-byte aligned.
 * Refused: x_t, mu or ratio NULL; N, C, H, W <= 0; C > 8; dtype outside {0, 1}; x_in_nhwc with Cp < C or Cp not a multiple of 8. */
int mdm_interp_shift(const float* x_t, const float* mu, const double* ratio, float shift, int N, int C, int H, int W, float* s,
                     float* x_in, int dtype, void* x_in_nhwc, int Cp, void* stream);

/* ONE row of uniforms thresholded per sample: mask[n][c][p] = ((double)u[p] > amount[n]) ? 1 : 0 for every channel c.
 *   u_row  [HW] float: the caller's draw (a replayed host draw), or NULL: u[p] is drawn here -- lane p & 3 of the Philox4x32-10 call
 *          at index p >> 2, counter rng[1] * 8 + 6, key rng[0] & 0xFFFFFFFF, through the library's 24-bit u01.  The high word of the
 *          key (the rank of a data-parallel process) is dropped ON PURPOSE: the row belongs to the whole batch, so the shards of one
 *          batch draw the same row.  One Philox call yields the four pixels of a thread.
 * 16-byte stores (and loads of u_row) run when HW is a multiple of 4 and the pointers are 16-byte aligned; scalar ones otherwise.
 * Refused: amount or mask NULL; u_row and rng both NULL; N, C, HW <= 0; C > 8. */
int mdm_interp_row_mask(const double* amount, const float* u_row, const uint64_t* rng, int N, int C, int HW, float* mask, void* stream);

/* The momentum write of the interpolation loop, two fp32 roundings: diff[i] = x_t[i] - d_t[i]; with update != 0 then
 * x_t[i] = d_next[i] + diff[i] (in place), with update == 0 x_t is not written (upstream's 'base_sampling' matches no branch there).
 * Refused: d_t, x_t or diff NULL; update != 0 with d_next NULL; n <= 0. */
int mdm_interp_update(const float* d_t, const float* d_next, float* x_t, float* diff, int update, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_INTERP_H */
