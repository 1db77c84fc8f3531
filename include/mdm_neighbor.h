/* mdm_neighbor.h -- the nearest-neighbour ABI of libmdm_hip.so: unit-length feature rows built straight from the stored data set, and
 * the column arg-max that searches them chunk by chunk.
 *
 * A sixth header of the same library.  include/mdm_hip.h stays the statement of the training / sampling ABI, include/mdm_vis.h of the
 * presentation ABI, include/mdm_data.h of the data ABI, include/mdm_interp.h of the interpolation sampler and include/mdm_ingest.h of
 * the ingest; what is declared here is bound next to them (mdm/_lib.py: NEIGHBOR_PROTOS / NEIGHBOR_EXPORTS).  Same conventions: every
 * function returns 0 or non-zero with the text in mdm_last_error (mdm_nn_plan: a count, or -1), a refused call launches nothing, the
 * stream is the last parameter, nothing here allocates or synchronises, there are no floating-point atomics: two launches give the
 * same bits.  mdm_nn_plan is host code with HOST pointers and no stream; the other two take DEVICE pointers.
 *
 * Replaces upstream's Sampler.get_nearest_neighbor (sampler.py:487-518): a DataLoader pass over the set per query, normalize01 and
 * transforms.Resize([32, 32]) of every batch, B x M cosine similarities, torch.max with the similarity against the mirrored batch, one
 * score.max(dim=0) -- and the same pass at full resolution in Tester.get_nearest_neighbor_idx (tester.py:189-206).
 */
#ifndef MDM_NEIGHBOR_H
#define MDM_NEIGHBOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The tap table of ONE axis of torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=...) from n_in to n_out
 * samples -- what transforms.Resize([32, 32]) of sampler.py:493-494, 499 runs on a tensor.  Host only: first, count and weight are HOST
 * arrays, nothing is launched.  In double, with floating-point contraction off; scale = n_in / n_out; for output i:
 *   antialias != 0:  support = max(scale, 1);  inv = 1 / support;  c = scale (i + 0.5)
 *                    lo = max(0, (int)(c - support + 0.5));  hi = min(n_in, (int)(c + support + 0.5))
 *                    w_j = max(0, 1 - |(j - c + 0.5) inv|) for j in [lo, hi), divided by their sum (a zero sum divides nothing)
 *   antialias == 0:  s = max(scale (i + 0.5) - 0.5, 0);  j0 = min((int)s, n_in - 1);  j1 = min(j0 + 1, n_in - 1)
 *                    1 - (s - j0) on j0 and s - j0 on j1: two taps, or one tap holding their sum where j0 == j1
 *   first   NULL or [n_out] int32: the first source index of output i
 *   count   NULL or [n_out] int32: its number of taps
 *   weight  NULL or [n_out][max_taps] float: the weights rounded once to float, zero behind the count taps of a row
 * Returns the largest tap count of the axis (>= 1), also with the three outputs NULL; n_in == n_out gives the identity (one tap of
 * weight 1 per output).  Refused (returns -1): n_in or n_out <= 0; some but not all of first, count, weight; max_taps below the
 * largest tap count when they are given. */
int mdm_nn_plan(int n_in, int n_out, int antialias, int32_t* first, int32_t* count, float* weight, int max_taps);

/* rows[r] = the feature row of stored image first + r, for r in [0, R).  The image is read exactly as mdm_data_gather reads it
 * (include/mdm_data.h: kind 0 float bit for bit, kind 1 uint8 through the 256-entry lut, any img_stride >= C H W, any alignment):
 *   1. normalize != 0: normalize01 over all C H W values of the image as mdm_normalize01 states it (utils/datautils.py:211-222,
 *      sampler.py:497): (x - min) / (max - min) in float; a constant image, or one holding a NaN, gives all zeros.
 *   2. flip != 0: mirrored along W (RandomHorizontalFlip of sampler.py:492, 504 when it flips).
 *   3. S > 0: resized to [C][S][S] with the two axis tables (the DEVICE copies of mdm_nn_plan(W, S, ...) and mdm_nn_plan(H, S, ...):
 *      first [S], count [S], weight [S][taps]), along W first: t[y][ox] = sum_i hweight[ox][i] v[y][hfirst[ox] + i], then
 *      out[oy][ox] = sum_j vweight[oy][j] t[vfirst[oy] + j][ox], both as float fused multiply-adds in tap order from 0
 *      (sampler.py:493-494, 499, 505).  S == 0 keeps [C][H][W] (tester.py:196-199).
 *   4. divided by max(||row||, eps) as mdm_unit_rows does: the squares summed as float, the row multiplied by the reciprocal
 *      (cosine_similarity of sampler.py:525 / tester.py:146).
 * rows is float with pitch row_ld >= D, D = C S S or C H W; elements D .. row_ld of every row are written as 0, so that the rows feed
 * mdm_gemm directly.  No image ever exists as float in global memory: the storage is read at most twice (range, then taps) and only
 * the row is written.
 * The tables are device memory the host cannot check, so the kernel clamps: a first index into [0, size - 1], a tap count into
 * [0, taps]; a tap on a column past the last one reads the last one, a tap on a row past the last one is dropped.  (A table of
 * mdm_nn_plan meets none of these clamps.)  Whatever the tables hold, nothing outside the R images is read and nothing outside the R
 * rows is written.
 * One workgroup per image; with S > 0 a tile of source rows of one channel (at most 4096 floats) is staged in LDS.
 * Refused: src or rows NULL; kind outside {0, 1}; kind 1 without lut; M, R, C, H, W <= 0; S < 0; C H W or C S S past 2^31 - 1;
 * img_stride < C H W; first < 0 or first + R > M; row_ld < D; S > 0 with a NULL table or htaps, vtaps < 1; what does not fit the
 * 64 KiB of LDS of a workgroup: S > 64 (the S S accumulators of a channel), W > 4095 (a source row and the tile), S htaps > 2048
 * (the horizontal table). */
int mdm_nn_rows(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                int64_t first, int R, int normalize, int flip, int S,
                const int32_t* hfirst, const int32_t* hcount, const float* hweight, int htaps,
                const int32_t* vfirst, const int32_t* vcount, const float* vweight, int vtaps,
                float eps, float* rows, int64_t row_ld, void* stream);

/* The column arg-max of a similarity matrix under mdm_col_argmax's rule (torch.max(dim=0), sampler.py:512 / tester.py:204: a NaN beats
 * every number, among equals the FIRST row wins), chunk by chunk and with the mirrored similarity of sampler.py:503-508:
 *   score[m][b] = S[m ld + b], or torch.max(S[m ld + b], S_aug[m ld + b]) -- a NaN on either side gives NaN -- where S_aug is given and
 *                 row_aug is NULL or row_aug[m] != 0                                  (m < M, b < B, B <= ld; row_aug is [M] uint8)
 *   carry == 0: (val[b], idx[b]) = (the largest score of column b, row0 + its first row)
 *   carry != 0: the incoming (val[b], idx[b]) competes as a row before row 0 of this chunk: it stays unless a score beats it (a tie
 *               keeps it), so a data set searched in chunks of rows in order gives what one call over all rows gives.
 * Refused: S, val or idx NULL; M, B <= 0; ld < B; row0 < 0. */
int mdm_nn_col_argmax(const float* S, const float* S_aug, const uint8_t* row_aug, int M, int B, int64_t ld, int64_t row0, int carry,
                      float* val, int64_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_NEIGHBOR_H */
