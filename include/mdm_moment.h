/* mdm_moment.h -- the set-moment ABI of libmdm_hip.so: the first and second moments of a set of feature rows, summed in fp64 on the
 * device.  With the Frechet distance of mdm/moments.py they give a set-level distance between samples and data.  On pixel rows that
 * distance is a PIXEL-SPACE Frechet distance; it is NOT FID.  On the feature rows of an extractor the caller brings it is FID.
 *
 * A tenth header of the same library, bound next to the others (mdm/_lib.py: MOMENT_PROTOS / MOMENT_EXPORTS).  Same conventions:
 * every pointer is a DEVICE pointer unless stated, every function returns 0 or non-zero with the text in mdm_last_error, a refused
 * call launches nothing and writes nothing, the stream is the last parameter, nothing here allocates or synchronises.  No
 * floating-point atomics: two launches give the same bits.
 *
 * Upstream has no counterpart (its FID import is commented out, sampler.py:13, 41-44).
 *
 * GEOMETRY.  outer = X^T X is cut into TILES of 64 x 64 outputs; only the T (T + 1) / 2 tiles (I, J), J >= I, T = ceil(d / 64), of the
 * upper triangle are computed.  The rows are cut into SPLITS of rows_per_split rows, a multiple of 16 (four steps of the matrix
 * instruction, K = 4): few tiles (small d) are spread over enough workgroups to fill the device, many tiles need one split.  The
 * first launch runs one 256-thread workgroup per (tile, split): it stages 16 rows of the two column slices X[:, I] and X[:, J]
 * through LDS -- read from memory as whole 256-byte row segments, widened to double ON THE WAY INTO LDS -- and each of its four waves
 * holds 2 x 2 results of v_mfma_f64_16x16x4_f64, 32 x 32 outputs, in registers.  The workgroups of the diagonal tiles also add the
 * 64 column sums of their slice.  Every workgroup leaves its tile in the caller's workspace.  The second launch runs one workgroup
 * per strip of 16 rows of a tile (few tiles still fill the device): it adds the splits, then the carry, and writes outer[i][j] and,
 * through an LDS transpose, outer[j][i].  Tile t is (I, J) in the order (0, 0), (0, 1) .. (0, T - 1), (1, 1) ..: mdm_moment_tile_of.
 *
 * ARITHMETIC.  Every x is widened to double, which is exact; products and sums are fp64.  The product of two widened floats is exact
 * (48 significand bits), so the only error is that of the fp64 summation.  Within a split the rows go four at a time, in row order,
 * through the matrix instruction onto one accumulator that starts at +0; the order of the four products inside one instruction is
 * the hardware's, so this header claims the bound below and not a bit pattern.  A column sum takes the rows of its split one by one,
 * in row order, onto +0.  The splits are added in index order by the second launch, then the incoming value (carry), one rounding
 * each.  For every element, with n the rows summed so far (this call's and the carried ones), s the splits of this call (the largest
 * of the calls) and c the carried calls,
 *     |outer[i][j] - exact| <= gamma(n + s + c) sum_r |x[r][i] x[r][j]|,     |sum[j] - exact| <= gamma(n + s + c) sum_r |x[r][j]|,
 *     gamma(k) = k u / (1 - k u),  u = 2^-53.
 * Where every partial sum is representable -- integers times a power of two, far below 2^53 units -- the result is exact whatever the
 * order, the splits and the chunking.
 *
 * MASKS.  Rows past R and columns past d are left out by selects (they are never loaded and a +0 stands in their place), never by a
 * multiplication with zero: memory behind them may hold anything.  A non-finite x[r][c] reaches sum[c], row c and column c of outer
 * and nothing else.
 */
#ifndef MDM_MOMENT_H
#define MDM_MOMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The launch plan of mdm_moment_accumulate for R rows of d values.  HOST code, HOST pointers, every output may be NULL:
 *   tile            the tile edge, 64 outputs
 *   tiles           T (T + 1) / 2, T = ceil(d / tile)
 *   splits, rows_per_split    rows_per_split = ceil(R / max(1, ceil(512 / tiles))) rounded up to a multiple of 16;
 *                   splits = ceil(R / rows_per_split): split s takes the rows [s rows_per_split, min(R, (s + 1) rows_per_split))
 *   grid [2]        the workgroups of the tile launch, tiles x splits, and of the combining launch, 4 x tiles
 *   lds_bytes [2]   the LDS of a workgroup of either launch
 * Refused: R or d <= 0; d > 8192 (a 512 MB outer). */
int mdm_moment_plan(int64_t R, int d, int32_t* tile, int64_t* tiles, int32_t* splits, int64_t* rows_per_split, int64_t* grid,
                    int32_t* lds_bytes);

/* The map both launches use from a tile index to its place in the upper triangle: tile in [0, tiles) -> (I, J), J >= I, row I of the
 * triangle after row I - 1.  HOST code, HOST pointers, either output may be NULL.
 * Refused: d <= 0; d > 8192; tile outside [0, tiles). */
int mdm_moment_tile_of(int d, int64_t tile, int32_t* I, int32_t* J);

/* The bytes of workspace mdm_moment_accumulate needs for R rows of d values: splits x (tiles x 64 x 64 + 64 T) doubles, the tile and
 * the column sums of every split.  -1 where mdm_moment_plan refuses. */
int64_t mdm_moment_ws_bytes(int64_t R, int d);

/* sum[j] (+)= sum_r x[r][j],  outer[i][j] (+)= sum_r x[r][i] x[r][j]  over the R rows, as stated above.
 *   rows      R rows of d values with pitch row_ld >= d, in elements
 *   kind      0: float, read bit for bit at any alignment a float has (4 bytes) -- by 16 bytes when rows is 16-byte aligned and
 *                row_ld is a multiple of 4, one float at a time otherwise;
 *             1: uint8 through lut, 256 floats, as the device data set is stored and read -- by 4 bytes when rows is 4-byte aligned
 *                and row_ld is a multiple of 4, one byte at a time otherwise.  A uint8 set at d = C H W is read in place
 *   sum       double [d]
 *   outer     double [d][outer_ld], the full symmetric matrix: the workgroup of tile (I, J) writes outer[i][j] and outer[j][i] from one
 *             value, so the matrix is bit-symmetric.  Elements d .. outer_ld of a row are not touched
 *   carry     0: sum and outer are overwritten;  != 0: this call's totals are added to the incoming values, one rounding each (read
 *             from the upper triangle: an incoming outer is taken to be symmetric) -- a set streamed in chunks
 *   ws        ws_bytes >= mdm_moment_ws_bytes(R, d) bytes; holds nothing between calls
 * Refused: rows, sum, outer or ws NULL; kind outside {0, 1}; kind 1 without lut; float rows off a 4-byte boundary; R or d <= 0;
 * d > 8192; row_ld < d; outer_ld < d; sum, outer or ws off an 8-byte boundary; ws_bytes below mdm_moment_ws_bytes. */
int mdm_moment_accumulate(const void* rows, int kind, const float* lut, int64_t row_ld, int64_t R, int d, int carry, double* sum,
                          double* outer, int64_t outer_ld, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_MOMENT_H */
