/* mdm_metric.h -- the image-quality ABI of libmdm_hip.so: MSE, PSNR and SSIM of images against held-out originals, over the whole
 * image and over the hole of an inpainting run, reduced on the device to eight numbers per image.
 *
 * An eighth header of the same library, bound next to the others (mdm/_lib.py: METRIC_PROTOS / METRIC_EXPORTS).  Same conventions:
 * every function returns 0 or non-zero with the text in mdm_last_error (mdm_metric_ws_bytes: a size, or -1), a refused call launches
 * nothing and writes nothing, the stream is the last parameter, nothing here allocates or synchronises, there are no floating-point
 * atomics: two launches give the same bits.  mdm_metric_plan and mdm_metric_ws_bytes are host code, callable with no device;
 * mdm_metric_plan takes HOST pointers and no stream.  Images are fp32 NCHW, contiguous, at any alignment.
 *
 * Upstream has no counterpart (it has no image-quality measure; its FID import is commented out, sampler.py:13, 41-44).  The SSIM is
 * Wang et al. 2004 with the usual defaults -- what torchmetrics' structural_similarity_index_measure and skimage's
 * structural_similarity(gaussian_weights=True, use_sample_covariance=False) state as their defaults.  PARITY UNPINNED: neither package
 * was available to compare against; the statement the tests hold this to is tests/_metric_ref.py, written from the formulas below.
 */
#ifndef MDM_METRIC_H
#define MDM_METRIC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The launch plan of mdm_metric_image for R rows of [C][H][W] and the window it applies.  Host only, nothing is launched.
 *   tile_h, tile_w   the extents of a tile of the SSIM map (one workgroup forms one tile from its (tile_h + 10) x (tile_w + 10) halo)
 *   tiles_y, tiles_x the tiles that cover the (H - 10) x (W - 10) map of one channel; a row has C tiles_y tiles_x tiles
 *   grid[2]          the workgroups of the tile launch (they walk the R C tiles_y tiles_x tiles with a grid stride) and of the
 *                    combining launch (R)
 *   lds_bytes        the LDS of a workgroup of the tile launch
 *   window[11]       exp(-(i - 5)^2 / (2 1.5^2)), i = 0 .. 10, formed and divided by their sum in double, each rounded once to float
 * Every output may be NULL.  Refused (returns -1): R, C, H, W <= 0; H < 11 or W < 11; C H W past 2^31 - 1. */
int mdm_metric_plan(int64_t R, int C, int H, int W, int32_t* tile_h, int32_t* tile_w, int32_t* tiles_y, int32_t* tiles_x, int64_t* grid,
                    int32_t* lds_bytes, float* window);

/* The bytes of workspace mdm_metric_image needs for this shape (six doubles per tile), or -1 where mdm_metric_plan refuses it. */
int64_t mdm_metric_ws_bytes(int64_t R, int C, int H, int W);

/* out[r][0 .. 8) for r in [0, R): row r of pred against truth[r % N].
 *   pred   [R][C][H][W]; R a positive multiple of N (a sampler history [T + 1][N][C][H][W] is read in place with R = (T + 1) N)
 *   truth  [N][C][H][W], never clamped
 *   keep   NULL, or [N][Ck][H][W] with Ck 1 or C.  Element (c, y, x) of row r is HOLE where keep[r % N][Ck == 1 ? 0 : c][y][x] == 0
 *          (so -0 is hole and a NaN counts as given, as mdm_inpaint_x0 reads it); with keep NULL every element is hole
 *   clamp_lo < clamp_hi: p = pred < clamp_lo ? clamp_lo : pred > clamp_hi ? clamp_hi : pred (comparisons: a NaN stays a NaN);
 *          otherwise p = pred
 *   data_range  L > 0;  C1 = (0.01 L)^2, C2 = (0.03 L)^2
 *   ws     [ws_bytes] of device memory the call may overwrite, ws_bytes >= mdm_metric_ws_bytes(R, C, H, W), 8-byte aligned
 * The SSIM map has C (H - 10) (W - 10) positions.  At (c, y, x), with W2[i][j] = window[i] window[j] over [y, y + 11) x [x, x + 11):
 *     mu_p = sum W2 p,  mu_t = sum W2 t,  var_p = sum W2 p^2 - mu_p^2,  var_t likewise,  cov = sum W2 p t - mu_p mu_t     (biased)
 *     SSIM = (2 mu_p mu_t + C1) (2 cov + C2) / ((mu_p^2 + mu_t^2 + C1) (var_p + var_t + C2))
 *   slot 0 mse        the mean over the C H W elements of (p - t)^2
 *        1 psnr       10 log10(L^2 / mse); +inf at mse == 0
 *        2 ssim       the mean of the map over all its positions
 *        3 mse_hole   the mean of (p - t)^2 over the hole elements; NaN (0 / 0) with no hole
 *        4 psnr_hole  from slot 3
 *        5 ssim_hole  the mean of the map over the positions whose CENTRE element (c, y + 5, x + 5) is hole; NaN if there is none
 *        6            the number of hole elements
 *        7            the number of hole-centred map positions
 * Arithmetic.  (p - t)^2 is two fp32 operations; every sum over elements and over map positions is taken in double in a fixed order
 * (a thread's items in order, the 64 lanes of a wave by butterfly, the four waves as (0 + 1) + (2 + 3), the tiles of a row strided
 * over 64 lanes and then by butterfly), divided in double and rounded once to float, as mdm_data_means does.  The windowed moments
 * are fp32 and separable: along W first, then along H, each a chain of fused multiply-adds in tap order from 0, acc = fma(window[i],
 * v[i], acc).  They are formed ABOUT A PIVOT so that constant areas do not cancel: per tile and per image, c_p (c_t) is the element
 * of p (t) at row min(y0 + 5 + tile_h / 2, H - 1), column min(x0 + 5 + tile_w / 2, W - 1) of the channel, (y0, x0) the tile's first map
 * position, or 0 where that element is not finite.  The tile holds d = fl(p - c_p), e = fl(t - c_t); the five chains sum d, e, fl(d d),
 * fl(e e), fl(d e).  From the five fp32 moments m_d, m_e, s_dd, s_ee, s_de everything else is double: mu_p = c_p + m_d, mu_t = c_t +
 * m_e, var_p = s_dd - m_d^2, var_t = s_ee - m_e^2, cov = s_de - m_d m_e, and the SSIM expression above.
 * NaN.  A NaN in row r's pred, or in truth[r % N], makes slots 0, 1 and 2 of row r NaN (every element lies in some window); slots 3
 * and 4 iff the NaN's element is hole; slot 5 iff a hole-centred position's window holds the NaN's element.  Slots 6 and 7 never
 * depend on pred or truth.  No other row is touched: a row reads nothing but its own pred, its truth and its keep.
 * Refused: pred, truth, out or ws NULL; R, N, C, H, W <= 0; R % N != 0; H < 11 or W < 11; keep given with Ck outside {1, C};
 * data_range <= 0 or not finite; C H W or R past 2^31 - 1; ws_bytes below mdm_metric_ws_bytes(R, C, H, W); ws off an 8-byte boundary. */
int mdm_metric_image(const float* pred, const float* truth, const float* keep, int Ck, int64_t R, int N, int C, int H, int W,
                     float clamp_lo, float clamp_hi, float data_range, void* ws, int64_t ws_bytes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_METRIC_H */
