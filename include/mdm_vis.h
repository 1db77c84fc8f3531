/* mdm_vis.h -- the presentation ABI of libmdm_hip.so: image grids built on the device.
 *
 * A second header of the same library.  include/mdm_hip.h stays the statement of the training / sampling ABI; what is declared
 * here draws pictures of its tensors and is bound next to it (mdm/_lib.py: VIS_PROTOS / VIS_EXPORTS).  Same conventions:
 * every pointer is a DEVICE pointer unless it says host, every function returns 0 or non-zero with the text in
 * mdm_last_error, a refused call launches nothing, the stream is the last parameter of whatever launches, nothing here
 * allocates or synchronises.
 *
 * Replaces upstream's normalize01 / normalize01_global (utils/datautils.py:211-229) + torchvision make_grid + the float -> uint8
 * sequence of save_image, as Sampler._save_image_grid (sampler.py:369-387) chains them: three or four torch passes, K narrow
 * copies and a host-side conversion per grid there; one range launch and one grid launch here, and what leaves the GPU is uint8.
 */
#ifndef MDM_VIS_H
#define MDM_VIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 32-bit words of the scratch block mdm_vis_range takes for a global range (below). */
#define MDM_VIS_RANGE_SCRATCH_FLOATS 4

/* Host only.  The grid of K images [C][H][W] laid out `nrow` to a row with `padding` pixels between and around them:
 * out = {Cg, Hg, Wg}.
 *   Cg = 3 when C == 1 (a single channel is written three times), else C.
 *   K == 1: the grid is the image, Hg = H, Wg = W, no border.
 *   else:   xmaps = min(nrow, K), ymaps = ceil(K / xmaps), Hg = ymaps (H + padding) + padding, Wg = xmaps (W + padding) + padding;
 *           image k has its corner at row (k / xmaps)(H + padding) + padding, column (k % xmaps)(W + padding) + padding.
 * Refused: K, C, H, W, nrow <= 0, padding < 0, out NULL, Hg or Wg past 2^31 - 1. */
int mdm_vis_grid_shape(int K, int C, int H, int W, int nrow, int padding, int32_t out[3]);

/* {min, max} of each of K images of E contiguous floats; image k starts at x + k img_stride (elements, img_stride >= E).
 *   global == 0: lohi[K][2], one pair per image; scratch is not read (NULL is fine).
 *   global != 0: lohi[1][2], one pair over all K E elements.  ONE launch: every workgroup folds its pair into `scratch` with
 *                device-scope integer atomics and the one that finishes last writes lohi.  scratch: MDM_VIS_RANGE_SCRATCH_FLOATS
 *                32-bit words, 16-byte aligned, ZERO before the first call; the kernel leaves them zero, so the block is
 *                zeroed once, when it is allocated.  One block per stream that may run this concurrently.
 * torch's amin / amax / min / max: a NaN anywhere in the range makes BOTH words NaN.  Min and max do not depend on the order of
 * the reduction, so the result has one possible bit pattern.  Any E, any alignment of x and img_stride (16-byte loads run over
 * the aligned middle of what a workgroup reads).
 * Refused: x or lohi NULL, K or E <= 0, img_stride < E, global without scratch. */
int mdm_vis_range(const float* x, int64_t img_stride, int K, int E, int global, float* lohi, float* scratch, void* stream);

/* Normalise, place and quantise in one launch: K images [C][H][W] at x + k img_stride -> the grid of mdm_vis_grid_shape.
 *   mode 0: v = x
 *   mode 1: v = (x - lo_k) / (hi_k - lo_k) with lohi[K][2], then NaN -> 0: upstream's normalize01, bit for bit what mdm_normalize01
 *           writes (a constant image and an image with a NaN pixel come out all 0)
 *   mode 2: v = (x - lo) / (hi - lo) with lohi[1][2], no NaN handling: normalize01_global (a constant batch gives NaN, as upstream)
 * Every element that no image covers -- borders and the cells of an unfilled last row -- is pad_value (not normalised).
 *   grid_f32 [Cg][Hg][Wg]  the value (what make_grid returns)
 *   grid_u8  [Hg][Wg][Cg]  (uint8) clamp(v 255 + 0.5, 0, 255): save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8); the product
 *                          and the sum are rounded separately (no fused multiply-add), NaN -> 0 (torch leaves that undefined)
 * Either output may be NULL, not both.  Any alignment of the three pointers (16-byte loads and stores, 4-byte stores of grid_u8,
 * run where the addresses allow them).
 * Refused: x NULL, K, C, H, W, nrow <= 0, padding < 0, img_stride < C H W, both outputs NULL, mode outside {0, 1, 2}, mode != 0
 * without lohi, Hg or Wg past 2^31 - 1. */
int mdm_vis_grid(const float* x, int64_t img_stride, int K, int C, int H, int W, const float* lohi, int mode, int nrow,
                 int padding, float pad_value, float* grid_f32, uint8_t* grid_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_VIS_H */
