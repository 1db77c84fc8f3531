/* mdm_ingest.h -- the ingest ABI of libmdm_hip.so: decoded image files become the uint8 storage of include/mdm_data.h, resized and
 * cropped on the device byte for byte as PIL resizes and torchvision crops.
 *
 * A fifth header of the same library.  include/mdm_hip.h stays the statement of the training / sampling ABI, include/mdm_vis.h of the
 * presentation ABI, include/mdm_data.h of the data ABI and include/mdm_interp.h of the interpolation sampler; what is declared here
 * is bound next to them (mdm/_lib.py: INGEST_PROTOS / INGEST_EXPORTS).  Same conventions: every function returns 0 or non-zero with
 * the text in mdm_last_error, a refused call launches nothing, the stream is the last parameter, nothing here allocates or
 * synchronises.  mdm_ingest_plan and mdm_ingest_launch_of are host code with HOST pointers and no stream; mdm_ingest_resize_crop
 * takes DEVICE pointers.
 *
 * Replaces the transform of upstream's get_dataset (utils/mydataset.py:77-83: Resize(size), CenterCrop(size), ToTensor(),
 * Normalize([0.5], [0.5]) on the PIL image an ImageFolder opens) as MyDataset.__init__ runs it over the whole set (:245-265).
 * Resize on a PIL image is PIL's antialiased bilinear filter in 22-bit fixed point: a horizontal pass, a rounding to uint8, a
 * vertical pass.  The crop keeps a window of the resized image, so only that window is planned and computed.  ToTensor and Normalize
 * are the 256-entry table of mdm_data.h.
 */
#ifndef MDM_INGEST_H
#define MDM_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The filter table of ONE axis for the output positions [first, first + count) of a resize from in_size to out_size samples: PIL's
 * bilinear precompute_coeffs followed by normalize_coeffs_8bpc.  Host only: bounds and coeffs are HOST arrays, nothing is launched.
 * In double, with floating-point contraction off:
 *     scale = in_size / out_size;  fs = max(scale, 1);  support = fs;  ks = 2 (int)ceil(support) + 1
 *     output xx:  center = (xx + 0.5) scale;  xmin = max((int)(center - support + 0.5), 0)
 *                 xmax = min((int)(center + support + 0.5), in_size) - xmin
 *     weight x < xmax:  a = (x + xmin - center + 0.5) / fs;  w = 1 - |a| if |a| < 1, else 0;  a non-zero sum divides every weight
 *     fixed point:  (int)(w 2^22 + 0.5), or - 0.5 for a negative w (the cast truncates)
 *   bounds  NULL or [count][2] int32: xmin, xmax (first source index, number of taps)
 *   coeffs  NULL or [count][ks] int32, zero behind the xmax taps of a row
 * Returns ks (>= 3), also with bounds and coeffs both NULL; a table for in_size == out_size is the identity.
 * Refused (returns -1): in_size, out_size or count <= 0; first < 0; first + count > out_size; one of bounds, coeffs without the other. */
int mdm_ingest_plan(int in_size, int out_size, int first, int count, int32_t* bounds, int32_t* coeffs);

/* K decoded images of ONE shape, resized and cropped into planar uint8 storage by one launch.
 *   src      [K][h][w][C] uint8, interleaved as numpy.asarray(pil_image) gives it; image k starts at byte k src_stride
 *            (src_stride >= h w C); C is 1 or 3; any alignment (16-byte loads run over the aligned middle of every row)
 *   hbounds, hcoeffs   the DEVICE copy of mdm_ingest_plan(w, ow, left, S): [S][2] and [S][ksh] int32, the S kept columns
 *   vbounds, vcoeffs   the DEVICE copy of mdm_ingest_plan(h, oh, top, S):  [S][2] and [S][ksv] int32, the S kept rows
 *   dst      M images [C][S][S] uint8, image m at byte m dst_stride (dst_stride >= C S S): the kind-1 storage of mdm_data.h.
 *            dst[(first + k) dst_stride + c S S + y S + x] is written for k < K; no other byte is.
 * Horizontal pass first: t = clip((2^21 + sum_i pixel[xmin + i] coeff[i]) >> 22, 0, 255) AS uint8; the vertical pass is the same
 * formula over those uint8 values.  Both passes always run.  Integer arithmetic without atomics: the same bits on every run.
 * The tables are device memory the host cannot check, so the kernel clamps: a first index into [0, size - 1], a tap count into
 * [0, ks]; a tap on a column past the last one reads the last one, a tap on a row past the last one is dropped.  (A table of
 * mdm_ingest_plan meets none of these clamps.)  Whatever the tables hold, nothing outside the K source images is read and nothing
 * outside the K destination images is written: a wrong table gives wrong pixels, never a fault.
 * One workgroup per (image, tile of output rows) walks the tile's source rows once; LDS and registers do not grow with the scale.
 * Refused: a NULL pointer; C outside {1, 3}; K, h, w, S, M <= 0; ksh or ksv < 1; src_stride < h w C; dst_stride < C S S;
 * first < 0 or first + K > M; h w C or C S S past 2^31 - 1; a source row (w C bytes, twice) and one row of S C accumulators that do
 * not fit the 64 KiB of LDS of a workgroup. */
int mdm_ingest_resize_crop(const uint8_t* src, int64_t src_stride, int K, int h, int w, int C,
                           const int32_t* hbounds, const int32_t* hcoeffs, int ksh,
                           const int32_t* vbounds, const int32_t* vcoeffs, int ksv,
                           uint8_t* dst, int64_t dst_stride, int64_t M, int64_t first, int S, void* stream);

/* The launch mdm_ingest_resize_crop would make for a source row of w pixels of C channels, S kept columns and a horizontal table of
 * ksh taps, without making it.  Host only: no stream, no device, nothing is launched.  It is the launcher's own statement of its
 * geometry (the launcher asks the same function), so a test that wants a given kernel instantiation or row tile asks here.
 *   out[0]  TR: the output rows of one workgroup, min(S, 8) shrunk until two row buffers (w C + 16 bytes, rounded up to 16, each),
 *           TR S C int32 accumulators and 2 TR vertical bounds fit the 64 KiB of LDS of a workgroup
 *   out[1]  1 when the horizontal table (S (2 + ksh) int32) fits behind them and is copied into LDS, 0 when the kernel reads it
 *           from global memory -- the two instantiations of the kernel
 *   out[2]  the dynamic LDS of a workgroup in bytes, the table included when it is in LDS (<= 65536)
 *   out[3]  the workgroups per image, ceil(S / TR); the last one has S - (out[3] - 1) TR rows
 * Refused: out NULL; C outside {1, 3}; w or S <= 0; ksh < 1; and what does not fit at TR = 1, exactly where and in the words with
 * which mdm_ingest_resize_crop refuses it. */
int mdm_ingest_launch_of(int w, int C, int S, int ksh, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* MDM_INGEST_H */
