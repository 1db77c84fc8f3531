/* mdm_data.h -- the data ABI of libmdm_hip.so: a data set resident in device memory, batches gathered by one launch.
 *
 * A third header of the same library.  include/mdm_hip.h stays the statement of the training / sampling ABI and include/mdm_vis.h of
 * the presentation ABI; what is declared here feeds the train step and is bound next to them (mdm/_lib.py: DATA_PROTOS /
 * DATA_EXPORTS).  Same conventions: every pointer is a DEVICE pointer, every function returns 0 or non-zero with the text in
 * mdm_last_error, a refused call launches nothing, the stream is the last parameter, nothing here allocates or synchronises.
 *
 * Replaces upstream's MyDataset.__getitem__ (utils/mydataset.py:270-278) behind DataLoader(shuffle=True, drop_last=True, pin_memory=True)
 * (main_train_masked.py:92-102) -- index, collate, pin and copy on the host per batch there; one launch that writes the batch where
 * the train step reads it here -- and the DataLoader pass of main_train_masked.py:60-73 that takes the means of every image.
 *
 * Storage, for both functions: `src` holds M images [C][H][W]; image m starts at element m img_stride (img_stride >= C H W).
 *   kind 0: float elements, taken bit for bit.
 *   kind 1: uint8 elements, the value is lut[byte]; lut is 256 floats made once by the host (for upstream's ToTensor +
 *           Normalize([0.5], [0.5]) it is (u.float().div(255) - 0.5) / 0.5 over arange(256) as torch computes it: the kernel holds
 *           no arithmetic, so the values are torch's by construction).
 * All offsets are 64-bit.  src, img_stride and C H W may have any alignment: 16-byte loads and stores (4-byte loads of uint8 storage)
 * run where the addresses allow them, which they do everywhere when the pointers are 16-byte aligned and C H W and W are multiples of 4.
 */
#ifndef MDM_DATA_H
#define MDM_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One batch in one launch: x0[n] = image index[first + n] for n in [0, N); x0 is [N][C][H][W] float, contiguous.
 *   index      int64, at least first + N entries; repeats are allowed.  An entry outside [0, M) reads nothing and writes NaN to every
 *              element of x0[n], to label_out[n] and to random_out[n][0 .. R): a bad index is a defined, visible result.
 *   flip       NULL or N bytes; non-zero: image n is written mirrored along W.
 *   label_out  NULL or [N]:    label_out[n] = label[idx]                       (label is [M] float)
 *   random_out NULL or [N][R]: random_out[n][r] = random[idx R + r], r < R     (random is [M][R] float)
 * Refused: src, index or x0 NULL; kind outside {0, 1}; kind 1 without lut; M, N, C, H, W <= 0; C H W past 2^31 - 1;
 * img_stride < C H W; first < 0; label_out without label; random_out without random or with R <= 0. */
int mdm_data_gather(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                    const int64_t* index, int64_t first, int N, const uint8_t* flip, float* x0,
                    const float* label, const float* random, int R, float* label_out, float* random_out, void* stream);

/* Means of the stored values (read as mdm_data_gather reads them):
 *   per_channel == 0: out[M][1], the mean over the C H W elements of an image
 *   per_channel != 0: out[M][C], the mean over the H W elements of a channel
 * Summed in double in a fixed order (no floating-point atomics: two runs give the same bits), divided in double, rounded once to float.
 * Refused: src or out NULL; kind outside {0, 1}; kind 1 without lut; M, C, H, W <= 0; C H W past 2^31 - 1; img_stride < C H W;
 * more than 2^31 - 1 means. */
int mdm_data_means(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                   int per_channel, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDM_DATA_H */
