// The data set in device memory (include/mdm_data.h): one launch gathers a batch -- images by index, optionally mirrored, with their
// label and random rows -- into the buffer the train step reads, and one launch takes the means of every image or channel.
//
// Replaces reference utils/mydataset.py:270-278 (MyDataset.__getitem__) behind the DataLoader of main_train_masked.py:92-102, and the
// statistics pass of main_train_masked.py:60-73.  Both kernels stream.  The gather is driven by its OUTPUT like the grid kernel of
// vis.hip: a lane owns four consecutive elements of x0 and looks up where they come from, so every store is whole.  uint8 storage goes
// through a 256-entry table the host made: there is no arithmetic here, a value is a copy of the stored float or of a table entry.
#include "common.h"
#include "../../include/mdm_data.h"

namespace mdm {

struct GatherArgs {
    const void* src;
    const float* lut;
    const int64_t* index;
    const uint8_t* flip;
    float* x0;
    const float *label, *random;
    float *label_out, *random_out;
    int64_t img_stride, M, first, total;       // total = N E
    int E, W, N, R, x_vec;
};

// the value of stored element `off`
template <int KIND> __device__ __forceinline__ float data_value(const void* src, const float* lut, int64_t off) {
    if (KIND == 0) return static_cast<const float*>(src)[off];
    return lut[static_cast<const uint8_t*>(src)[off]];
}
// the values of stored elements [off, off + 4): one 16-byte (kind 0) or 4-byte (kind 1) load where the address allows it
template <int KIND> __device__ __forceinline__ void data_value4(const void* src, const float* lut, int64_t off, float v[4]) {
    if (KIND == 0) {
        const float* p = static_cast<const float*>(src) + off;
        if (((uintptr_t)p & 15u) == 0) {
            const float4 q = load4(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
        }
    } else {
        const uint8_t* p = static_cast<const uint8_t*>(src) + off;
        uint32_t w;
        if (((uintptr_t)p & 3u) == 0) w = *reinterpret_cast<const uint32_t*>(p);
        else w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        v[0] = lut[w & 255u]; v[1] = lut[(w >> 8) & 255u]; v[2] = lut[(w >> 16) & 255u]; v[3] = lut[w >> 24];
    }
}
// element i of the flat output, on its own: the lanes whose four elements straddle two images or a mirrored row end
template <int KIND> __device__ __forceinline__ float gather_one(const GatherArgs& a, int64_t i) {
    const int64_t n = i / a.E;
    int e = (int)(i - n * a.E);
    const int64_t idx = a.index[a.first + n];
    if (idx < 0 || idx >= a.M) return __builtin_nanf("");
    if (a.flip && a.flip[n]) {
        const int w = e % a.W;
        e += a.W - 1 - 2 * w;
    }
    return data_value<KIND>(a.src, a.lut, idx * a.img_stride + e);
}

// lane g: elements [4g, 4g + 4) of x0 (flat over [N][E]); the first N lanes also write a label, the first N R a random element
template <int KIND> __global__ __launch_bounds__(256) void gather_kernel(GatherArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = 4 * g;
    if (i0 < a.total) {
        const int cnt = a.total - i0 < 4 ? (int)(a.total - i0) : 4;
        const int64_t n = i0 / a.E;
        const int e = (int)(i0 - n * a.E);
        float v[4];
        bool done = false;
        if (cnt == 4 && e + 3 < a.E) {                      // four elements of one image
            const int64_t idx = a.index[a.first + n];
            if (idx < 0 || idx >= a.M) {
                v[0] = v[1] = v[2] = v[3] = __builtin_nanf("");
                done = true;
            } else if (!(a.flip && a.flip[n])) {
                data_value4<KIND>(a.src, a.lut, idx * a.img_stride + e, v);
                done = true;
            } else {
                const int w = e % a.W;
                if (w + 3 < a.W) {                          // four pixels of one row: columns W-4-w .. W-1-w, read forwards, written backwards
                    float t[4];
                    data_value4<KIND>(a.src, a.lut, idx * a.img_stride + e + (a.W - 4 - 2 * w), t);
                    v[0] = t[3]; v[1] = t[2]; v[2] = t[1]; v[3] = t[0];
                    done = true;
                }
            }
        }
        if (!done)
            for (int j = 0; j < cnt; ++j) v[j] = gather_one<KIND>(a, i0 + j);
        if (cnt == 4 && a.x_vec) store4(a.x0 + i0, make_float4(v[0], v[1], v[2], v[3]));
        else for (int j = 0; j < cnt; ++j) a.x0[i0 + j] = v[j];
    }
    if (a.label_out && g < a.N) {
        const int64_t idx = a.index[a.first + g];
        a.label_out[g] = idx < 0 || idx >= a.M ? __builtin_nanf("") : a.label[idx];
    }
    if (a.random_out && g < (int64_t)a.N * a.R) {
        const int64_t n = g / a.R, r = g - n * a.R;
        const int64_t idx = a.index[a.first + n];
        a.random_out[g] = idx < 0 || idx >= a.M ? __builtin_nanf("") : a.random[idx * a.R + r];
    }
}

// ------------------------------------------------------------------ means
// sum of the values of stored elements [off, off + len) in double, every lane of the workgroup its own elements in a fixed order:
// scalar loads up to the first 16-byte boundary, 16-byte loads over the aligned middle, scalar loads behind it
template <int KIND> __device__ __forceinline__ double means_span(const void* src, const float* lut, int64_t off, int len, int t) {
    double s = 0.0;
    if (KIND == 0) {
        const float* p = static_cast<const float*>(src) + off;
        int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
        if (((uintptr_t)p & 3u) != 0 || head > len) head = len;
        for (int64_t i = t; i < head; i += 256) s += (double)p[i];
        const float* q = p + head;
        const int n4 = (len - head) >> 2;
        for (int64_t i = t; i < n4; i += 256) {
            const float4 v = load4(q + 4 * i);
            s += (double)v.x; s += (double)v.y; s += (double)v.z; s += (double)v.w;
        }
        for (int64_t i = (int64_t)head + 4 * (int64_t)n4 + t; i < len; i += 256) s += (double)p[i];
    } else {
        const uint8_t* p = static_cast<const uint8_t*>(src) + off;
        int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u);
        if (head > len) head = len;
        for (int64_t i = t; i < head; i += 256) s += (double)lut[p[i]];
        const uint8_t* q = p + head;
        const int n16 = (len - head) >> 4;
        for (int64_t i = t; i < n16; i += 256) {
            const uint4 v = *reinterpret_cast<const uint4*>(q + 16 * i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s += (double)lut[w[j] & 255u]; s += (double)lut[(w[j] >> 8) & 255u];
                s += (double)lut[(w[j] >> 16) & 255u]; s += (double)lut[w[j] >> 24];
            }
        }
        for (int64_t i = (int64_t)head + 16 * (int64_t)n16 + t; i < len; i += 256) s += (double)lut[p[i]];
    }
    return s;
}

// one workgroup per mean: workgroup b = (image, part) with `parts` means of `len` elements per image
template <int KIND> __global__ __launch_bounds__(256) void means_kernel(const void* src, const float* lut, int64_t img_stride, int parts,
                                                                        int len, float* out) {
    __shared__ double s_sum[4];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x, m = b / parts, c = b - m * parts;
    double s = means_span<KIND>(src, lut, m * img_stride + c * len, len, t);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);      // a butterfly: one order of additions, whatever the timing
    if ((t & 63) == 0) s_sum[t >> 6] = s;
    __syncthreads();
    if (t == 0) out[b] = (float)(((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])) / (double)len);
}

static int data_storage_ok(const char* who, const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W,
                           const float* lut) {
    MDM_REQUIRE(src, "%s: src is NULL", who);
    MDM_REQUIRE(kind == 0 || kind == 1, "%s: kind %d is not 0 (float) or 1 (uint8)", who, kind);
    MDM_REQUIRE(kind == 0 || lut, "%s: kind 1 needs lut", who);
    MDM_REQUIRE(M > 0, "%s: M must be positive (%lld)", who, (long long)M);
    MDM_REQUIRE(C > 0 && H > 0 && W > 0, "%s: C, H, W must be positive (%d, %d, %d)", who, C, H, W);
    MDM_REQUIRE((int64_t)C * H * W <= INT32_MAX, "%s: C H W = %lld is past 2^31 - 1", who, (long long)((int64_t)C * H * W));
    MDM_REQUIRE(img_stride >= (int64_t)C * H * W, "%s: img_stride %lld < C H W", who, (long long)img_stride);
    return 0;
}

}  // namespace mdm
using namespace mdm;

extern "C" int mdm_data_gather(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                               const int64_t* index, int64_t first, int N, const uint8_t* flip, float* x0, const float* label,
                               const float* random, int R, float* label_out, float* random_out, void* stream) {
    if (int rc = data_storage_ok("data_gather", src, kind, img_stride, M, C, H, W, lut)) return rc;
    MDM_REQUIRE(index, "data_gather: index is NULL");
    MDM_REQUIRE(x0, "data_gather: x0 is NULL");
    MDM_REQUIRE(N > 0, "data_gather: N must be positive (%d)", N);
    MDM_REQUIRE(first >= 0, "data_gather: first %lld is negative", (long long)first);
    MDM_REQUIRE(!label_out || label, "data_gather: label_out needs label");
    MDM_REQUIRE(!random_out || random, "data_gather: random_out needs random");
    MDM_REQUIRE(!random_out || R > 0, "data_gather: random_out needs R > 0 (%d)", R);
    GatherArgs a;
    a.src = src; a.lut = lut; a.index = index; a.flip = flip; a.x0 = x0;
    a.label = label; a.random = random; a.label_out = label_out; a.random_out = random_out;
    a.img_stride = img_stride; a.M = M; a.first = first;
    a.E = C * H * W; a.W = W; a.N = N; a.R = random_out ? R : 0;
    a.total = (int64_t)N * a.E;
    a.x_vec = (int)(((uintptr_t)x0 & 15u) == 0);
    int64_t lanes = (a.total + 3) / 4;
    if (lanes < N) lanes = N;
    if (lanes < (int64_t)N * a.R) lanes = (int64_t)N * a.R;
    const int64_t blocks = (lanes + 255) / 256;
    MDM_REQUIRE(blocks <= INT32_MAX, "data_gather: N C H W = %lld is too many elements for one launch", (long long)a.total);
    if (kind == 0) hipLaunchKernelGGL(gather_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(gather_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status("data_gather");
}

extern "C" int mdm_data_means(const void* src, int kind, int64_t img_stride, int64_t M, int C, int H, int W, const float* lut,
                              int per_channel, float* out, void* stream) {
    if (int rc = data_storage_ok("data_means", src, kind, img_stride, M, C, H, W, lut)) return rc;
    MDM_REQUIRE(out, "data_means: out is NULL");
    const int parts = per_channel ? C : 1, len = per_channel ? H * W : C * H * W;
    MDM_REQUIRE(M <= INT32_MAX / parts, "data_means: M x parts = %lld x %d means are too many for one launch", (long long)M, parts);
    if (kind == 0)
        hipLaunchKernelGGL(means_kernel<0>, dim3((unsigned)(M * parts)), dim3(256), 0, (hipStream_t)stream, src, lut, img_stride, parts, len, out);
    else
        hipLaunchKernelGGL(means_kernel<1>, dim3((unsigned)(M * parts)), dim3(256), 0, (hipStream_t)stream, src, lut, img_stride, parts, len, out);
    return launch_status("data_means");
}
