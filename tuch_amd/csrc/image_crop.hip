// The regressor's input crops (tuch/utils/imutils.py:67-106 crop + tuch/datasets/base_dataset.py:192-205 rgb_processing)
// for a whole batch in ONE launch: box, rotation, flip, resize with K x K supersampling, pixel noise, clamp, /255 and
// normalisation.  The resampling rule is stated above tuch_crop_batch in include/tuch_amd.h; sample positions are 64-bit
// integers (units of 2^-16 px) computed from the per-sample records the host built, so no float decides which texel is
// read, and tests/image_cases.py restates the same integers.
//
// Shape: one thread per output pixel and all its channels; a workgroup is 256 consecutive pixels of one sample, so a
// wavefront stores runs of 64 floats (256 B) per channel plane.  Texels are fetched directly: neighbouring lanes read
// neighbouring texels (rot = 0: the same source rows; rotated: a slanted band a few rows high), which the vector L1 and
// the L2 serve; at the sizes of a training batch the kernel is bound by its 38.5 MB of stores.
#include "common.h"

// include/tuch_amd.h: tuch_crop_record (120 bytes; tuch_amd/ops.py CROP_RECORD is the same layout)
struct tuch_crop_record {
    int64_t offset, stride;
    int64_t ax[3], ay[3];
    int32_t height, width, channels, type;
    int32_t pw, ph, ox, oy;
    int32_t K, flip;
    float pn[3];
    int32_t reserved;
};
static_assert(sizeof(tuch_crop_record) == 120, "tuch_crop_record is 120 bytes in the header and in the binding");

namespace {

constexpr int kBlock = 256;
constexpr int kMaxRes = 1024;      // 2 K R <= 2^15: the integer affine stays far inside 64 bits (see crop_records)
constexpr int kMaxK = 16;

struct CropNorm { float mean[3], std[3]; };

// the record is usable: every address the fetch can form lies inside [offset, offset + (H-1) stride + row bytes) and that
// inside the buffer.  The binding checks the same on the host before the launch; a record that fails here gives zeros.
static __device__ __forceinline__ bool record_ok(const tuch_crop_record& r, size_t buffer_bytes, int out_channels)
{
    if (r.type != 0 && r.type != 1) return false;
    if (r.channels != 1 && r.channels != 3) return false;
    if (r.channels == 3 && out_channels != 3) return false;
    if (r.K < 1 || r.K > kMaxK) return false;
    if (r.height < 1 || r.width < 1 || r.pw < 1 || r.ph < 1) return false;
    const int lim = 1 << 29;                            // texel index + origin stays an int
    if (r.pw > lim || r.ph > lim || r.ox < -lim || r.ox > lim || r.oy < -lim || r.oy > lim) return false;
    const long long es = r.type ? 4 : 1;
    const long long row = (long long)r.width * r.channels * es;
    if (r.offset < 0 || r.stride < row) return false;
    if (r.type && ((r.offset | r.stride) & 3)) return false;
    if (r.stride > (1ll << 40) || r.offset > (1ll << 60)) return false;
    const long long end = r.offset + (long long)(r.height - 1) * r.stride + row;
    return end >= 0 && (unsigned long long)end <= (unsigned long long)buffer_bytes;
}

template <int C, bool kFloat>
static __device__ __forceinline__ void texel(const uint8_t* __restrict__ img, long long stride, int H, int W, int sx, int sy,
                                             float (&t)[C])
{
    if ((unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H) {
        if (kFloat) {
            const float* p = (const float*)(img + (long long)sy * stride) + (long long)sx * C;
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = p[c];
        } else {
            const uint8_t* p = img + (long long)sy * stride + (long long)sx * C;
#pragma unroll
            for (int c = 0; c < C; ++c) t[c] = (float)p[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = 0.f;
    }
}

#pragma clang fp contract(off)
// sum over the K x K samples of pixel (i, j), rows of samples outermost, every sample a bilinear fetch:
//   top = fma(t01, wx, t00 (1 - wx)), bottom likewise, sample = fma(bottom, wy, top (1 - wy)); acc += sample
template <int C, bool kFloat>
static __device__ __forceinline__ void gather(const tuch_crop_record& r, const uint8_t* __restrict__ img, int R, int i, int j,
                                              float (&acc)[C])
{
    const int K = r.K;
    const long long g0x = r.flip ? (long long)2 * K * R - ((long long)2 * K * j + 1) : (long long)2 * K * j + 1;
    const long long stepx = r.flip ? -2 : 2;
    const long long g0y = (long long)2 * K * i + 1;
    // unshifted positions (32 fractional bits) of sample (u, v) = (0, 0); a step in u or v is an exact integer add
    const long long x00 = r.ax[0] * g0x + r.ax[1] * g0y + r.ax[2];
    const long long y00 = r.ay[0] * g0x + r.ay[1] * g0y + r.ay[2];
    const long long dxu = r.ax[0] * stepx, dyu = r.ay[0] * stepx, dxv = r.ax[1] * 2, dyv = r.ay[1] * 2;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int v = 0; v < K; ++v) {
        long long xs = x00 + dxv * v, ys = y00 + dyv * v;
        for (int u = 0; u < K; ++u, xs += dxu, ys += dyu) {
            const long long X = xs >> 16, Y = ys >> 16;             // units of 2^-16 px, texel-index coordinates of P
            const long long ix = X >> 16, iy = Y >> 16;
            const float wx = (float)(int)(X & 0xffff) * (1.0f / 65536.0f), wy = (float)(int)(Y & 0xffff) * (1.0f / 65536.0f);
            const float ux = (float)(65536 - (int)(X & 0xffff)) * (1.0f / 65536.0f);
            const float uy = (float)(65536 - (int)(Y & 0xffff)) * (1.0f / 65536.0f);
            const long long px = r.pw - 1, py = r.ph - 1;
            const int x0 = (int)(ix < 0 ? 0 : ix > px ? px : ix) + r.ox, x1 = (int)(ix + 1 < 0 ? 0 : ix + 1 > px ? px : ix + 1) + r.ox;
            const int y0 = (int)(iy < 0 ? 0 : iy > py ? py : iy) + r.oy, y1 = (int)(iy + 1 < 0 ? 0 : iy + 1 > py ? py : iy + 1) + r.oy;
            float t00[C], t01[C], t10[C], t11[C];
            texel<C, kFloat>(img, r.stride, r.height, r.width, x0, y0, t00);
            texel<C, kFloat>(img, r.stride, r.height, r.width, x1, y0, t01);
            texel<C, kFloat>(img, r.stride, r.height, r.width, x0, y1, t10);
            texel<C, kFloat>(img, r.stride, r.height, r.width, x1, y1, t11);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float top = __builtin_fmaf(t01[c], wx, t00[c] * ux);
                const float bot = __builtin_fmaf(t11[c], wx, t10[c] * ux);
                acc[c] = acc[c] + __builtin_fmaf(bot, wy, top * uy);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void crop_kernel(const uint8_t* __restrict__ buffer, size_t buffer_bytes,
                                                      const tuch_crop_record* __restrict__ records, int R, int CO, CropNorm nrm,
                                                      float* __restrict__ out, float* __restrict__ raw)
{
    const int b = blockIdx.y;
    const int pix = blockIdx.x * kBlock + threadIdx.x;
    if (pix >= R * R) return;
    const tuch_crop_record r = records[b];
    const int i = pix / R, j = pix - i * R;
    float m[3] = {0.f, 0.f, 0.f};
    if (record_ok(r, buffer_bytes, CO)) {
        const uint8_t* img = buffer + r.offset;
        if (r.channels == 3) {
            float a[3];
            if (r.type) gather<3, true>(r, img, R, i, j, a); else gather<3, false>(r, img, R, i, j, a);
            m[0] = a[0]; m[1] = a[1]; m[2] = a[2];
        } else {
            float a[1];
            if (r.type) gather<1, true>(r, img, R, i, j, a); else gather<1, false>(r, img, R, i, j, a);
            m[0] = m[1] = m[2] = a[0];
        }
    }
    const float kk = (float)(r.K * r.K);
    const size_t plane = (size_t)R * R;
    for (int c = 0; c < CO; ++c) {
        float v = (m[c] / kk) * r.pn[c];
        v = __builtin_fminf(255.0f, __builtin_fmaxf(0.0f, v));      // base_dataset.py:200-202 (a NaN becomes 0)
        const float q = v / 255.0f;
        const size_t at = ((size_t)b * CO + c) * plane + pix;
        if (raw) raw[at] = q;
        out[at] = (q - nrm.mean[c]) / nrm.std[c];
    }
}
#pragma clang fp contract(fast)

}  // namespace

extern "C" int tuch_crop_batch(const void* buffer, size_t buffer_bytes, const tuch_crop_record* records, int B, int res,
                               int channels, const float* mean, const float* std, float* out, float* raw, void* stream)
{
    TUCH_REQUIRE(B >= 0 && B <= 65535, "tuch_crop_batch: B must be in [0, 65535]");
    TUCH_REQUIRE(res >= 1 && res <= kMaxRes, "tuch_crop_batch: res must be in [1, %d]", kMaxRes);
    TUCH_REQUIRE(channels == 1 || channels == 3, "tuch_crop_batch: 1 or 3 output channels");
    if (B == 0) return TUCH_OK;
    TUCH_REQUIRE(buffer && records && mean && std && out, "tuch_crop_batch: null pointer");
    CropNorm nrm = {};
    for (int c = 0; c < channels; ++c) {
        TUCH_REQUIRE(std[c] != 0.f && std[c] == std[c] && mean[c] == mean[c], "tuch_crop_batch: std must be non-zero");
        nrm.mean[c] = mean[c];
        nrm.std[c] = std[c];
    }
    hipLaunchKernelGGL(crop_kernel, dim3(ceil_div(res * res, kBlock), B), dim3(kBlock), 0, (hipStream_t)stream,
                       (const uint8_t*)buffer, buffer_bytes, records, res, channels, nrm, out, raw);
    return tuch_check_launch("tuch_crop_batch");
}
