// Raw-frame ingest: the reference's per-frame ImageResize(max_img_size, "bilinear") + ImagePad(max_img_size, max_img_size)
// (src/datasets/data_utils.py:112-253, applied in src/datasets/dataset_base.py:270-273) + ImageNorm (:256-276) + the RGB -> BGR flip
// (src/modeling/grid_feat.py:92-94), from the decoder's native-resolution uint8 frames straight into the packed NHWC4 image the stem
// reads -- one launch for a ragged batch (every frame its own size), geometry from a device table, no host synchronisation.
//
// One pass, HBM-bound: one thread per destination pixel with w fastest and one 8 / 16-byte store per pixel, as stem_pack_kernel; the
// frame index is the grid's y axis, so a frame's table row is wave-uniform (scalar loads).  The 12 tap bytes of a pixel are plain byte
// loads: neighbouring threads read neighbouring source pixels (the taps of a row sit in 2 source rows), which the caches absorb.
//
// Arithmetic = PyTorch's upsample_bilinear2d, align_corners=False, no antialiasing, fp32.  Every fused multiply-add is WRITTEN as one
// (the host emulator build and hipcc then evaluate the same operations whatever -ffp-contract says): the single rounding of the source
// coordinate is what keeps the result within 2 fp32 ulp at 255 of the reference's F.interpolate.
//
// Two sources feed the same pixel routine (resize_pack_pixel): packed RGB bytes (cb_resize_pack_u8) and the planes of a YUV 4:2:0
// frame as a decoder emits them (cb_resize_pack_yuv420: I420 or NV12), whose taps are converted to RGB bytes one by one first.
//
// WHERE the buffer lies is a parameter of that routine too: in the kernel arguments (DirectBytes: the two entry points above) or in a
// 16-byte descriptor in device memory that the kernel reads (IndirectBytes: cb_resize_pack_u8_src / cb_resize_pack_yuv420_src) -- a
// captured launch then depends on no address or size of the batch and serves every batch of its (N, S).
#include "common.h"

namespace {

struct Axis { int i0, i1; float l0, l1; };

// source taps of destination index `dst` on an axis resized from `in` to `out` samples
__device__ __forceinline__ Axis axis_taps(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    Axis a;
    a.i0 = (int)src;
    a.i0 = a.i0 < in - 1 ? a.i0 : in - 1;
    a.i1 = a.i0 + 1 < in - 1 ? a.i0 + 1 : in - 1;
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

constexpr int64_t MAX_SIDE = 1 << 14;         // h, w of a source frame (3 * h * w then fits 32 bits with room to spare)

// ---- where the taps come from: frame_bytes(h, w) = what a frame occupies; tap(i, j, rgb) = R, G, B of source pixel (i, j), 0..255 ------
template <bool HWC>
struct RgbSource {                            // packed RGB: interleaved (h, w, 3) or planar (3, h, w)
    struct Params {};
    static __host__ __device__ int64_t frame_bytes(int64_t h, int64_t w) { return 3 * h * w; }
    const uint8_t* f;
    int64_t cs, ps, w;                        // channel / pixel strides in bytes, row length in pixels
    __device__ RgbSource(const uint8_t* frame, int h, int w_, Params) : f(frame), cs(HWC ? 1 : (int64_t)h * w_), ps(HWC ? 3 : 1), w(w_) {}
    __device__ __forceinline__ void tap(int i, int j, float (&rgb)[3]) const {
        const int64_t at = (i * w + j) * ps;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (float)f[c * cs + at];
    }
};

// Y'CbCr -> R'G'B' as y' = ys * (Y - yo), R = y' + rv * cr, G = y' - gu * cb - gv * cr, B = y' + bu * cb with cb = U - 128, cr = V - 128
// (the four matrices: yuv_matrix below)
struct YuvMatrix { float ys, yo, rv, gu, gv, bu; };

// The correctly rounded fp32 product as an operation of its own.  Here the choice is the OPPOSITE of the bilinear part above: the
// conversion is DEFINED as separate fp32 multiplies and adds in the written order (a numpy float32 restatement reproduces every byte:
// tests/yuv_restatement.py), so nothing may be contracted.  A plain a * b does not say that -- and neither do __fmul_rn / __fadd_rn or a
// contract(off) pragma: under hipcc -ffp-contract=fast the backend fuses whatever multiply feeds an add.  fma(a, b, +0) IS the rounded
// product (but for the sign of a zero, which no byte depends on), is kept as written, and no add can be folded into it.
__device__ __forceinline__ float mul_rn(float a, float b) { return __builtin_fmaf(a, b, 0.0f); }
__device__ __forceinline__ float to_byte(float v) {          // round to nearest even, clamp to 0..255
    v = rintf(v);
    return v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
}

template <bool NV12>
struct YuvSource {                            // 4:2:0 planes, tightly packed: Y (h x w), then U, V (ch x cw each: I420) or interleaved UV (ch x 2 cw: NV12)
    typedef YuvMatrix Params;
    static __host__ __device__ int64_t frame_bytes(int64_t h, int64_t w) { return h * w + 2 * ((h + 1) / 2) * ((w + 1) / 2); }
    const uint8_t *y, *u, *v;
    int w, cpitch;                            // row lengths of the luma plane and of a chroma row, in bytes
    YuvMatrix m;
    __device__ YuvSource(const uint8_t* frame, int h, int w_, Params m_) : y(frame), w(w_), m(m_) {
        const int ch = (h + 1) / 2, cw = (w_ + 1) / 2;
        u = frame + (int64_t)h * w_;
        v = NV12 ? u + 1 : u + (int64_t)ch * cw;
        cpitch = NV12 ? 2 * cw : cw;
    }
    // the pixel's own luma sample and the chroma sample of its 2 x 2 block (nearest replication), converted to RGB BYTES
    __device__ __forceinline__ void tap(int i, int j, float (&rgb)[3]) const {
        const int64_t at = (int64_t)(i >> 1) * cpitch + (j >> 1) * (NV12 ? 2 : 1);
        const float yy = mul_rn(m.ys, (float)y[(int64_t)i * w + j] - m.yo);
        const float cb = (float)u[at] - 128.f, cr = (float)v[at] - 128.f;
        rgb[0] = to_byte(yy + mul_rn(m.rv, cr));
        rgb[1] = to_byte(yy - mul_rn(m.gu, cb) - mul_rn(m.gv, cr));
        rgb[2] = to_byte(yy + mul_rn(m.bu, cb));
    }
};

// ---- where the buffer lies: base() / bytes(), uniform over the grid --------------------------------------------------------------------
struct DirectBytes {                          // kernel arguments
    const uint8_t* flat;
    int64_t flat_bytes;
    __device__ __forceinline__ const uint8_t* base() const { return flat; }
    __device__ __forceinline__ int64_t bytes() const { return flat_bytes; }
};
struct IndirectBytes {                        // a cb_frame_source in device memory: one address for the whole grid (scalar loads)
    const cb_frame_source* src;
    __device__ __forceinline__ const uint8_t* base() const { return src->base; }
    __device__ __forceinline__ int64_t bytes() const { return src->bytes; }
};

// dst (N, Hp, Wp, 4), channels B, G, R, 0.  Pixel (hp, wp) -> image position (y, x) = (hp - pad, wp - pad):
//   inside new_h x new_w : the bilinear sample, normalised
//   inside S x S         : the zero PIXEL ImagePad appends, normalised -- (0 - mean) * (1 / std): the reference pads before it normalises
//   elsewhere            : zeros (the convolution's halo), as cb_stem_pack writes
// A table row that does not describe a frame inside the buffer makes its frame all padding; nothing is read through it (a buffer of
// 0 bytes holds no frame: base() is then never used).
template <typename T, typename Src, typename Bytes>
__device__ __forceinline__ void resize_pack_pixel(Bytes buf, const int64_t* table, T* dst, int S, int Hp, int Wp, int pad,
                                                  f32x4 mean, f32x4 istd, typename Src::Params prm) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hp * Wp) return;
    const int y = pix / Wp - pad, x = pix % Wp - pad;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S) {
        const int64_t* row = table + (int64_t)n * 5;
        const int64_t off = row[0], h64 = row[1], w64 = row[2], nh64 = row[3], nw64 = row[4];
        const int64_t flat_bytes = buf.bytes();
        const bool ok = off >= 0 && h64 >= 1 && w64 >= 1 && h64 <= MAX_SIDE && w64 <= MAX_SIDE && nh64 >= 1 && nw64 >= 1 && nh64 <= S && nw64 <= S &&
                        off <= flat_bytes && Src::frame_bytes(h64, w64) <= flat_bytes - off;
        float rgb[3] = {0.f, 0.f, 0.f};
        if (ok && y < (int)nh64 && x < (int)nw64) {
            const int h = (int)h64, w = (int)w64;
            const Axis ay = axis_taps(y, h, (int)nh64), ax = axis_taps(x, w, (int)nw64);
            const Src src(buf.base() + off, h, w, prm);
            float p00[3], p01[3], p10[3], p11[3];
            src.tap(ay.i0, ax.i0, p00); src.tap(ay.i0, ax.i1, p01);
            src.tap(ay.i1, ax.i0, p10); src.tap(ay.i1, ax.i1, p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // l0 * a + l1 * b as fma(l0, a, l1 * b), x first, then y: the operation order of PyTorch's CPU kernel built with FMA
                // (bit-identical to F.interpolate on most shapes, <= 2 fp32 ulp at 255 otherwise); exact for l1 = 0
                const float top = __builtin_fmaf(ax.l0, p00[c], ax.l1 * p01[c]), bot = __builtin_fmaf(ax.l0, p10[c], ax.l1 * p11[c]);
                rgb[c] = __builtin_fmaf(ay.l0, top, ay.l1 * bot);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (rgb[2 - c] - mean[2 - c]) * istd[2 - c];
    }
    store4(dst + ((int64_t)n * Hp * Wp + pix) * 4, v);
}

template <typename T, bool HWC>
__global__ void __launch_bounds__(256) resize_pack_kernel(const uint8_t* flat, int64_t flat_bytes, const int64_t* table, T* dst, int S, int Hp,
                                                          int Wp, int pad, f32x4 mean, f32x4 istd) {
    resize_pack_pixel<T, RgbSource<HWC>>(DirectBytes{flat, flat_bytes}, table, dst, S, Hp, Wp, pad, mean, istd, {});
}

template <typename T, bool NV12>
__global__ void __launch_bounds__(256) resize_pack_yuv_kernel(const uint8_t* flat, int64_t flat_bytes, const int64_t* table, T* dst, int S, int Hp,
                                                              int Wp, int pad, f32x4 mean, f32x4 istd, YuvMatrix m) {
    resize_pack_pixel<T, YuvSource<NV12>>(DirectBytes{flat, flat_bytes}, table, dst, S, Hp, Wp, pad, mean, istd, m);
}

template <typename T, bool HWC>
__global__ void __launch_bounds__(256) resize_pack_src_kernel(const cb_frame_source* src, const int64_t* table, T* dst, int S, int Hp, int Wp, int pad,
                                                              f32x4 mean, f32x4 istd) {
    resize_pack_pixel<T, RgbSource<HWC>>(IndirectBytes{src}, table, dst, S, Hp, Wp, pad, mean, istd, {});
}

template <typename T, bool NV12>
__global__ void __launch_bounds__(256) resize_pack_yuv_src_kernel(const cb_frame_source* src, const int64_t* table, T* dst, int S, int Hp, int Wp,
                                                                  int pad, f32x4 mean, f32x4 istd, YuvMatrix m) {
    resize_pack_pixel<T, YuvSource<NV12>>(IndirectBytes{src}, table, dst, S, Hp, Wp, pad, mean, istd, m);
}

// BT.601 / BT.709, limited (Y 16..235, chroma 16..240) and full range: the CB_YUV_BT* codes of the header, in their order
const YuvMatrix yuv_matrix[4] = {{1.164383f, 16.f, 1.596027f, 0.391762f, 0.812968f, 2.017232f},
                                 {1.f, 0.f, 1.402f, 0.344136f, 0.714136f, 1.772f},
                                 {1.164383f, 16.f, 1.792741f, 0.213249f, 0.532909f, 2.112402f},
                                 {1.f, 0.f, 1.5748f, 0.187324f, 0.468124f, 1.8556f}};

// what every entry point asks of the arguments that do not depend on the batch
int resize_pack_check(const char* who, const void* table, int N, const float* mean3, const float* std3, const void* dst, int S, int Hp, int Wp, int pad) {
    CB_REQUIRE(table && dst && mean3 && std3, "%s: null operand", who);
    CB_REQUIRE(N > 0 && N <= 65535 && S >= 1 && pad >= 0, "%s: bad N / S / pad (%d, %d, %d)", who, N, S, pad);
    CB_REQUIRE(Hp >= S + 2 * pad && Wp >= S + 2 * pad && (int64_t)Hp * Wp < (1ll << 30), "%s: packed image %d x %d does not hold %d + 2 x %d", who, Hp, Wp, S, pad);
    CB_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0, "%s: dst / table alignment", who);
    return 0;
}

// ... and the direct ones of the buffer they are handed; the rows of a host table: cb_resize_table_check
int resize_pack_check_direct(const char* who, const void* flat, int64_t flat_bytes, const int64_t* table, const int64_t* table_host, int N, const float* mean3,
                             const float* std3, const void* dst, int S, int Hp, int Wp, int pad, int pixfmt) {
    CB_REQUIRE(flat && table && dst && mean3 && std3, "%s: null operand", who);
    CB_REQUIRE(N > 0 && N <= 65535 && S >= 1 && pad >= 0 && flat_bytes > 0, "%s: bad N / S / pad / buffer size (%d, %d, %d, %lld)", who, N, S, pad,
               (long long)flat_bytes);
    if (resize_pack_check(who, table, N, mean3, std3, dst, S, Hp, Wp, pad)) return -1;
    return table_host ? cb_resize_table_check(table_host, N, flat_bytes, S, pixfmt) : 0;
}

int resize_pack_check_src(const char* who, const cb_frame_source* src, const int64_t* table, int N, const float* mean3, const float* std3, const void* dst,
                          int S, int Hp, int Wp, int pad) {
    CB_REQUIRE(src, "%s: null operand", who);
    CB_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0, "%s: the cb_frame_source is not 16-byte aligned", who);
    return resize_pack_check(who, table, N, mean3, std3, dst, S, Hp, Wp, pad);
}

}  // namespace

extern "C" int cb_resize_table_check(const int64_t* table_host, int32_t N, int64_t flat_bytes, int32_t S, int32_t pixfmt) {
    CB_REQUIRE(pixfmt == CB_PIXFMT_RGB || pixfmt == CB_PIXFMT_I420 || pixfmt == CB_PIXFMT_NV12, "cb_resize_table_check: bad pixfmt %d (CB_PIXFMT_RGB, CB_PIXFMT_I420, CB_PIXFMT_NV12)", pixfmt);
    const bool rgb = pixfmt == CB_PIXFMT_RGB;
    // the messages name the direct entry point that would have refused the row: one text whoever runs the check
    const char *who = rgb ? "cb_resize_pack_u8" : "cb_resize_pack_yuv420", *each = rgb ? " x 3" : " 4:2:0";
    CB_REQUIRE(table_host, "%s: null host table", who);
    CB_REQUIRE(N > 0 && N <= 65535 && S >= 1, "%s: bad N / S (%d, %d)", who, N, S);
    for (int i = 0; i < N; ++i) {
        const int64_t* r = table_host + (int64_t)i * 5;
        CB_REQUIRE(r[1] >= 1 && r[2] >= 1 && r[1] <= MAX_SIDE && r[2] <= MAX_SIDE, "%s: frame %d is %lld x %lld", who, i, (long long)r[1], (long long)r[2]);
        CB_REQUIRE(r[3] >= 1 && r[4] >= 1 && r[3] <= S && r[4] <= S, "%s: frame %d resizes to %lld x %lld, outside 1..%d", who, i, (long long)r[3],
                   (long long)r[4], S);
        const int64_t need = rgb ? RgbSource<false>::frame_bytes(r[1], r[2]) : YuvSource<false>::frame_bytes(r[1], r[2]);
        CB_REQUIRE(r[0] >= 0 && r[0] <= flat_bytes && need <= flat_bytes - r[0], "%s: frame %d (offset %lld, %lld x %lld%s) leaves the %lld-byte buffer",
                   who, i, (long long)r[0], (long long)r[1], (long long)r[2], each, (long long)flat_bytes);
    }
    return 0;
}

extern "C" int cb_resize_pack_u8(int32_t dtype, const uint8_t* flat, int64_t flat_bytes, const int64_t* table, const int64_t* table_host,
                                 int32_t N, int32_t hwc, const float* mean3, const float* std3, void* dst, int32_t S, int32_t Hp, int32_t Wp,
                                 int32_t pad, void* stream) {
    if (resize_pack_check_direct("cb_resize_pack_u8", flat, flat_bytes, table, table_host, N, mean3, std3, dst, S, Hp, Wp, pad, CB_PIXFMT_RGB)) return -1;
    f32x4 mean = {mean3[0], mean3[1], mean3[2], 0.f}, istd = {1.0f / std3[0], 1.0f / std3[1], 1.0f / std3[2], 1.f};
    dim3 g((unsigned)(((int64_t)Hp * Wp + 255) / 256), (unsigned)N), b(256);
    hipStream_t st = cb_stream(stream);
    if (dtype == CB_BF16) {
        if (hwc) hipLaunchKernelGGL((resize_pack_kernel<bf16, true>), g, b, 0, st, flat, flat_bytes, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd);
        else hipLaunchKernelGGL((resize_pack_kernel<bf16, false>), g, b, 0, st, flat, flat_bytes, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd);
    } else if (dtype == CB_F32) {
        if (hwc) hipLaunchKernelGGL((resize_pack_kernel<float, true>), g, b, 0, st, flat, flat_bytes, table, (float*)dst, S, Hp, Wp, pad, mean, istd);
        else hipLaunchKernelGGL((resize_pack_kernel<float, false>), g, b, 0, st, flat, flat_bytes, table, (float*)dst, S, Hp, Wp, pad, mean, istd);
    } else return cb_fail("cb_resize_pack_u8: bad dtype");
    return cb_launch_status("cb_resize_pack_u8");
}

extern "C" int cb_resize_pack_yuv420(int32_t dtype, const uint8_t* flat, int64_t flat_bytes, const int64_t* table, const int64_t* table_host,
                                     int32_t N, int32_t layout, int32_t matrix, const float* mean3, const float* std3, void* dst, int32_t S,
                                     int32_t Hp, int32_t Wp, int32_t pad, void* stream) {
    CB_REQUIRE(dtype == CB_BF16 || dtype == CB_F32, "cb_resize_pack_yuv420: bad dtype");
    CB_REQUIRE(layout == CB_YUV_I420 || layout == CB_YUV_NV12, "cb_resize_pack_yuv420: bad layout %d (CB_YUV_I420, CB_YUV_NV12)", layout);
    CB_REQUIRE(matrix >= CB_YUV_BT601 && matrix <= CB_YUV_BT709_FULL, "cb_resize_pack_yuv420: bad matrix %d (CB_YUV_BT601 .. CB_YUV_BT709_FULL)", matrix);
    if (resize_pack_check_direct("cb_resize_pack_yuv420", flat, flat_bytes, table, table_host, N, mean3, std3, dst, S, Hp, Wp, pad, CB_PIXFMT_I420)) return -1;
    f32x4 mean = {mean3[0], mean3[1], mean3[2], 0.f}, istd = {1.0f / std3[0], 1.0f / std3[1], 1.0f / std3[2], 1.f};
    dim3 g((unsigned)(((int64_t)Hp * Wp + 255) / 256), (unsigned)N), b(256);
    hipStream_t st = cb_stream(stream);
    const YuvMatrix m = yuv_matrix[matrix];
    const bool nv12 = layout == CB_YUV_NV12;
    if (dtype == CB_BF16) {
        if (nv12) hipLaunchKernelGGL((resize_pack_yuv_kernel<bf16, true>), g, b, 0, st, flat, flat_bytes, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd, m);
        else hipLaunchKernelGGL((resize_pack_yuv_kernel<bf16, false>), g, b, 0, st, flat, flat_bytes, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd, m);
    } else {
        if (nv12) hipLaunchKernelGGL((resize_pack_yuv_kernel<float, true>), g, b, 0, st, flat, flat_bytes, table, (float*)dst, S, Hp, Wp, pad, mean, istd, m);
        else hipLaunchKernelGGL((resize_pack_yuv_kernel<float, false>), g, b, 0, st, flat, flat_bytes, table, (float*)dst, S, Hp, Wp, pad, mean, istd, m);
    }
    return cb_launch_status("cb_resize_pack_yuv420");
}

extern "C" int cb_resize_pack_u8_src(int32_t dtype, const cb_frame_source* src, const int64_t* table, int32_t N, int32_t hwc, const float* mean3,
                                     const float* std3, void* dst, int32_t S, int32_t Hp, int32_t Wp, int32_t pad, void* stream) {
    if (resize_pack_check_src("cb_resize_pack_u8_src", src, table, N, mean3, std3, dst, S, Hp, Wp, pad)) return -1;
    f32x4 mean = {mean3[0], mean3[1], mean3[2], 0.f}, istd = {1.0f / std3[0], 1.0f / std3[1], 1.0f / std3[2], 1.f};
    dim3 g((unsigned)(((int64_t)Hp * Wp + 255) / 256), (unsigned)N), b(256);
    hipStream_t st = cb_stream(stream);
    if (dtype == CB_BF16) {
        if (hwc) hipLaunchKernelGGL((resize_pack_src_kernel<bf16, true>), g, b, 0, st, src, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd);
        else hipLaunchKernelGGL((resize_pack_src_kernel<bf16, false>), g, b, 0, st, src, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd);
    } else if (dtype == CB_F32) {
        if (hwc) hipLaunchKernelGGL((resize_pack_src_kernel<float, true>), g, b, 0, st, src, table, (float*)dst, S, Hp, Wp, pad, mean, istd);
        else hipLaunchKernelGGL((resize_pack_src_kernel<float, false>), g, b, 0, st, src, table, (float*)dst, S, Hp, Wp, pad, mean, istd);
    } else return cb_fail("cb_resize_pack_u8_src: bad dtype");
    return cb_launch_status("cb_resize_pack_u8_src");
}

extern "C" int cb_resize_pack_yuv420_src(int32_t dtype, const cb_frame_source* src, const int64_t* table, int32_t N, int32_t layout, int32_t matrix,
                                         const float* mean3, const float* std3, void* dst, int32_t S, int32_t Hp, int32_t Wp, int32_t pad, void* stream) {
    CB_REQUIRE(dtype == CB_BF16 || dtype == CB_F32, "cb_resize_pack_yuv420_src: bad dtype");
    CB_REQUIRE(layout == CB_YUV_I420 || layout == CB_YUV_NV12, "cb_resize_pack_yuv420_src: bad layout %d (CB_YUV_I420, CB_YUV_NV12)", layout);
    CB_REQUIRE(matrix >= CB_YUV_BT601 && matrix <= CB_YUV_BT709_FULL, "cb_resize_pack_yuv420_src: bad matrix %d (CB_YUV_BT601 .. CB_YUV_BT709_FULL)", matrix);
    if (resize_pack_check_src("cb_resize_pack_yuv420_src", src, table, N, mean3, std3, dst, S, Hp, Wp, pad)) return -1;
    f32x4 mean = {mean3[0], mean3[1], mean3[2], 0.f}, istd = {1.0f / std3[0], 1.0f / std3[1], 1.0f / std3[2], 1.f};
    dim3 g((unsigned)(((int64_t)Hp * Wp + 255) / 256), (unsigned)N), b(256);
    hipStream_t st = cb_stream(stream);
    const YuvMatrix m = yuv_matrix[matrix];
    const bool nv12 = layout == CB_YUV_NV12;
    if (dtype == CB_BF16) {
        if (nv12) hipLaunchKernelGGL((resize_pack_yuv_src_kernel<bf16, true>), g, b, 0, st, src, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd, m);
        else hipLaunchKernelGGL((resize_pack_yuv_src_kernel<bf16, false>), g, b, 0, st, src, table, (bf16*)dst, S, Hp, Wp, pad, mean, istd, m);
    } else {
        if (nv12) hipLaunchKernelGGL((resize_pack_yuv_src_kernel<float, true>), g, b, 0, st, src, table, (float*)dst, S, Hp, Wp, pad, mean, istd, m);
        else hipLaunchKernelGGL((resize_pack_yuv_src_kernel<float, false>), g, b, 0, st, src, table, (float*)dst, S, Hp, Wp, pad, mean, istd, m);
    }
    return cb_launch_status("cb_resize_pack_yuv420_src");
}
