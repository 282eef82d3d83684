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

// dst (N, Hp, Wp, 4), channels B, G, R, 0.  Pixel (hp, wp) -> image position (y, x) = (hp - pad, wp - pad):
//   inside new_h x new_w : the bilinear sample, normalised
//   inside S x S         : the zero PIXEL ImagePad appends, normalised -- (0 - mean) * (1 / std): the reference pads before it normalises
//   elsewhere            : zeros (the convolution's halo), as cb_stem_pack writes
// A table row that does not describe a frame inside the buffer makes its frame all padding; nothing is read through it.
template <typename T, bool HWC>
__global__ void __launch_bounds__(256) resize_pack_kernel(const uint8_t* flat, int64_t flat_bytes, const int64_t* table, T* dst, int S, int Hp,
                                                          int Wp, int pad, f32x4 mean, f32x4 istd) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= Hp * Wp) return;
    const int y = pix / Wp - pad, x = pix % Wp - pad;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S) {
        const int64_t* row = table + (int64_t)n * 5;
        const int64_t off = row[0], h64 = row[1], w64 = row[2], nh64 = row[3], nw64 = row[4];
        const bool ok = off >= 0 && h64 >= 1 && w64 >= 1 && h64 <= MAX_SIDE && w64 <= MAX_SIDE && nh64 >= 1 && nw64 >= 1 && nh64 <= S && nw64 <= S &&
                        off <= flat_bytes && 3 * h64 * w64 <= flat_bytes - off;
        float rgb[3] = {0.f, 0.f, 0.f};
        if (ok && y < (int)nh64 && x < (int)nw64) {
            const int h = (int)h64, w = (int)w64;
            const Axis ay = axis_taps(y, h, (int)nh64), ax = axis_taps(x, w, (int)nw64);
            const uint8_t* f = flat + off;
            const int64_t cs = HWC ? 1 : (int64_t)h * w, ps = HWC ? 3 : 1;       // channel / pixel strides in bytes
            const int64_t r0 = (int64_t)ay.i0 * w, r1 = (int64_t)ay.i1 * w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* fc = f + c * cs;
                const float p00 = (float)fc[(r0 + ax.i0) * ps], p01 = (float)fc[(r0 + ax.i1) * ps];
                const float p10 = (float)fc[(r1 + ax.i0) * ps], p11 = (float)fc[(r1 + ax.i1) * ps];
                // l0 * a + l1 * b as fma(l0, a, l1 * b), x first, then y: the operation order of PyTorch's CPU kernel built with FMA
                // (bit-identical to F.interpolate on most shapes, <= 2 fp32 ulp at 255 otherwise); exact for l1 = 0
                const float top = __builtin_fmaf(ax.l0, p00, ax.l1 * p01), bot = __builtin_fmaf(ax.l0, p10, ax.l1 * p11);
                rgb[c] = __builtin_fmaf(ay.l0, top, ay.l1 * bot);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (rgb[2 - c] - mean[2 - c]) * istd[2 - c];
    }
    store4(dst + ((int64_t)n * Hp * Wp + pix) * 4, v);
}

}  // namespace

extern "C" int cb_resize_pack_u8(int32_t dtype, const uint8_t* flat, int64_t flat_bytes, const int64_t* table, const int64_t* table_host,
                                 int32_t N, int32_t hwc, const float* mean3, const float* std3, void* dst, int32_t S, int32_t Hp, int32_t Wp,
                                 int32_t pad, void* stream) {
    CB_REQUIRE(flat && table && dst && mean3 && std3, "cb_resize_pack_u8: null operand");
    CB_REQUIRE(N > 0 && N <= 65535 && S >= 1 && pad >= 0 && flat_bytes > 0, "cb_resize_pack_u8: bad N / S / pad / buffer size (%d, %d, %d, %lld)", N, S, pad,
               (long long)flat_bytes);
    CB_REQUIRE(Hp >= S + 2 * pad && Wp >= S + 2 * pad && (int64_t)Hp * Wp < (1ll << 30), "cb_resize_pack_u8: packed image %d x %d does not hold %d + 2 x %d", Hp, Wp, S, pad);
    CB_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(table) & 7) == 0, "cb_resize_pack_u8: dst / table alignment");
    for (int i = 0; table_host && i < N; ++i) {
        const int64_t* r = table_host + (int64_t)i * 5;
        CB_REQUIRE(r[1] >= 1 && r[2] >= 1 && r[1] <= MAX_SIDE && r[2] <= MAX_SIDE, "cb_resize_pack_u8: frame %d is %lld x %lld", i, (long long)r[1], (long long)r[2]);
        CB_REQUIRE(r[3] >= 1 && r[4] >= 1 && r[3] <= S && r[4] <= S, "cb_resize_pack_u8: frame %d resizes to %lld x %lld, outside 1..%d", i, (long long)r[3],
                   (long long)r[4], S);
        CB_REQUIRE(r[0] >= 0 && r[0] <= flat_bytes && 3 * r[1] * r[2] <= flat_bytes - r[0], "cb_resize_pack_u8: frame %d (offset %lld, %lld x %lld x 3) leaves the %lld-byte buffer",
                   i, (long long)r[0], (long long)r[1], (long long)r[2], (long long)flat_bytes);
    }
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
