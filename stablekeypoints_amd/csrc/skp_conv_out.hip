// 3x3 / stride 1 / padding 1 convolution to AT MOST FOUR output channels: the `conv_out` of the VAE decoder (128 -> 3 at the image
// resolution, reached from ptp_utils.py `latent2image`) -- the mirror of skp_conv_in.hip.  With M = Cout <= 4 a matrix
// instruction would idle 12 of its 16 rows, and the layer is small (128 -> 3 at 512^2 is 1.8 GF), so this is a plain VALU kernel:
//   thread = two horizontally adjacent output pixels, Cout packed accumulators; per input channel the 3 x 4 patch is loaded
//   (zero padding by predication: one 8-byte load and two edge loads per row) and multiplied by the channel's 9 * Cout
//   weights, which are wave-uniform (scalar loads, one SGPR operand per packed fma).
// Optional image epilogue: clamp(y / 2 + 0.5, 0, 1), the [-1, 1] -> [0, 1] map of `latent2image`.  NCHW in and out, bias folded in.
// Also here, the rest of the decoder's way out to the image:
//   skp_image_u8_nhwc_f32   float [B,3,H,W] in [0, 1] -> uint8 [B,H,W,3], so that what crosses to the host is bytes.  16-byte loads
//                           where the plane size and the pointers allow, a scalar form otherwise, the grid capped at 2048 workgroups
//                           with a grid-stride loop.
#include "skp_common.h"

namespace {

template <int CO>
__global__ __launch_bounds__(256) void skp_conv_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, int Ci, int H,
                                                           int W, int image) {
    const int W2 = W >> 1;
    const int pi = blockIdx.x * 256 + threadIdx.x;
    if (pi >= H * W2) return;
    const int b = blockIdx.y;
    const int yy = pi / W2, x0 = 2 * (pi - yy * W2);
    const size_t plane = (size_t)H * W;
    const float* xb = x + (size_t)b * Ci * plane;
    bool rin[3];
    size_t roff[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int iy = yy + r - 1;
        rin[r] = iy >= 0 && iy < H;
        roff[r] = (size_t)(rin[r] ? iy : 0) * W + x0;
    }
    const bool lin = x0 > 0, rtin = x0 + 2 < W;
    f32x2 acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) {
        const float bv = bias ? bias[co] : 0.f;
        acc[co] = f32x2{bv, bv};
    }
#pragma unroll 4
    for (int ci = 0; ci < Ci; ++ci) {
        const float* xc = xb + (size_t)ci * plane;
        f32x2 p[3][3];                                              // {col j, col j + 1} pairs for the three taps of a row
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* row = xc + roff[r];
            const f32x2 mid = rin[r] ? *(const f32x2*)row : f32x2{0.f, 0.f};
            const float lf = (rin[r] && lin) ? row[-1] : 0.f;
            const float rt = (rin[r] && rtin) ? row[2] : 0.f;
            p[r][0] = f32x2{lf, mid[0]};
            p[r][1] = mid;
            p[r][2] = f32x2{mid[1], rt};
        }
#pragma unroll
        for (int co = 0; co < CO; ++co) {
            const float* wc = w + ((size_t)co * Ci + ci) * 9;       // uniform: scalar loads
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float wv = wc[r * 3 + c];
                    acc[co] = f32x2{wv, wv} * p[r][c] + acc[co];
                }
        }
    }
    float* yb = y + (size_t)b * CO * plane + (size_t)yy * W + x0;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
        f32x2 v = acc[co];
        if (image) {
            v[0] = fminf(fmaxf(v[0] * 0.5f + 0.5f, 0.f), 1.f);
            v[1] = fminf(fmaxf(v[1] * 0.5f + 0.5f, 0.f), 1.f);
        }
        *(f32x2*)(yb + (size_t)co * plane) = v;
    }
}

// One lane = four horizontally consecutive pixels of one image: three 16-byte loads (one per channel plane), twelve bytes out as
// three dwords.  Needs H * W % 4 == 0 (every plane then starts 16-byte aligned, every group of four pixels 4-byte aligned in y).
__device__ __forceinline__ unsigned u8_of(float v) { return (unsigned)(int)(v * 255.0f) & 0xffu; }

__global__ __launch_bounds__(SKP_EW_BLOCK) void skp_image_u8_vec_kernel(const float* __restrict__ x, unsigned* __restrict__ y,
                                                                        long long plane4, long long total) {
    const long long stride = (long long)gridDim.x * SKP_EW_BLOCK;
    for (long long i = (long long)blockIdx.x * SKP_EW_BLOCK + threadIdx.x; i < total; i += stride) {
        const long long b = i / plane4, q = i - b * plane4;
        const f32x4* xb = (const f32x4*)x + b * 3 * plane4 + q;
        const f32x4 r = xb[0], g = xb[plane4], bl = xb[2 * plane4];
        unsigned px[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[3 * k] = u8_of(r[k]);
            px[3 * k + 1] = u8_of(g[k]);
            px[3 * k + 2] = u8_of(bl[k]);
        }
        unsigned* yo = y + i * 3;
#pragma unroll
        for (int w = 0; w < 3; ++w) yo[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | (px[4 * w + 3] << 24);
    }
}

// Any H, W: one lane = one pixel, three byte stores.
__global__ __launch_bounds__(SKP_EW_BLOCK) void skp_image_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ y,
                                                                    long long plane, long long total) {
    const long long stride = (long long)gridDim.x * SKP_EW_BLOCK;
    for (long long i = (long long)blockIdx.x * SKP_EW_BLOCK + threadIdx.x; i < total; i += stride) {
        const long long b = i / plane, p = i - b * plane;
        const float* xb = x + b * 3 * plane + p;
        unsigned char* yo = y + i * 3;
        yo[0] = (unsigned char)u8_of(xb[0]);
        yo[1] = (unsigned char)u8_of(xb[plane]);
        yo[2] = (unsigned char)u8_of(xb[2 * plane]);
    }
}

}  // namespace

extern "C" int skp_conv3x3_small_out_f32(const void* x, const void* w, const void* bias, void* y, int B, int Cin, int Cout, int H,
                                         int W, int image, void* stream) {
    if (!x || !w || !y || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return SKP_E_BADARG;
    if ((Cin & 15) || Cout > 4 || (W & 1) || B > 65535 || (long)H * W / 2 > (1L << 30)) return SKP_E_RANGE;
    dim3 grid((unsigned)(((long)H * (W / 2) + 255) / 256), B, 1), block(256);
    hipStream_t st = (hipStream_t)stream;
#define SKP_COUT(CO) \
    hipLaunchKernelGGL(skp_conv_out_kernel<CO>, grid, block, 0, st, (const float*)x, (const float*)w, (const float*)bias, (float*)y, Cin, H, W, image ? 1 : 0)
    switch (Cout) {
        case 1: SKP_COUT(1); break;
        case 2: SKP_COUT(2); break;
        case 3: SKP_COUT(3); break;
        default: SKP_COUT(4); break;
    }
#undef SKP_COUT
    return skp_launch_status();
}

extern "C" int skp_image_u8_nhwc_f32(const float* x, unsigned char* y, int B, int H, int W, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0) return SKP_E_BADARG;
    const long long plane = (long long)H * W, total = plane * B;
    hipStream_t st = (hipStream_t)stream;
    if ((plane & 3) == 0 && skp_aligned16(x) && ((uintptr_t)y & 3) == 0) {
        hipLaunchKernelGGL(skp_image_u8_vec_kernel, dim3(skp_capped_grid(total / 4)), dim3(SKP_EW_BLOCK), 0, st, x, (unsigned*)y,
                           plane / 4, total / 4);
    } else {
        hipLaunchKernelGGL(skp_image_u8_kernel, dim3(skp_capped_grid(total)), dim3(SKP_EW_BLOCK), 0, st, x, y, plane, total);
    }
    return skp_launch_status();
}
