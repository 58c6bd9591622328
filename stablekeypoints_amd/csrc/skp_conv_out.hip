// 3x3 / stride 1 / padding 1 convolution to AT MOST FOUR output channels: the `conv_out` of the VAE decoder (128 -> 3 at the image
// resolution, reached from ptp_utils.py `latent2image`) -- the mirror of skp_conv_in.hip.  With M = Cout <= 4 a matrix
// instruction would idle 12 of its 16 rows, and the layer is small (128 -> 3 at 512^2 is 1.8 GF), so this is a plain VALU kernel:
//   thread = two horizontally adjacent output pixels, Cout packed accumulators; per input channel the 3 x 4 patch is loaded
//   (zero padding by predication: one 8-byte load and two edge loads per row) and multiplied by the channel's 9 * Cout
//   weights, which are wave-uniform (scalar loads, one SGPR operand per packed fma).
// Optional image epilogue: clamp(y / 2 + 0.5, 0, 1), the [-1, 1] -> [0, 1] map of `latent2image`.  NCHW in and out, bias folded in.
// Also here: the DDIM update of the sampling loop, x_prev = c1 x + c2 eps with host-computed coefficients.
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

__global__ __launch_bounds__(256) void skp_axpby_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                        float* __restrict__ y, long long n, float ca, float cb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = ca * x[i] + cb * z[i];
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

// y[i] = a * x[i] + b * z[i], i < n (y may be x or z).  The eta = 0 DDIM update with clip_sample off is exactly this.
extern "C" int skp_axpby_f32(const void* x, const void* z, void* y, int64_t n, float a, float b, void* stream) {
    if (!x || !z || !y || n <= 0) return SKP_E_BADARG;
    if (n > (int64_t)0x7fffffff * 256) return SKP_E_RANGE;
    hipLaunchKernelGGL(skp_axpby_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)z, (float*)y, (long long)n, a, b);
    return skp_launch_status();
}
