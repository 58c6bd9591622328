// The elementwise ends of the image-sampling loop (ptp_utils.py `text2image_ldm_stable`):
//   skp_ddim_step_f32       classifier-free guidance mix + the eta = 0 DDIM update for epsilon / v / sample prediction, with the
//                           optional x0 clamp, in one pass; the result may be written twice (the duplicated UNet input of the next
//                           guided step, so the loop needs no concatenation);
//   skp_image_u8_nhwc_f32   float [B,3,H,W] in [0, 1] -> uint8 [B,H,W,3], so that what crosses to the host is bytes.
// Both are memory-bound and tiny (a latent is 16 K floats): 16-byte accesses where pointers and counts allow, a scalar form
// otherwise, the grid capped at 2048 workgroups with a grid-stride loop.  Every output element is computed by the lane that read its
// inputs, after reading them, which is what makes y == x legal.
#include "skp_common.h"

namespace {

constexpr int DDIM_BLOCK = 256;
constexpr long long DDIM_MAX_BLOCKS = 2048;

struct DdimCoef {
    float g, sa, sb, pa, pb;
    int prediction, clip;
};

template <bool GUIDED>
__device__ __forceinline__ float ddim_one(float x, float mc, float mu, const DdimCoef& c) {
    const float m = GUIDED ? mu + c.g * (mc - mu) : mc;
    float x0, eps;
    if (c.prediction == 0) {
        x0 = (x - c.sb * m) / c.sa;
        eps = m;
    } else if (c.prediction == 1) {
        x0 = c.sa * x - c.sb * m;
        eps = c.sa * m + c.sb * x;
    } else {
        x0 = m;
        eps = (x - c.sa * m) / c.sb;
    }
    if (c.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    return c.pa * x0 + c.pb * eps;
}

// VEC: x, m_c, m_u, y are 16-byte aligned; groups of four elements per lane, the n % 4 tail by the first lanes of workgroup 0.
// Y2VEC: the second copy y + n is 16-byte aligned too (n % 4 == 0); otherwise it is written with scalar stores.
// x and y carry no __restrict__: they may be the same buffer.
template <bool GUIDED, bool VEC, bool Y2VEC>
__global__ __launch_bounds__(DDIM_BLOCK) void skp_ddim_step_kernel(const float* x, const float* __restrict__ mc,
                                                                   const float* __restrict__ mu, float* y, long long n, int copies,
                                                                   DdimCoef c) {
    const long long tid = (long long)blockIdx.x * DDIM_BLOCK + threadIdx.x;
    const long long stride = (long long)gridDim.x * DDIM_BLOCK;
    float* y2 = copies == 2 ? y + n : nullptr;
    if (VEC) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += stride) {
            const f32x4 xv = ((const f32x4*)x)[i];
            const f32x4 cv = ((const f32x4*)mc)[i];
            const f32x4 uv = GUIDED ? ((const f32x4*)mu)[i] : cv;
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = ddim_one<GUIDED>(xv[k], cv[k], uv[k], c);
            ((f32x4*)y)[i] = r;
            if (y2) {
                if (Y2VEC) {
                    ((f32x4*)y2)[i] = r;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) y2[4 * i + k] = r[k];
                }
            }
        }
        const long long t = (n4 << 2) + tid;                        // tail: at most three elements
        if (tid < 4 && t < n) {
            const float r = ddim_one<GUIDED>(x[t], mc[t], GUIDED ? mu[t] : 0.f, c);
            y[t] = r;
            if (y2) y2[t] = r;
        }
    } else {
        for (long long i = tid; i < n; i += stride) {
            const float r = ddim_one<GUIDED>(x[i], mc[i], GUIDED ? mu[i] : 0.f, c);
            y[i] = r;
            if (y2) y2[i] = r;
        }
    }
}

// One lane = four horizontally consecutive pixels of one image: three 16-byte loads (one per channel plane), twelve bytes out as
// three dwords.  Needs H * W % 4 == 0 (every plane then starts 16-byte aligned, every group of four pixels 4-byte aligned in y).
__device__ __forceinline__ unsigned u8_of(float v) { return (unsigned)(int)(v * 255.0f) & 0xffu; }

__global__ __launch_bounds__(DDIM_BLOCK) void skp_image_u8_vec_kernel(const float* __restrict__ x, unsigned* __restrict__ y,
                                                                      long long plane4, long long total) {
    const long long stride = (long long)gridDim.x * DDIM_BLOCK;
    for (long long i = (long long)blockIdx.x * DDIM_BLOCK + threadIdx.x; i < total; i += stride) {
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
__global__ __launch_bounds__(DDIM_BLOCK) void skp_image_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ y,
                                                                  long long plane, long long total) {
    const long long stride = (long long)gridDim.x * DDIM_BLOCK;
    for (long long i = (long long)blockIdx.x * DDIM_BLOCK + threadIdx.x; i < total; i += stride) {
        const long long b = i / plane, p = i - b * plane;
        const float* xb = x + b * 3 * plane + p;
        unsigned char* yo = y + i * 3;
        yo[0] = (unsigned char)u8_of(xb[0]);
        yo[1] = (unsigned char)u8_of(xb[plane]);
        yo[2] = (unsigned char)u8_of(xb[2 * plane]);
    }
}

inline unsigned capped_grid(long long items) {
    const long long blocks = (items + DDIM_BLOCK - 1) / DDIM_BLOCK;
    return (unsigned)(blocks < 1 ? 1 : (blocks > DDIM_MAX_BLOCKS ? DDIM_MAX_BLOCKS : blocks));
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int skp_ddim_step_f32(const float* x, const float* m_c, const float* m_u, float* y, int64_t n, int copies, float guidance,
                                 int prediction, float sa, float sb, float pa, float pb, int clip, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    const DdimCoef c{guidance, sa, sb, pa, pb, prediction, clip ? 1 : 0};
    const bool vec = aligned16(x) && aligned16(m_c) && aligned16(y) && (!m_u || aligned16(m_u)) && n >= 4;
    const bool y2vec = (n & 3) == 0;
    const dim3 grid(capped_grid(vec ? n / 4 : n)), block(DDIM_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define SKP_DDIM(G, V, Y2) \
    hipLaunchKernelGGL((skp_ddim_step_kernel<G, V, Y2>), grid, block, 0, st, x, m_c, m_u, y, (long long)n, copies, c)
    if (m_u) {
        if (!vec) SKP_DDIM(true, false, false);
        else if (y2vec) SKP_DDIM(true, true, true);
        else SKP_DDIM(true, true, false);
    } else {
        if (!vec) SKP_DDIM(false, false, false);
        else if (y2vec) SKP_DDIM(false, true, true);
        else SKP_DDIM(false, true, false);
    }
#undef SKP_DDIM
    return skp_launch_status();
}

extern "C" int skp_image_u8_nhwc_f32(const float* x, unsigned char* y, int B, int H, int W, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0) return SKP_E_BADARG;
    const long long plane = (long long)H * W, total = plane * B;
    hipStream_t st = (hipStream_t)stream;
    if ((plane & 3) == 0 && aligned16(x) && ((uintptr_t)y & 3) == 0) {
        hipLaunchKernelGGL(skp_image_u8_vec_kernel, dim3(capped_grid(total / 4)), dim3(DDIM_BLOCK), 0, st, x, (unsigned*)y, plane / 4,
                           total / 4);
    } else {
        hipLaunchKernelGGL(skp_image_u8_kernel, dim3(capped_grid(total)), dim3(DDIM_BLOCK), 0, st, x, y, plane, total);
    }
    return skp_launch_status();
}
