// The step of the image-sampling loop for the samplers of ldm/samplers.py (stochastic DDIM, DPM-Solver++(2M), SDE-DPM-Solver++(2M)):
//   skp_sampler_step_f32    classifier-free guidance mix + (x0, eps) for epsilon / v / sample prediction + the optional x0 clamp +
//                           y = cx x + c0 x0 + ce eps + c1 x0_prev + cn noise in one pass; y may be written twice (the duplicated
//                           UNet input of the next guided step) and the clamped x0 is kept for the next step's x0_prev.
// Built like skp_ddim_step.hip: memory-bound and tiny (a latent is 16 K floats), 16-byte accesses where pointers and counts allow, a
// scalar form otherwise, the grid capped at 2048 workgroups with a grid-stride loop.  Every output element is computed by the lane
// that read its inputs, after reading them, which is what makes y == x and x0_out == x0_prev legal.
#include "skp_common.h"

namespace {

constexpr int SAMP_BLOCK = 256;
constexpr long long SAMP_MAX_BLOCKS = 2048;

struct SamplerCoef {
    float g, sa, sb, cx, c0, ce, c1, cn;
    int prediction, clip;
};

// -> y; x0 (after the clamp) through `x0c`.  `p` / `nz` are 0 where x0_prev / noise are absent (their coefficients are 0 then).
template <bool GUIDED>
__device__ __forceinline__ float sampler_one(float x, float mc, float mu, float p, float nz, const SamplerCoef& c, float& x0c) {
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
    x0c = x0;
    return c.cx * x + c.c0 * x0 + c.ce * eps + c.c1 * p + c.cn * nz;
}

// VEC: every pointer given is 16-byte aligned; groups of four elements per lane, the n % 4 tail by the first lanes of workgroup 0.
// Y2VEC: the second copy y + n is 16-byte aligned too (n % 4 == 0); otherwise it is written with scalar stores.
// x / y and x0_prev / x0_out carry no __restrict__: each pair may be one buffer.  x0_prev, noise and x0_out may be null.
template <bool GUIDED, bool VEC, bool Y2VEC>
__global__ __launch_bounds__(SAMP_BLOCK) void skp_sampler_step_kernel(const float* x, const float* __restrict__ mc,
                                                                      const float* __restrict__ mu, const float* x0_prev,
                                                                      const float* __restrict__ noise, float* y, float* x0_out,
                                                                      long long n, int copies, SamplerCoef c) {
    const long long tid = (long long)blockIdx.x * SAMP_BLOCK + threadIdx.x;
    const long long stride = (long long)gridDim.x * SAMP_BLOCK;
    float* y2 = copies == 2 ? y + n : nullptr;
    if (VEC) {
        const long long n4 = n >> 2;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (long long i = tid; i < n4; i += stride) {
            const f32x4 xv = ((const f32x4*)x)[i];
            const f32x4 cv = ((const f32x4*)mc)[i];
            const f32x4 uv = GUIDED ? ((const f32x4*)mu)[i] : cv;
            const f32x4 pv = x0_prev ? ((const f32x4*)x0_prev)[i] : zero;
            const f32x4 nv = noise ? ((const f32x4*)noise)[i] : zero;
            f32x4 r, z;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x0c;
                r[k] = sampler_one<GUIDED>(xv[k], cv[k], uv[k], pv[k], nv[k], c, x0c);
                z[k] = x0c;
            }
            ((f32x4*)y)[i] = r;
            if (y2) {
                if (Y2VEC) {
                    ((f32x4*)y2)[i] = r;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) y2[4 * i + k] = r[k];
                }
            }
            if (x0_out) ((f32x4*)x0_out)[i] = z;
        }
        const long long t = (n4 << 2) + tid;                        // tail: at most three elements
        if (tid < 4 && t < n) {
            float x0c;
            const float r = sampler_one<GUIDED>(x[t], mc[t], GUIDED ? mu[t] : 0.f, x0_prev ? x0_prev[t] : 0.f,
                                                noise ? noise[t] : 0.f, c, x0c);
            y[t] = r;
            if (y2) y2[t] = r;
            if (x0_out) x0_out[t] = x0c;
        }
    } else {
        for (long long i = tid; i < n; i += stride) {
            float x0c;
            const float r = sampler_one<GUIDED>(x[i], mc[i], GUIDED ? mu[i] : 0.f, x0_prev ? x0_prev[i] : 0.f,
                                                noise ? noise[i] : 0.f, c, x0c);
            y[i] = r;
            if (y2) y2[i] = r;
            if (x0_out) x0_out[i] = x0c;
        }
    }
}

inline unsigned capped_grid(long long items) {
    const long long blocks = (items + SAMP_BLOCK - 1) / SAMP_BLOCK;
    return (unsigned)(blocks < 1 ? 1 : (blocks > SAMP_MAX_BLOCKS ? SAMP_MAX_BLOCKS : blocks));
}

inline bool aligned16_or_null(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int skp_sampler_step_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise,
                                    float* y, float* x0_out, int64_t n, int copies, float guidance, int prediction, float sa,
                                    float sb, float cx, float c0, float ce, float c1, float cn, int clip, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if ((c1 != 0.f && !x0_prev) || (cn != 0.f && !noise)) return SKP_E_BADARG;
    if (c1 == 0.f) x0_prev = nullptr;                               // not read: a buffer that holds no x0 yet may be anything, NaN included
    if (cn == 0.f) noise = nullptr;
    const SamplerCoef c{guidance, sa, sb, cx, c0, ce, c1, cn, prediction, clip ? 1 : 0};
    const bool vec = aligned16_or_null(x) && aligned16_or_null(m_c) && aligned16_or_null(m_u) && aligned16_or_null(x0_prev) &&
                     aligned16_or_null(noise) && aligned16_or_null(y) && aligned16_or_null(x0_out) && n >= 4;
    const bool y2vec = (n & 3) == 0;
    const dim3 grid(capped_grid(vec ? n / 4 : n)), block(SAMP_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define SKP_SAMP(G, V, Y2)                                                                                                    \
    hipLaunchKernelGGL((skp_sampler_step_kernel<G, V, Y2>), grid, block, 0, st, x, m_c, m_u, x0_prev, noise, y, x0_out, (long long)n, \
                       copies, c)
    if (m_u) {
        if (!vec) SKP_SAMP(true, false, false);
        else if (y2vec) SKP_SAMP(true, true, true);
        else SKP_SAMP(true, true, false);
    } else {
        if (!vec) SKP_SAMP(false, false, false);
        else if (y2vec) SKP_SAMP(false, true, true);
        else SKP_SAMP(false, true, false);
    }
#undef SKP_SAMP
    return skp_launch_status();
}
