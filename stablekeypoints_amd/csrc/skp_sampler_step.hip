// The step of the image-sampling loop (ptp_utils.py `text2image_ldm_stable`), one kernel behind two entries:
//   skp_ddim_step_f32       classifier-free guidance mix + (x0, eps) for epsilon / v / sample prediction + the optional x0 clamp +
//                           the eta = 0 DDIM update y = pa x0 + pb eps (ldm/scheduler.py `DDIMScheduler.step`);
//   skp_sampler_step_f32    the same up to the clamp, then y = cx x + c0 x0 + ce eps + c1 x0_prev + cn noise for the samplers of
//                           ldm/samplers.py (stochastic DDIM, DPM-Solver++(2M), SDE-DPM-Solver++(2M)); the clamped x0 is kept for
//                           the next step's x0_prev;
//   skp_sampler_step_kp_f32 the sampler form with the gradient term of keypoint guidance: between deriving (x0, eps) and the clamp,
//                           eps += s g and x0 -= (sb / sa) s g, s = gs[row of the element] read from device memory.
// Either may write y twice (the duplicated UNet input of the next guided step, so the loop needs no concatenation).
// Memory-bound and tiny (a latent is 16 K floats): 16-byte accesses where pointers and counts allow, a scalar form otherwise, the grid
// capped at 2048 workgroups with a grid-stride loop.  Every output element is computed by the lane that read its inputs, after
// reading them, which is what makes y == x and x0_out == x0_prev legal.
// Also here: skp_axpby_f32, the plain unguided epsilon form of the DDIM update, x_prev = c1 x + c2 eps with host-computed coefficients.
// Device-row forms (include/skp_sampler_graph.h; the captured sampling loop): the same kernel body behind a second __global__ that
// first reads this step's StepCoef from row *step of a table in device memory, where the by-value kernel receives it as an
// argument.  `step_one` and the loop around it are shared, so equal floats give equal bits.  skp_step_advance moves the counter.
#include "skp_common.h"
#include "../../include/skp_sampler_graph.h"

namespace {

struct StepCoef {
    float g, sa, sb, cx, c0, ce, c1, cn;                            // cx, c1, cn: FULL only
    float kr;                                                       // sb / sa (KP only)
    int prediction, clip;
};

// What only the FULL (sampler) form takes, each may be null; the DDIM form carries no such arguments.  kg / kgs / per: the guidance
// gradient, its per-row scales and the elements per row (KP only).
template <bool FULL>
struct StepExtra {
    const float *x0_prev, *noise;
    float* x0_out;
    const float *kg, *kgs;
    long long per;
};
template <>
struct StepExtra<false> {
    static constexpr const float *x0_prev = nullptr, *noise = nullptr;
    static constexpr float* x0_out = nullptr;
    static constexpr const float *kg = nullptr, *kgs = nullptr;
    static constexpr long long per = 1;
};

// -> y; x0 (after the clamp) through `x0c`.  `p` / `nz` are 0 where x0_prev / noise are absent (their coefficients are 0 then).
// The DDIM form is an expression of its own, not the five terms with zeros: the two contract into different fused multiply-adds.
// KP: `sg` = s g of this element, the shift of eps; x0 moves by -(sb / sa) of it, so that sa x0 + sb eps stays x.
template <bool GUIDED, bool FULL, bool KP = false>
__device__ __forceinline__ float step_one(float x, float mc, float mu, float p, float nz, const StepCoef& c, float& x0c, float sg = 0.f) {
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
    if (KP) {
        eps += sg;
        x0 -= c.kr * sg;
    }
    if (c.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    x0c = x0;
    if (FULL) return c.cx * x + c.c0 * x0 + c.ce * eps + c.c1 * p + c.cn * nz;
    return c.c0 * x0 + c.ce * eps;
}

// VEC: every pointer given is 16-byte aligned; groups of four elements per lane, the n % 4 tail by the first lanes of workgroup 0.
// Y2VEC: the second copy y + n is 16-byte aligned too (n % 4 == 0); otherwise it is written with scalar stores.
// x / y and x0_prev / x0_out carry no __restrict__: each pair may be one buffer.
template <bool GUIDED, bool VEC, bool Y2VEC, bool FULL, bool KP = false>
__device__ __forceinline__ void step_body(const float* x, const float* __restrict__ mc, const float* __restrict__ mu,
                                          const StepExtra<FULL>& e, float* y, long long n, int copies, const StepCoef& c) {
    const long long tid = (long long)blockIdx.x * SKP_EW_BLOCK + threadIdx.x;
    const long long stride = (long long)gridDim.x * SKP_EW_BLOCK;
    float* y2 = copies == 2 ? y + n : nullptr;
    const float* x0_prev = e.x0_prev;
    const float* __restrict__ noise = e.noise;
    float* x0_out = e.x0_out;
    const float* __restrict__ kg = e.kg;
    const float* __restrict__ kgs = e.kgs;
    if (VEC) {
        const long long n4 = n >> 2;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (long long i = tid; i < n4; i += stride) {
            const f32x4 xv = ((const f32x4*)x)[i];
            const f32x4 cv = ((const f32x4*)mc)[i];
            const f32x4 uv = GUIDED ? ((const f32x4*)mu)[i] : cv;
            const f32x4 pv = x0_prev ? ((const f32x4*)x0_prev)[i] : zero;
            const f32x4 nv = noise ? ((const f32x4*)noise)[i] : zero;
            const f32x4 gv = KP ? ((const f32x4*)kg)[i] : zero;
            f32x4 r, z;
            // the row of the group's first element, by one division; later elements step over a row's end (several, if rows are
            // shorter than a group) and reload the scale only there
            long long row = KP ? (4 * i) / e.per : 0;
            long long at = KP ? 4 * i - row * e.per : 0;
            float s = KP ? kgs[row] : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x0c;
                if (KP) {
                    while (at >= e.per) {
                        at -= e.per;
                        s = kgs[++row];
                    }
                    ++at;
                }
                r[k] = step_one<GUIDED, FULL, KP>(xv[k], cv[k], uv[k], pv[k], nv[k], c, x0c, s * gv[k]);
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
            const float r = step_one<GUIDED, FULL, KP>(x[t], mc[t], GUIDED ? mu[t] : 0.f, x0_prev ? x0_prev[t] : 0.f,
                                                       noise ? noise[t] : 0.f, c, x0c, KP ? kgs[t / e.per] * kg[t] : 0.f);
            y[t] = r;
            if (y2) y2[t] = r;
            if (x0_out) x0_out[t] = x0c;
        }
    } else {
        for (long long i = tid; i < n; i += stride) {
            float x0c;
            const float r = step_one<GUIDED, FULL, KP>(x[i], mc[i], GUIDED ? mu[i] : 0.f, x0_prev ? x0_prev[i] : 0.f,
                                                       noise ? noise[i] : 0.f, c, x0c, KP ? kgs[i / e.per] * kg[i] : 0.f);
            y[i] = r;
            if (y2) y2[i] = r;
            if (x0_out) x0_out[i] = x0c;
        }
    }
}

template <bool GUIDED, bool VEC, bool Y2VEC, bool FULL, bool KP = false>
__global__ __launch_bounds__(SKP_EW_BLOCK) void skp_sampler_step_kernel(const float* x, const float* __restrict__ mc,
                                                                        const float* __restrict__ mu, StepExtra<FULL> e, float* y,
                                                                        long long n, int copies, StepCoef c) {
    step_body<GUIDED, VEC, Y2VEC, FULL, KP>(x, mc, mu, e, y, n, copies, c);
}

// The device-row form: StepCoef from row *step of `table` ([steps, SKP_STEP_ROW]: sa sb cx c0 ce c1 cn guidance), this step's noise
// at noise + *step * n.  A term whose coefficient is 0 loses its pointer here, before the body: the body then neither reads the
// buffer nor sees what it holds (p / nz are 0, as for the by-value entry's null pointers).  *step and the row are the same for
// every lane of the grid, so these branches are uniform.  A counter outside the table: nothing is read or written.
template <bool GUIDED, bool VEC, bool Y2VEC, bool FULL, bool KP = false>
__global__ __launch_bounds__(SKP_EW_BLOCK) void skp_sampler_step_dev_kernel(const float* x, const float* __restrict__ mc,
                                                                            const float* __restrict__ mu, StepExtra<FULL> e, float* y,
                                                                            long long n, int copies, const float* __restrict__ table,
                                                                            const int* __restrict__ step, int steps, int prediction,
                                                                            int clip) {
    const int s = *step;
    if (s < 0 || s >= steps) return;
    const float* __restrict__ r = table + (long long)s * SKP_STEP_ROW;
    StepCoef c;
    c.g = r[7], c.sa = r[0], c.sb = r[1], c.c0 = r[3], c.ce = r[4];
    c.cx = FULL ? r[2] : 0.f, c.c1 = FULL ? r[5] : 0.f, c.cn = FULL ? r[6] : 0.f;
    c.kr = KP ? (float)((double)c.sb / (double)c.sa) : 0.f;
    c.prediction = prediction, c.clip = clip;
    if constexpr (FULL) {
        if (c.c1 == 0.f) e.x0_prev = nullptr;
        e.noise = (c.cn == 0.f || !e.noise) ? nullptr : e.noise + (long long)s * n;
    }
    step_body<GUIDED, VEC, Y2VEC, FULL, KP>(x, mc, mu, e, y, n, copies, c);
}

// The alignment decision, the grid and the launch for both entries, which have checked their arguments.  `full`: the sampler form;
// otherwise x0_prev, noise and x0_out are null and the kernel does not take them.  `kg` (sampler form only): the guidance gradient,
// with its `rows` scales `kgs`; null for the two entries without it.
int step_launch(bool full, const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise, float* y,
                float* x0_out, int64_t n, int copies, const StepCoef& c, void* stream, const float* kg = nullptr,
                const float* kgs = nullptr, int rows = 1, const float* table = nullptr, const int* step = nullptr, int steps = 0) {
    // (device-row form: `noise` is the base of [steps, n], and its rows are 16-byte aligned with it only when n % 4 == 0)
    const bool vec = skp_aligned16(x) && skp_aligned16(m_c) && skp_aligned16(m_u) && skp_aligned16(x0_prev) && skp_aligned16(noise) &&
                     skp_aligned16(y) && skp_aligned16(x0_out) && skp_aligned16(kg) && n >= 4 &&
                     !(table && noise && (n & 3) != 0);
    const long long per = n / rows;
    const bool y2vec = (n & 3) == 0;
    const dim3 grid(skp_capped_grid(vec ? n / 4 : n)), block(SKP_EW_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define SKP_STEP_AS(G, V, Y2, FULL, KP, ...)                                                                                           \
    do {                                                                                                                               \
        if (table)                                                                                                                     \
            hipLaunchKernelGGL((skp_sampler_step_dev_kernel<G, V, Y2, FULL, KP>), grid, block, 0, st, x, m_c, m_u,                     \
                               StepExtra<FULL>{__VA_ARGS__}, y, (long long)n, copies, table, step, steps, c.prediction, c.clip);       \
        else                                                                                                                           \
            hipLaunchKernelGGL((skp_sampler_step_kernel<G, V, Y2, FULL, KP>), grid, block, 0, st, x, m_c, m_u,                         \
                               StepExtra<FULL>{__VA_ARGS__}, y, (long long)n, copies, c);                                              \
    } while (0)
#define SKP_STEP(G, V, Y2)                                                                      \
    do {                                                                                        \
        if (kg) SKP_STEP_AS(G, V, Y2, true, true, x0_prev, noise, x0_out, kg, kgs, per);        \
        else if (full) SKP_STEP_AS(G, V, Y2, true, false, x0_prev, noise, x0_out, nullptr, nullptr, 1); \
        else SKP_STEP_AS(G, V, Y2, false, false);                                               \
    } while (0)
    if (m_u) {
        if (!vec) SKP_STEP(true, false, false);
        else if (y2vec) SKP_STEP(true, true, true);
        else SKP_STEP(true, true, false);
    } else {
        if (!vec) SKP_STEP(false, false, false);
        else if (y2vec) SKP_STEP(false, true, true);
        else SKP_STEP(false, true, false);
    }
#undef SKP_STEP
#undef SKP_STEP_AS
    return skp_launch_status();
}

__global__ __launch_bounds__(256) void skp_axpby_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                        float* __restrict__ y, long long n, float ca, float cb) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = ca * x[i] + cb * z[i];
}

// the same expression with (ca, cb) = (cx, ce) of row *step
__global__ __launch_bounds__(256) void skp_axpby_dev_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                            float* __restrict__ y, long long n, const float* __restrict__ table,
                                                            const int* __restrict__ step, int steps) {
    const int s = *step;
    if (s < 0 || s >= steps) return;
    const float ca = table[(long long)s * SKP_STEP_ROW + 2], cb = table[(long long)s * SKP_STEP_ROW + 4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = ca * x[i] + cb * z[i];
}

// one lane; the value goes through a vector register (volatile: a plain global load and store, nothing the compiler may move)
__global__ __launch_bounds__(64) void skp_step_advance_kernel(volatile int* step) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int v = *step;
        *step = v + 1;
    }
}

}  // namespace

extern "C" int skp_ddim_step_f32(const float* x, const float* m_c, const float* m_u, float* y, int64_t n, int copies, float guidance,
                                 int prediction, float sa, float sb, float pa, float pb, int clip, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    const StepCoef c{guidance, sa, sb, 0.f, pa, pb, 0.f, 0.f, 0.f, prediction, clip ? 1 : 0};
    return step_launch(false, x, m_c, m_u, nullptr, nullptr, y, nullptr, n, copies, c, stream);
}

extern "C" int skp_sampler_step_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise,
                                    float* y, float* x0_out, int64_t n, int copies, float guidance, int prediction, float sa,
                                    float sb, float cx, float c0, float ce, float c1, float cn, int clip, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if ((c1 != 0.f && !x0_prev) || (cn != 0.f && !noise)) return SKP_E_BADARG;
    if (c1 == 0.f) x0_prev = nullptr;                               // not read: a buffer that holds no x0 yet may be anything, NaN included
    if (cn == 0.f) noise = nullptr;
    const StepCoef c{guidance, sa, sb, cx, c0, ce, c1, cn, 0.f, prediction, clip ? 1 : 0};
    return step_launch(true, x, m_c, m_u, x0_prev, noise, y, x0_out, n, copies, c, stream);
}

extern "C" int skp_sampler_step_kp_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise,
                                       float* y, float* x0_out, int64_t n, int copies, float guidance, int prediction, float sa,
                                       float sb, float cx, float c0, float ce, float c1, float cn, int clip, const float* g,
                                       const float* gs, int rows, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if ((c1 != 0.f && !x0_prev) || (cn != 0.f && !noise)) return SKP_E_BADARG;
    if (!g || !gs || rows <= 0 || n % rows != 0) return SKP_E_BADARG;
    if (c1 == 0.f) x0_prev = nullptr;
    if (cn == 0.f) noise = nullptr;
    const StepCoef c{guidance, sa, sb, cx, c0, ce, c1, cn, (float)((double)sb / (double)sa), prediction, clip ? 1 : 0};
    return step_launch(true, x, m_c, m_u, x0_prev, noise, y, x0_out, n, copies, c, stream, g, gs, rows);
}

// y[i] = a * x[i] + b * z[i], i < n (y may be x or z).  The eta = 0 DDIM update with clip_sample off is exactly this.
extern "C" int skp_axpby_f32(const void* x, const void* z, void* y, int64_t n, float a, float b, void* stream) {
    if (!x || !z || !y || n <= 0) return SKP_E_BADARG;
    if (n > (int64_t)0x7fffffff * 256) return SKP_E_RANGE;
    hipLaunchKernelGGL(skp_axpby_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)z, (float*)y, (long long)n, a, b);
    return skp_launch_status();
}

// ---- device-row forms (include/skp_sampler_graph.h) ----
extern "C" int skp_axpby_dev_f32(const float* x, const float* z, float* y, int64_t n, const float* table, const int32_t* step,
                                 int steps, void* stream) {
    if (!x || !z || !y || n <= 0 || !table || !step || steps <= 0) return SKP_E_BADARG;
    if (n > (int64_t)0x7fffffff * 256) return SKP_E_RANGE;
    hipLaunchKernelGGL(skp_axpby_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, z, y,
                       (long long)n, table, (const int*)step, steps);
    return skp_launch_status();
}

extern "C" int skp_ddim_step_dev_f32(const float* x, const float* m_c, const float* m_u, float* y, int64_t n, int copies,
                                     int prediction, int clip, const float* table, const int32_t* step, int steps, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if (!table || !step || steps <= 0) return SKP_E_BADARG;
    const StepCoef c{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, prediction, clip ? 1 : 0};      // (the kernel fills the floats)
    return step_launch(false, x, m_c, m_u, nullptr, nullptr, y, nullptr, n, copies, c, stream, nullptr, nullptr, 1, table,
                       (const int*)step, steps);
}

extern "C" int skp_sampler_step_dev_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise,
                                        float* y, float* x0_out, int64_t n, int copies, int prediction, int clip, const float* table,
                                        const int32_t* step, int steps, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if (!table || !step || steps <= 0) return SKP_E_BADARG;
    const StepCoef c{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, prediction, clip ? 1 : 0};
    return step_launch(true, x, m_c, m_u, x0_prev, noise, y, x0_out, n, copies, c, stream, nullptr, nullptr, 1, table,
                       (const int*)step, steps);
}

extern "C" int skp_sampler_step_kp_dev_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev,
                                           const float* noise, float* y, float* x0_out, int64_t n, int copies, int prediction,
                                           int clip, const float* table, const int32_t* step, int steps, const float* g,
                                           const float* gs, int rows, void* stream) {
    if (!x || !m_c || !y || n <= 0 || (copies != 1 && copies != 2) || prediction < 0 || prediction > 2) return SKP_E_BADARG;
    if (!table || !step || steps <= 0) return SKP_E_BADARG;
    if (!g || !gs || rows <= 0 || n % rows != 0) return SKP_E_BADARG;
    const StepCoef c{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, prediction, clip ? 1 : 0};
    return step_launch(true, x, m_c, m_u, x0_prev, noise, y, x0_out, n, copies, c, stream, g, gs, rows, table, (const int*)step,
                       steps);
}

extern "C" int skp_step_advance(int32_t* step, void* stream) {
    if (!step) return SKP_E_BADARG;
    hipLaunchKernelGGL(skp_step_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (volatile int*)step);
    return skp_launch_status();
}
