// Energy of pose transfer (ptp_utils.py `keypoint_energy_grad` with map targets; the reference's optimize.py
// `find_gaussian_loss_at_point` with the target handed in): K maps per image against K target maps read from device memory, and its
// unit gradient by the maps.  The sibling of skp_point_loss.hip; the formulas per element are in include/skp_targets.h.
//   mode 0 (mse):    one pass, like the sibling: the 1024-element chunk sums of (M - T)^2 and G = 2 (M - T) / (K R^2).
//   mode 1 (cosine): two passes.  The first writes per chunk (sum M^2, sum T^2, sum M T); the second folds the chunk sums of its own
//                    map in a fixed order, normalises both maps, and writes G and the chunk sums of (M/|M| - T/|T|)^2.
// One workgroup per (image, map, chunk), four elements per lane, also for maps of one chunk: a workgroup per whole map would leave
// most of the chip idle at the K ~ 10 maps of 128^2 this is built for, and the plan stays a function of (B, K, R) alone.  The sums are
// the fixed butterfly of skp_block_sum_256, here on doubles: no atomics, the same bits from call to call.  Everything between the
// float inputs and the float outputs is fp64 (a product of two floats is exact there), so each output carries one rounding; the
// kernels stay bound by their 8 to 12 bytes per element.
#include "skp_common.h"
#include "../../include/skp_targets.h"

namespace {

constexpr int TL_CHUNK = 1024;

__device__ __forceinline__ double tl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// skp_block_sum_256 on doubles; `red` = 4 doubles of LDS.  All threads get the result.
__device__ __forceinline__ double tl_block_sum_256(double v, double* red) {
    v = tl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// map = b * K + k -> the target's map: b * K + k with a target per image, k with a shared one
__device__ __forceinline__ long long tl_target_map(long long map, int K, int shared) { return shared ? map % K : map; }

__global__ __launch_bounds__(256) void skp_target_mse_kernel(const float* __restrict__ M, const float* __restrict__ Tg, int K, int R,
                                                             int nchunk, int shared, double unit, float* __restrict__ partial,
                                                             float* __restrict__ G) {
    __shared__ double red[4];
    const long long map = blockIdx.x / nchunk;                      // b * K + k
    const int chunk = blockIdx.x - (unsigned)(map * nchunk);
    const int n = R * R;
    const float* m = M + map * n;
    const float* t = Tg + tl_target_map(map, K, shared) * n;
    float* g = G + map * n;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < TL_CHUNK / 256; ++e) {
        const int p = chunk * TL_CHUNK + e * 256 + threadIdx.x;
        if (p < n) {
            const double d = (double)m[p] - (double)t[p];
            g[p] = (float)(d * unit);
            acc += d * d;
        }
    }
    const double s = tl_block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = (float)s;
}

__global__ __launch_bounds__(256) void skp_target_dots_kernel(const float* __restrict__ M, const float* __restrict__ Tg, int K, int R,
                                                              int nchunk, int shared, double* __restrict__ sums) {
    __shared__ double red[4];
    const long long map = blockIdx.x / nchunk;
    const int chunk = blockIdx.x - (unsigned)(map * nchunk);
    const int n = R * R;
    const float* m = M + map * n;
    const float* t = Tg + tl_target_map(map, K, shared) * n;
    double a = 0.0, c = 0.0, d = 0.0;
#pragma unroll
    for (int e = 0; e < TL_CHUNK / 256; ++e) {
        const int p = chunk * TL_CHUNK + e * 256 + threadIdx.x;
        if (p < n) {
            const double mv = m[p], tv = t[p];
            a += mv * mv;
            c += tv * tv;
            d += mv * tv;
        }
    }
    a = tl_block_sum_256(a, red);
    c = tl_block_sum_256(c, red);
    d = tl_block_sum_256(d, red);
    if (threadIdx.x == 0) {
        double* o = sums + 3LL * blockIdx.x;
        o[0] = a;
        o[1] = c;
        o[2] = d;
    }
}

__global__ __launch_bounds__(256) void skp_target_cosine_kernel(const float* __restrict__ M, const float* __restrict__ Tg, int K, int R,
                                                                int nchunk, int shared, const double* __restrict__ sums,
                                                                float* __restrict__ partial, float* __restrict__ G) {
    __shared__ double red[4];
    const long long map = blockIdx.x / nchunk;
    const int chunk = blockIdx.x - (unsigned)(map * nchunk);
    const int n = R * R;
    // the chunk sums of this map: lane i takes chunks i, i + 256, ... in rising order, then the butterfly
    double a = 0.0, c = 0.0, d = 0.0;
    const double* s = sums + 3LL * map * nchunk;
    for (int j = threadIdx.x; j < nchunk; j += 256) {
        a += s[3LL * j];
        c += s[3LL * j + 1];
        d += s[3LL * j + 2];
    }
    a = tl_block_sum_256(a, red);
    c = tl_block_sum_256(c, red);
    d = tl_block_sum_256(d, red);
    const float* m = M + map * n;
    const float* t = Tg + tl_target_map(map, K, shared) * n;
    float* g = G + map * n;
    if (a == 0.0 || c == 0.0) {                                     // a map or a target of zeros: E_k = 1 (the sum is 2), G = 0
#pragma unroll
        for (int e = 0; e < TL_CHUNK / 256; ++e) {
            const int p = chunk * TL_CHUNK + e * 256 + threadIdx.x;
            if (p < n) g[p] = 0.f;
        }
        if (threadIdx.x == 0) partial[blockIdx.x] = chunk == 0 ? 2.f : 0.f;
        return;
    }
    const double ia = 1.0 / sqrt(a), ic = 1.0 / sqrt(c);
    const double cs = d / sqrt(a * c);
    const double coef = ia / (double)K;                             // 1 / (K sqrt(a))
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < TL_CHUNK / 256; ++e) {
        const int p = chunk * TL_CHUNK + e * 256 + threadIdx.x;
        if (p < n) {
            const double mh = (double)m[p] * ia, th = (double)t[p] * ic;
            const double df = mh - th;
            g[p] = (float)((cs * mh - th) * coef);
            acc += df * df;
        }
    }
    const double e = tl_block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = (float)e;
}

// -> workgroups of one pass, or an SKP_E_* code
long long tl_blocks(int B, int K, int R) {
    if (B <= 0 || K <= 0 || R <= 0) return SKP_E_BADARG;
    if (R > 32768) return SKP_E_RANGE;                              // R * R in an int
    const long long nchunk = ((long long)R * R + TL_CHUNK - 1) / TL_CHUNK;
    const long long blocks = (long long)B * K * nchunk;
    return blocks > 0x7fffffffLL ? (long long)SKP_E_RANGE : blocks;
}

}  // namespace

extern "C" int64_t skp_map_target_loss_workspace(int B, int K, int R, int mode) {
    if (mode != 0 && mode != 1) return SKP_E_BADARG;
    const long long blocks = tl_blocks(B, K, R);
    if (blocks < 0) return blocks;
    return mode == 0 ? 0 : blocks * 3 * (int64_t)sizeof(double);
}

extern "C" int skp_map_target_loss_f32(const float* M, const float* Tg, int B, int Bt, int K, int R, int mode, float* partial, float* G,
                                       void* workspace, void* stream) {
    if (!M || !Tg || !partial || !G || (mode != 0 && mode != 1) || (mode == 1 && !workspace)) return SKP_E_BADARG;
    const long long blocks = tl_blocks(B, K, R);
    if (blocks < 0) return (int)blocks;
    if (Bt != 1 && Bt != B) return SKP_E_BADARG;
    const int nchunk = (int)(((long long)R * R + TL_CHUNK - 1) / TL_CHUNK);
    const int shared = Bt == 1;
    if (mode == 0) {
        const double unit = 2.0 / ((double)K * R * R);
        hipLaunchKernelGGL(skp_target_mse_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, M, Tg, K, R, nchunk, shared,
                           unit, partial, G);
        return skp_launch_status();
    }
    double* sums = (double*)workspace;
    hipLaunchKernelGGL(skp_target_dots_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, M, Tg, K, R, nchunk, shared,
                       sums);
    const int rc = skp_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(skp_target_cosine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, M, Tg, K, R, nchunk, shared,
                       (const double*)sums, partial, G);
    return skp_launch_status();
}
