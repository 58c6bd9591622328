// Energy of keypoint guidance (ptp_utils.py `keypoint_energy_grad`; the reference's optimize.py `find_gaussian_loss_at_point` with one
// point per token): for K maps per image and a caller-given position per map, in device memory,
//   t[r,c] = exp(-((c + 0.5 - R p_col)^2 + (r + 0.5 - R p_row)^2) / (2 sigma^2)),   E = mean_{k,r,c} (M - t)^2,
// one pass that writes the 1024-element chunk sums of (M - t)^2 and the unit gradient G = 2 (M - t) / (K R^2).
// One workgroup per (image, map, chunk), four elements per lane; the chunk sum is the fixed butterfly of skp_block_sum_256: no atomics,
// the same bits from call to call.  The exponent is formed in fp64 (its inputs are fp32 numbers and small integers, so it is exact up
// to the division) and split into a float and its remainder, e^-a = expf(-a_hi) (1 - a_lo): a plain float exponent of size a carries
// a relative error of a * 2^-24 into t, two decimal digits at the rim of the target where a is about 100.
#include "skp_common.h"

namespace {

constexpr int PL_CHUNK = 1024;

__global__ __launch_bounds__(256) void skp_point_loss_kernel(const float* __restrict__ M, const float* __restrict__ pos, int R, int nchunk,
                                                             double inv_den, float unit, float* __restrict__ partial,
                                                             float* __restrict__ G) {
    __shared__ float red[4];
    const long long map = blockIdx.x / nchunk;                      // b * K + k
    const int chunk = blockIdx.x - (unsigned)(map * nchunk);
    const int n = R * R;
    const double pr = (double)pos[2 * map] * R, pc = (double)pos[2 * map + 1] * R;
    const float* m = M + map * n;
    float* g = G + map * n;
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < PL_CHUNK / 256; ++e) {
        const int p = chunk * PL_CHUNK + e * 256 + threadIdx.x;
        if (p < n) {
            const int r = p / R, c = p - r * R;
            const double dr = (double)r + 0.5 - pr, dc = (double)c + 0.5 - pc;
            // beyond 200 the target is 0 in fp32 either way (expf underflows past 104); the cap keeps a far position's exponent
            // from overflowing the float split into inf - inf
            const double a = fmin((dc * dc + dr * dr) * inv_den, 200.0);
            const float ah = (float)a;
            const float al = (float)(a - (double)ah);
            const float t = expf(-ah) * (1.f - al);
            const float d = m[p] - t;
            g[p] = d * unit;
            acc += d * d;
        }
    }
    const float s = skp_block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

}  // namespace

extern "C" int skp_point_loss_f32(const float* M, const float* pos, int B, int K, int R, float sigma, float* partial, float* G,
                                  void* stream) {
    if (!M || !pos || !partial || !G || B <= 0 || K <= 0 || R <= 0 || !(sigma > 0.f)) return SKP_E_BADARG;
    if (R > 32768) return SKP_E_RANGE;                              // R * R in an int
    const long long nchunk = ((long long)R * R + PL_CHUNK - 1) / PL_CHUNK;
    const long long blocks = (long long)B * K * nchunk;
    if (blocks > 0x7fffffffLL) return SKP_E_RANGE;
    const double inv_den = 1.0 / (2.0 * (double)sigma * (double)sigma);
    const float unit = (float)(2.0 / ((double)K * R * R));
    hipLaunchKernelGGL(skp_point_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, M, pos, R, (int)nchunk, inv_den,
                       unit, partial, G);
    return skp_launch_status();
}
