// Evaluation stage (include/skp_locate.h; stablekeypoints_amd/eval.py `locate_keypoints`): the location of the peak of every map of
// a whole group of images in one pass -- the arg-max, and under `weighted_avg` the intensity-weighted mean over the window around it.
//   skp_locate_kernel<G>      a GROUP of G threads (one wave for maps of <= 1024 elements, else the whole 256-thread workgroup) scans
//                             one segment of one map: 16-byte loads, (value, index) butterflies, for G = 256 a fold of the four
//                             waves through LDS.  A map that is not split is finished by its group at once; the segments of a
//                             split map leave their (value, index) pair -- and for the whole-map mean their three fp64 sums -- in
//                             the workspace.
//   skp_locate_fold_kernel    one workgroup per split map folds its <= 256 pairs (and sums) in a fixed order and finishes the map.
// Finishing = `lc_finish`, the same code on both ways: for distance >= 0 the group walks the bounding box of the window, element k
// of the box by thread k % G, and sums by the same butterflies, so the bits do not depend on whether or how the map was split.
// The sums are fp64 (the kernels are bound by memory or by launch latency; the few fp64 operations per element do not show).
#include "skp_common.h"
#include "../../include/skp_locate.h"

namespace {

constexpr int LC_MAX_SIDE = 4096;            // (r - r*)^2 + (c - c*)^2 is exact in fp32 term by term, and H W fits an int
constexpr int LC_WAVE_PLANE = 1024;          // maps up to here: one wave each
constexpr int LC_SPLIT_PLANE = 8192;         // maps from here on may be split ...
constexpr int LC_MIN_SEG = 4096;             // ... into segments of at least this many elements,
constexpr int LC_MAX_SPLITS = 256;           // at most this many (the fold kernel's one workgroup takes one pair per thread),
constexpr int LC_WANT_GROUPS = 2048;         // about this many workgroups over all maps

struct LcPart {                              // what a segment leaves in the workspace: 32 bytes
    float v;
    int i;
    double t, sr, sc;
};
static_assert(sizeof(LcPart) == 32, "the workspace query counts 32 bytes per segment");

struct LcPlan {
    int group;                               // threads per map segment: 64 or 256
    int splits;
    int seg;                                 // elements per segment, a multiple of 4
};
LcPlan lc_plan(int N, int H, int W) {
    const int plane = H * W;
    if (plane <= LC_WAVE_PLANE) return LcPlan{64, 1, plane};
    if (plane < LC_SPLIT_PLANE) return LcPlan{256, 1, plane};
    int want = (LC_WANT_GROUPS + N - 1) / N, most = plane / LC_MIN_SEG;
    int splits = want < most ? want : most;
    splits = splits < 1 ? 1 : (splits > LC_MAX_SPLITS ? LC_MAX_SPLITS : splits);
    if (splits == 1) return LcPlan{256, 1, plane};
    const int seg = ((plane + splits - 1) / splits + 3) / 4 * 4;
    return LcPlan{256, (plane + seg - 1) / seg, seg};               // no empty segment
}

struct LcArgs {
    const float* M;
    float* loc;
    int* flat;
    LcPart* part;
    int N, H, W, mode, splits, seg;
    float distance;
};

// (value desc, index asc): torch.argmax's "first maximal index", the order of skp_token_stats_f32.  NaN never wins.
__device__ __forceinline__ bool lc_better(float v, int i, float bv, int bi) { return (v > bv) || (v == bv && i < bi); }

__device__ __forceinline__ double lc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct LcShared {                            // G = 256 only
    float v[4];
    int i[4];
    double s[3][4];
};

// every thread of the group ends with the group's pair
template <int G>
__device__ __forceinline__ void lc_group_best(float& bv, int& bi, LcShared* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (lc_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (G == 256) {
        __syncthreads();                                            // (the arrays may still be read from an earlier fold)
        if ((threadIdx.x & 63) == 0) { sh->v[threadIdx.x >> 6] = bv; sh->i[threadIdx.x >> 6] = bi; }
        __syncthreads();
        bv = sh->v[0]; bi = sh->i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (lc_better(sh->v[w], sh->i[w], bv, bi)) { bv = sh->v[w]; bi = sh->i[w]; }
    }
}

// every thread of the group ends with the group's three sums: butterflies, then ((w0 + w1) + (w2 + w3))
template <int G>
__device__ __forceinline__ void lc_group_sums(double& t, double& sr, double& sc, LcShared* sh) {
    t = lc_wave_sum(t); sr = lc_wave_sum(sr); sc = lc_wave_sum(sc);
    if (G == 256) {
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
            const int w = threadIdx.x >> 6;
            sh->s[0][w] = t; sh->s[1][w] = sr; sh->s[2][w] = sc;
        }
        __syncthreads();
        t = (sh->s[0][0] + sh->s[0][1]) + (sh->s[0][2] + sh->s[0][3]);
        sr = (sh->s[1][0] + sh->s[1][1]) + (sh->s[1][2] + sh->s[1][3]);
        sc = (sh->s[2][0] + sh->s[2][1]) + (sh->s[2][2] + sh->s[2][3]);
    }
}

__device__ __forceinline__ void lc_take(float v, int e, int r, int c, bool whole, float& bv, int& bi, double& t, double& sr,
                                        double& sc) {
    if (lc_better(v, e, bv, bi)) { bv = v; bi = e; }
    if (whole) {
        const double d = (double)v;
        t += d; sr += (double)r * d; sc += (double)c * d;
    }
}

// The group holds the arg-max `bi` of map n (and, for the whole-map mean, the sums): writes flat[n] and loc[n].  `lane` = the
// thread's index in its group.
template <int G>
__device__ __forceinline__ void lc_finish(const LcArgs& a, long long n, int bi, double t, double sr, double sc, int lane,
                                          LcShared* sh) {
    const int plane = a.H * a.W;
    if ((unsigned)bi >= (unsigned)plane) bi = 0;                   // a map of only NaN: no element ever won
    const int rs = bi / a.W, cs = bi - rs * a.W;
    float y = (float)rs + 0.5f, x = (float)cs + 0.5f;
    if (a.mode == 1) {
        if (a.distance >= 0.f) {
            // bounding box of the window, clipped to the map; floor(distance) capped so that the int arithmetic cannot overflow
            const int R = (int)fminf(a.distance, (float)LC_MAX_SIDE);
            const int r0 = max(0, rs - R), r1 = min(a.H - 1, rs + R), c0 = max(0, cs - R), c1 = min(a.W - 1, cs + R);
            const int ww = c1 - c0 + 1, count = (r1 - r0 + 1) * ww;
            const float* m = a.M + n * plane;
            t = sr = sc = 0.0;
            for (int k = lane; k < count; k += G) {
                const int kr = k / ww, r = r0 + kr, c = c0 + (k - kr * ww);
                const int dr = r - rs, dc = c - cs;
                if (__fsqrt_rn((float)(dr * dr + dc * dc)) <= a.distance) {
                    const double d = (double)m[r * a.W + c];
                    t += d; sr += (double)r * d; sc += (double)c * d;
                }
            }
            lc_group_sums<G>(t, sr, sc, sh);
        }
        const double den = t + 1e-6;
        y = (float)(sr / den + 0.5);
        x = (float)(sc / den + 0.5);
    }
    if (lane == 0) {
        a.flat[n] = bi;
        a.loc[2 * n] = y;
        a.loc[2 * n + 1] = x;
    }
}

// group g of the grid: segment g % splits of map g / splits.  G = 64: four groups (waves) per workgroup, no LDS, no barrier.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void skp_locate_kernel(const LcArgs a) {
    __shared__ LcShared sh;
    const int lane = threadIdx.x & (G - 1);
    const long long g = (long long)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (g >= (long long)a.N * a.splits) return;                     // (G = 64 only: whole waves leave, nothing below is a barrier for them)
    const long long n = g / a.splits;
    const int s = (int)(g - n * a.splits), plane = a.H * a.W;
    const int e0 = s * a.seg, e1 = min(plane, e0 + a.seg);
    const float* m = a.M + n * plane;
    const bool whole = a.mode == 1 && a.distance < 0.f;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    double t = 0.0, sr = 0.0, sc = 0.0;
    if (VEC) {                                                      // plane % 4 == 0 and M 16-byte aligned: e0, e1 are multiples of 4
        const f32x4* m4 = (const f32x4*)m;
        for (int q = e0 / 4 + lane; q < e1 / 4; q += G) {
            const f32x4 v = m4[q];
            int e = 4 * q, r = 0, c = 0;
            if (whole) { r = e / a.W; c = e - r * a.W; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lc_take(v[j], e + j, r, c, whole, bv, bi, t, sr, sc);
                if (++c == a.W) { c = 0; ++r; }
            }
        }
    } else {
        for (int e = e0 + lane; e < e1; e += G) {
            int r = 0, c = 0;
            if (whole) { r = e / a.W; c = e - r * a.W; }
            lc_take(m[e], e, r, c, whole, bv, bi, t, sr, sc);
        }
    }
    lc_group_best<G>(bv, bi, &sh);
    if (whole) lc_group_sums<G>(t, sr, sc, &sh);
    if (a.splits == 1) {
        lc_finish<G>(a, n, bi, t, sr, sc, lane, &sh);
    } else if (lane == 0) {
        a.part[g] = LcPart{bv, bi, t, sr, sc};
    }
}

// one workgroup per split map: thread s takes segment s (splits <= 256)
__global__ __launch_bounds__(256) void skp_locate_fold_kernel(const LcArgs a) {
    __shared__ LcShared sh;
    const long long n = blockIdx.x;
    const int s = threadIdx.x;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    double t = 0.0, sr = 0.0, sc = 0.0;
    if (s < a.splits) {
        const LcPart p = a.part[n * a.splits + s];
        bv = p.v; bi = p.i; t = p.t; sr = p.sr; sc = p.sc;
    }
    lc_group_best<256>(bv, bi, &sh);
    if (a.mode == 1 && a.distance < 0.f) lc_group_sums<256>(t, sr, sc, &sh);
    lc_finish<256>(a, n, bi, t, sr, sc, s, &sh);
}

int lc_check(int N, int H, int W, LcPlan* pl) {
    if (N <= 0 || H <= 0 || W <= 0) return SKP_E_BADARG;
    if (H > LC_MAX_SIDE || W > LC_MAX_SIDE) return SKP_E_RANGE;
    *pl = lc_plan(N, H, W);                                         // (N * splits <= max(N, 2048 + 256): a legal grid)
    return 0;
}

}  // namespace

extern "C" int64_t skp_locate_workspace(int N, int H, int W) {
    LcPlan pl;
    const int rc = lc_check(N, H, W, &pl);
    if (rc) return rc;
    return pl.splits > 1 ? (int64_t)N * pl.splits * (int64_t)sizeof(LcPart) : 0;
}

extern "C" int skp_locate_f32(const float* M, int N, int H, int W, int mode, float distance, float* loc, int* flat, void* ws,
                              int64_t ws_bytes, void* stream) {
    if (!M || !loc || !flat) return SKP_E_BADARG;
    LcPlan pl;
    const int rc = lc_check(N, H, W, &pl);
    if (rc) return rc;
    if (mode != 0 && mode != 1) return SKP_E_BADARG;
    if (mode == 1 && !(distance >= 0.f || distance == -1.f)) return SKP_E_BADARG;
    if (pl.splits > 1 && (!ws || ws_bytes < (int64_t)N * pl.splits * (int64_t)sizeof(LcPart))) return SKP_E_BADARG;
    const LcArgs a{M, loc, flat, (LcPart*)ws, N, H, W, mode, pl.splits, pl.seg, mode == 1 ? distance : 0.f};
    hipStream_t st = (hipStream_t)stream;
    const long long groups = (long long)N * pl.splits;
    const bool vec = ((H * W) & 3) == 0 && skp_aligned16(M);
    if (pl.group == 64) {
        const dim3 grid((unsigned)((groups + 3) / 4)), block(256);
        if (vec) hipLaunchKernelGGL((skp_locate_kernel<64, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((skp_locate_kernel<64, false>), grid, block, 0, st, a);
    } else {
        const dim3 grid((unsigned)groups), block(256);
        if (vec) hipLaunchKernelGGL((skp_locate_kernel<256, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((skp_locate_kernel<256, false>), grid, block, 0, st, a);
    }
    if (pl.splits > 1) hipLaunchKernelGGL(skp_locate_fold_kernel, dim3((unsigned)N), dim3(256), 0, st, a);
    return skp_launch_status();
}
