// Keypoint visualisation (include/skp_overlay.h; stablekeypoints_amd/visualize.py): from (images, maps, points) to bytes in one pass.
//   skp_map_range_f32    (min, max) of every map, NaN ignored.  A map is cut into segments over several workgroups so that one map
//                        fills the machine as 990 do; every workgroup reduces its segment (16-byte loads, wave butterflies, LDS) to
//                        a pair of integer keys, a second small kernel folds the pairs.  The keys are the bit patterns in an order
//                        that is the order of the floats (-0 < +0), so integer min / max are exact and independent of the split.
//   skp_overlay_u8_f32   clamp -> heat map through a colour table -> numbered markers -> uint8 NHWC into a canvas of tiles.  The
//                        sibling of skp_image_u8_nhwc_f32 (skp_conv_out.hip): one lane = four consecutive pixels (16-byte loads,
//                        three dwords out) or one pixel, the grid capped with a grid-stride loop.  The loop runs over UNITS of
//                        256 lanes' pixels of ONE image, so everything per image (range, points, colours) is workgroup-uniform and
//                        comes through scalar loads; the colour table and the glyphs are staged in LDS once per workgroup.  Per
//                        unit, lane j < K tests marker j against the rows the unit covers, and a ballot leaves the markers that
//                        can touch it as two 64-bit masks: the marker loop runs over set bits only, in ascending order.
#include "skp_common.h"
#include "../../include/skp_overlay.h"

// No fma contraction in this file: every product and sum of the overlay is rounded on its own, as in `visualize.overlay_formula` in
// float32 (torch rounds every op), so the device route and the host route agree operation by operation.  The kernels are bound by
// memory; the handful of extra VALU operations per pixel does not show.
#pragma clang fp contract(off)

namespace {

constexpr int OV_MAX_SIDE = 4096, OV_MAX_K = 100, OV_MAX_L = 1024;

// ---------------------------------------------------------------------------------------------------------------------------
// range
// ---------------------------------------------------------------------------------------------------------------------------
// bit pattern -> a signed key whose integer order is the order of the floats (negative floats reversed; -0 = -1 < +0 = 0); its own inverse
__device__ __forceinline__ int rg_key(int bits) { return bits < 0 ? bits ^ 0x7fffffff : bits; }

__device__ __forceinline__ void rg_take(float v, int& lo, int& hi) {
    const int k = rg_key(__float_as_int(v));
    const bool ok = v == v;
    lo = ok ? min(lo, k) : lo;
    hi = ok ? max(hi, k) : hi;
}

__device__ __forceinline__ void rg_finish(int lo, int hi, float* out) {      // an empty set (only NaN) is (0, 0)
    const bool any = lo <= hi;
    out[0] = any ? __int_as_float(rg_key(lo)) : 0.f;
    out[1] = any ? __int_as_float(rg_key(hi)) : 0.f;
}

// 256 threads: all of them end with the workgroup's pair; `red` = 8 ints of LDS
__device__ __forceinline__ void rg_block(int& lo, int& hi, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = min(min(red[0], red[1]), min(red[2], red[3]));
    hi = max(max(red[4], red[5]), max(red[6], red[7]));
}

// workgroup (n, s): elements [s * seg, min(plane, (s + 1) * seg)) of map n; seg % 4 == 0.  splits == 1: the finished pair to `range`.
template <bool VEC>
__global__ __launch_bounds__(256) void skp_map_range_kernel(const float* __restrict__ M, int* __restrict__ part,
                                                            float* __restrict__ range, long long plane, long long seg,
                                                            int splits) {
    __shared__ int red[8];
    const long long n = blockIdx.x / splits;
    const int s = blockIdx.x - (int)n * splits;
    const long long e0 = (long long)s * seg, e1 = min(plane, e0 + seg);
    const float* m = M + n * plane;
    int lo = 0x7fffffff, hi = (int)0x80000000;
    if (VEC) {                                                     // plane % 4 == 0 and M 16-byte aligned: e0 and e1 are multiples of 4
        const f32x4* m4 = (const f32x4*)m;
        for (long long q = e0 / 4 + threadIdx.x; q < e1 / 4; q += 256) {
            const f32x4 v = m4[q];
            rg_take(v[0], lo, hi);
            rg_take(v[1], lo, hi);
            rg_take(v[2], lo, hi);
            rg_take(v[3], lo, hi);
        }
    } else {
        for (long long e = e0 + threadIdx.x; e < e1; e += 256) rg_take(m[e], lo, hi);
    }
    rg_block(lo, hi, red);
    if (threadIdx.x == 0) {
        if (splits == 1) {
            rg_finish(lo, hi, range + 2 * n);
        } else {
            part[2 * (long long)blockIdx.x] = lo;
            part[2 * (long long)blockIdx.x + 1] = hi;
        }
    }
}

// one wave per map: folds its `splits` pairs (splits <= 256)
__global__ __launch_bounds__(64) void skp_map_range_fold_kernel(const int* __restrict__ part, float* __restrict__ range, int splits) {
    const long long n = blockIdx.x;
    int lo = 0x7fffffff, hi = (int)0x80000000;
    for (int s = threadIdx.x; s < splits; s += 64) {
        lo = min(lo, part[2 * (n * splits + s)]);
        hi = max(hi, part[2 * (n * splits + s) + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (threadIdx.x == 0) rg_finish(lo, hi, range + 2 * n);
}

// The split of a map: enough workgroups to fill the machine (about 2048 over all maps), at least 1024 elements each, at most 256.
struct RangePlan {
    int splits;
    long long seg;
};
RangePlan rg_plan(int N, long long plane) {
    long long want = (2048 + N - 1) / N, most = (plane + 1023) / 1024;
    long long splits = want < most ? want : most;
    splits = splits < 1 ? 1 : (splits > 256 ? 256 : splits);
    long long seg = ((plane + splits - 1) / splits + 3) / 4 * 4;
    splits = (plane + seg - 1) / seg;                              // no empty segment
    return RangePlan{(int)splits, seg};
}

// ---------------------------------------------------------------------------------------------------------------------------
// overlay
// ---------------------------------------------------------------------------------------------------------------------------
struct OvArgs {
    const float *img, *map, *range, *lut, *pts, *colors;
    const unsigned char* glyphs;
    unsigned char* out;
    int B, H, W, S, L, K;
    float alpha, r_ring, r_disc;                                   // radius + ring + 0.5, radius + 0.5
    int labels, fs1, fs2;                                          // glyph scale of one- and two-digit labels
    long long ld;
    int y0, x0, cols, gap;
    int upi;                                                       // units per image
    long long units;
};

__device__ __forceinline__ unsigned ov_u8(float v) { return (unsigned)(int)(v * 255.0f) & 0xffu; }      // (skp_conv_out.hip: u8_of)
__device__ __forceinline__ float ov_sat(float v) { return fminf(fmaxf(v, 0.f), 1.f); }                  // (NaN -> 0)
__device__ __forceinline__ float ov_lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ void ov_heat(float c[3], float m, float lo, float hi, const float* lut, int L, float alpha) {
    const float n = (hi > lo && m == m) ? ov_sat((m - lo) / (hi - lo)) : 0.f;
    const float t = n * (float)(L - 1);
    const int i = min((int)t, L - 2);
    const float f = t - (float)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float colour = ov_lerp(lut[3 * i + k], lut[3 * i + 3 + k], f);
        const float keep = (1.f - alpha) * c[k];
        c[k] = keep + alpha * colour;
    }
}

// source coordinate of F.interpolate(mode="bilinear", align_corners=False): two indices and the weight of the second
__device__ __forceinline__ void ov_tap(int dst, float ratio, int S, int& i0, int& i1, float& t) {
    const float src = fmaxf(ratio * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = min((int)src, S - 1);
    i1 = min(i0 + 1, S - 1);
    t = src - (float)i0;
}

struct OvMarker {                                                  // workgroup-uniform
    float py, px, col[3];
    int oy, ox, fs, bw, d_hi, d_lo;                                // label box: top-left, scale, width in glyph columns, digits
};

__device__ __forceinline__ void ov_mark(float c[3], int y, int x, const OvMarker& mk, float r_ring, float r_disc, int labels,
                                        const unsigned char* glyph) {
    const float dy = ((float)y + 0.5f) - mk.py, dx = ((float)x + 0.5f) - mk.px;
    const float d = sqrtf(dy * dy + dx * dx);
    const float ar = ov_sat(r_ring - d), ad = ov_sat(r_disc - d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = ov_lerp(c[k], 1.f, ar);
        c[k] = ov_lerp(c[k], mk.col[k], ad);
    }
    if (labels) {
        int gy = y - mk.oy, gx = x - mk.ox;
        if (gy >= 0 && gy < 7 * mk.fs && gx >= 0 && gx < mk.bw * mk.fs) {
            gy /= mk.fs;
            gx /= mk.fs;
            int digit = mk.d_lo;
            if (mk.bw == 11) {                                     // tens digit, one empty column, ones digit
                digit = gx < 5 ? mk.d_hi : (gx > 5 ? mk.d_lo : -1);
                gx = gx > 5 ? gx - 6 : gx;
            }
            if (digit >= 0 && ((glyph[7 * digit + gy] >> (4 - gx)) & 1)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = ov_lerp(c[k], 1.f, ad);
            }
        }
    }
}

// V pixels per lane (4: W % 4 == 0 and every alignment holds; 1: anything).  MAP 0: none, 1: S = H = W, 2: bilinear.
template <int V, int MAP>
__global__ __launch_bounds__(SKP_EW_BLOCK) void skp_overlay_kernel(const OvArgs a) {
    __shared__ float s_lut[MAP ? 3 * OV_MAX_L : 1];
    __shared__ unsigned char s_glyph[72];
    __shared__ unsigned long long s_mask[2];
    const int tid = threadIdx.x;
    if (MAP)
        for (int i = tid; i < 3 * a.L; i += SKP_EW_BLOCK) s_lut[i] = a.lut[i];
    if (a.K > 0 && a.labels && tid < 70) s_glyph[tid] = a.glyphs[tid];
    const long long plane = (long long)a.H * a.W;
    const long long lanes = plane / V;                             // lane items per image
    const float ry = (float)a.S / (float)a.H, rx = (float)a.S / (float)a.W;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int b = (int)(u / a.upi);
        const long long first = (u - (long long)b * a.upi) * SKP_EW_BLOCK;         // the unit's first lane item
        __syncthreads();                                           // the tables are staged / the previous unit's masks are read
        if (a.K > 0) {
            // rows the unit covers, and which markers reach them: |row centre - py| <= r_ring + 1 for some row (one pixel of slack
            // over the exact a > 0 test, so rounding cannot drop a marker that paints)
            const long long last = min(first + SKP_EW_BLOCK, lanes) * V - 1;
            const float y_lo = (float)(int)(first * V / a.W) + 0.5f, y_hi = (float)(int)(last / a.W) + 0.5f;
            if (tid < 128) {
                bool on = false;
                if (tid < a.K) {
                    const float py = a.pts[((long long)b * a.K + tid) * 2] * (float)a.H;
                    const float px = a.pts[((long long)b * a.K + tid) * 2 + 1] * (float)a.W;
                    on = py == py && px == px && y_lo - py <= a.r_ring + 1.f && py - y_hi <= a.r_ring + 1.f;
                }
                const unsigned long long m = __ballot(on);
                if ((tid & 63) == 0) s_mask[tid >> 6] = m;
            }
            __syncthreads();
        }
        const long long q = first + tid;
        if (q >= lanes) continue;                                  // (no barrier below this line)
        const long long p = q * V;
        const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
        const float* ib = a.img + (long long)b * 3 * plane + p;
        float c[V][3];
        if (V == 4) {
            const f32x4 r = *(const f32x4*)ib, g = *(const f32x4*)(ib + plane), bl = *(const f32x4*)(ib + 2 * plane);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                c[v][0] = ov_sat(r[v]);
                c[v][1] = ov_sat(g[v]);
                c[v][2] = ov_sat(bl[v]);
            }
        } else {
            c[0][0] = ov_sat(ib[0]);
            c[0][1] = ov_sat(ib[plane]);
            c[0][2] = ov_sat(ib[2 * plane]);
        }
        if (MAP) {
            const float lo = a.range[2 * b], hi = a.range[2 * b + 1];
            const float* mb = a.map + (long long)b * a.S * a.S;
            float m[V];
            if (MAP == 1) {
                if (V == 4) {
                    const f32x4 mv = *(const f32x4*)(mb + p);
#pragma unroll
                    for (int v = 0; v < V; ++v) m[v] = mv[v];
                } else {
                    m[0] = mb[p];
                }
            } else {
                int r0, r1;
                float ty;
                ov_tap(y, ry, a.S, r0, r1, ty);
                const float *row0 = mb + (long long)r0 * a.S, *row1 = mb + (long long)r1 * a.S;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    int c0, c1;
                    float tx;
                    ov_tap(x + v, rx, a.S, c0, c1, tx);
                    const float top = (1.f - tx) * row0[c0] + tx * row0[c1];
                    const float bot = (1.f - tx) * row1[c0] + tx * row1[c1];
                    m[v] = (1.f - ty) * top + ty * bot;
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) ov_heat(c[v], m[v], lo, hi, s_lut, a.L, a.alpha);
        }
        if (a.K > 0) {
#pragma unroll 1
            for (int w = 0; w < 2; ++w) {
                const unsigned long long mv = s_mask[w];
                unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)mv), mhi = __builtin_amdgcn_readfirstlane((unsigned)(mv >> 32));
                unsigned long long mask = ((unsigned long long)mhi << 32) | mlo;
                while (mask) {
                    const int j = 64 * w + __builtin_ctzll(mask);
                    mask &= mask - 1;
                    OvMarker mk;
                    mk.py = a.pts[((long long)b * a.K + j) * 2] * (float)a.H;
                    mk.px = a.pts[((long long)b * a.K + j) * 2 + 1] * (float)a.W;
                    mk.col[0] = a.colors[3 * j];
                    mk.col[1] = a.colors[3 * j + 1];
                    mk.col[2] = a.colors[3 * j + 2];
                    mk.fs = j < 10 ? a.fs1 : a.fs2;
                    mk.bw = j < 10 ? 5 : 11;
                    mk.d_hi = j / 10;
                    mk.d_lo = j - 10 * mk.d_hi;
                    const float hh = 3.5f * (float)mk.fs, hw = 0.5f * (float)(mk.bw * mk.fs);
                    const float ty = mk.py - hh, tx = mk.px - hw;
                    mk.oy = (int)floorf(ty + 0.5f);
                    mk.ox = (int)floorf(tx + 0.5f);
#pragma unroll
                    for (int v = 0; v < V; ++v) ov_mark(c[v], y, x + v, mk, a.r_ring, a.r_disc, a.labels, s_glyph);
                }
            }
        }
        const long long pix = ((long long)a.y0 + (long long)(b / a.cols) * (a.H + a.gap) + y) * a.ld + a.x0 +
                              (long long)(b % a.cols) * (a.W + a.gap) + x;
        unsigned char* yo = a.out + pix * 3;
        if (V == 4) {
            unsigned px[12];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                px[3 * v] = ov_u8(c[v][0]);
                px[3 * v + 1] = ov_u8(c[v][1]);
                px[3 * v + 2] = ov_u8(c[v][2]);
            }
            unsigned* yw = (unsigned*)yo;
#pragma unroll
            for (int w = 0; w < 3; ++w) yw[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | (px[4 * w + 3] << 24);
        } else {
            yo[0] = (unsigned char)ov_u8(c[0][0]);
            yo[1] = (unsigned char)ov_u8(c[0][1]);
            yo[2] = (unsigned char)ov_u8(c[0][2]);
        }
    }
}

template <int V>
void ov_launch(const OvArgs& a, int mode, unsigned grid, hipStream_t st) {
    switch (mode) {
        case 0: hipLaunchKernelGGL((skp_overlay_kernel<V, 0>), dim3(grid), dim3(SKP_EW_BLOCK), 0, st, a); break;
        case 1: hipLaunchKernelGGL((skp_overlay_kernel<V, 1>), dim3(grid), dim3(SKP_EW_BLOCK), 0, st, a); break;
        default: hipLaunchKernelGGL((skp_overlay_kernel<V, 2>), dim3(grid), dim3(SKP_EW_BLOCK), 0, st, a); break;
    }
}

int ov_glyph_scale(float radius, int bw) {
    const int fs = (int)((double)radius / (0.5 * sqrt((double)(bw * bw + 49))));
    return fs < 1 ? 1 : fs;
}

}  // namespace

extern "C" int64_t skp_map_range_workspace(int N, int64_t plane) {
    if (N <= 0 || plane <= 0) return SKP_E_BADARG;
    const RangePlan pl = rg_plan(N, plane);
    if ((long long)N * pl.splits > 0x7fffffffLL) return SKP_E_RANGE;
    return pl.splits > 1 ? (int64_t)N * pl.splits * 2 * (int64_t)sizeof(int) : 0;
}

extern "C" int skp_map_range_f32(const float* M, float* range, void* workspace, int N, int64_t plane, void* stream) {
    if (!M || !range || N <= 0 || plane <= 0) return SKP_E_BADARG;
    const RangePlan pl = rg_plan(N, plane);
    if ((long long)N * pl.splits > 0x7fffffffLL) return SKP_E_RANGE;
    if (pl.splits > 1 && !workspace) return SKP_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)N * pl.splits)), block(256);
    if ((plane & 3) == 0 && skp_aligned16(M))
        hipLaunchKernelGGL(skp_map_range_kernel<true>, grid, block, 0, st, M, (int*)workspace, range, (long long)plane, pl.seg, pl.splits);
    else
        hipLaunchKernelGGL(skp_map_range_kernel<false>, grid, block, 0, st, M, (int*)workspace, range, (long long)plane, pl.seg, pl.splits);
    if (pl.splits > 1)
        hipLaunchKernelGGL(skp_map_range_fold_kernel, dim3((unsigned)N), dim3(64), 0, st, (const int*)workspace, range, pl.splits);
    return skp_launch_status();
}

extern "C" int skp_overlay_u8_f32(const float* img, const float* map, const float* range, const float* lut, const float* pts,
                                  const float* colors, const unsigned char* glyphs, unsigned char* out, int B, int H, int W, int S,
                                  int L, int K, float alpha, float radius, float ring, int labels, int ld, int canvas_h, int y0,
                                  int x0, int cols, int gap, void* stream) {
    if (!img || !out || B <= 0 || H <= 0 || W <= 0 || K < 0) return SKP_E_BADARG;
    if (map && (!range || !lut || S <= 0 || L < 2)) return SKP_E_BADARG;
    if (K > 0 && (!pts || !colors || (labels && !glyphs) || !(radius >= 0.f) || !(ring >= 0.f))) return SKP_E_BADARG;
    if (cols < 1 || gap < 0 || y0 < 0 || x0 < 0 || ld < 1 || canvas_h < 1) return SKP_E_BADARG;
    if (H > OV_MAX_SIDE || W > OV_MAX_SIDE || K > OV_MAX_K || (map && (S > OV_MAX_SIDE || L > OV_MAX_L))) return SKP_E_RANGE;
    const long long used_cols = B < cols ? B : cols, rows = ((long long)B + cols - 1) / cols;
    if (x0 + used_cols * ((long long)W + gap) - gap > ld || y0 + rows * ((long long)H + gap) - gap > canvas_h) return SKP_E_BADARG;
    const int mode = !map ? 0 : (S == H && S == W ? 1 : 2);
    const bool vec = (W & 3) == 0 && skp_aligned16(img) && (mode != 1 || skp_aligned16(map)) && ((uintptr_t)out & 3) == 0 &&
                     (ld & 3) == 0 && (x0 & 3) == 0 && (used_cols == 1 || ((W + gap) & 3) == 0);
    OvArgs a;
    a.img = img; a.map = map; a.range = range; a.lut = lut; a.pts = pts; a.colors = colors; a.glyphs = glyphs; a.out = out;
    a.B = B; a.H = H; a.W = W; a.S = map ? S : 1; a.L = map ? L : 2; a.K = K;
    a.alpha = alpha;
    a.r_ring = (float)((double)radius + (double)ring + 0.5);
    a.r_disc = (float)((double)radius + 0.5);
    a.labels = labels ? 1 : 0;
    a.fs1 = ov_glyph_scale(radius, 5);
    a.fs2 = ov_glyph_scale(radius, 11);
    a.ld = ld; a.y0 = y0; a.x0 = x0; a.cols = cols; a.gap = gap;
    const long long lanes = (long long)H * W / (vec ? 4 : 1);
    a.upi = (int)((lanes + SKP_EW_BLOCK - 1) / SKP_EW_BLOCK);
    a.units = (long long)B * a.upi;
    const unsigned grid = skp_capped_grid(a.units * SKP_EW_BLOCK);                  // one workgroup per unit, capped
    hipStream_t st = (hipStream_t)stream;
    if (vec) ov_launch<4>(a, mode, grid, st);
    else ov_launch<1>(a, mode, grid, st);
    return skp_launch_status();
}
