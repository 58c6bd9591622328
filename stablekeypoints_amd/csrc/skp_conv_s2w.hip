// 3x3 / stride 2 convolution (forward, asymmetric (0,1,0,1) zero extension: the VAE's Downsample2D) as a POLYPHASE Winograd
// F(4x4,2x2) on the fp32 matrix cores.  The direct form (skp_conv_s2.hip) runs near its MFMA limit; what is left to remove
// are multiplies.  Split the input into its four pixel phases.  In 1-D, with base = 2 i:
//     y[i] = w0 x[2i] + w1 x[2i+1] + w2 x[2i+2] = (w0, w2) * A[i .. i+1] + (w1, 0) * B[i .. i+1],   A[k] = x[2k], B[k] = x[2k+1]
// so in 2-D the phases (rp, cp) see 2x2, 2x1, 1x2 and 1x1 filters: ONE stride-1 2x2 convolution over 4 Cin channels at the
// output resolution.  F(4x4,2x2) (points 0, 1, -1, 2, inf; 5x5 tiles) makes 16 outputs from 25 multiplies per channel: 100 per
// original channel against 144 direct.  The inf row of G picks a filter's LAST tap, which is the structural zero of the one-tap
// phases: their transformed filters vanish at row (rp = 1) / column (cp = 1) 4, so only 25 + 20 + 20 + 16 = 81 of the 100
// (position, phase) blocks are multiplied at all (and the input rows / columns that only those blocks read are not loaded).
//
//   Y = A^T [ sum_{phase, ci} (G g G^T) (.) (B^T d B) ] A          d = 5x5 patch of one phase, g = that phase's 2x2 filter
//
// Kernel: the 128-channel form of skp_conv_wino4.hip (skp_wino4_conv_c128_kernel) with 25 positions instead of 36: workgroup =
// 128 output channels x 16 tiles of 4x4 outputs, one wave per SIMD, wave = 32 channels x 16 tiles x 25 positions = 200 named
// AGPR accumulators (skp_wino4_common.h; all of them fit the AGPR file), v_mfma_f32_16x16x4_f32, persistent work ids in
// w4_work's XCD-banded order.  A STAGE is 16 input channels of one phase; the four stages of a 16-channel group run in the
// order (rp,cp) = (0,1) (0,0) (1,1) (1,0): one contiguous row load serves both column phases, so a thread loads the 5 (4) rows
// of a row phase of its (tile, channel) once, transforms them vertically on column PAIRS (packed fp32), and the horizontal pass
// of each column phase feeds one stage -- all of it as side jobs of the MFMA loop of the stage before (the row loads and the
// vertical pass ride on the larger stage of each row phase).  The transformed filter is stored in exactly the order the loop
// consumes it, U[Cin/16][81 blocks][kq][Cout][m], and streamed from L2 through a register ring.
// Zero padding = out-of-range buffer loads; fp32 throughout; no K split, no atomics, no workspace: bit-identical from call to call.
#include <algorithm>
#include "skp_common.h"
#include "skp_wino4_common.h"
#include <stdlib.h>

namespace {

#ifdef S2W_ALL_BLOCKS                               // lab builds only: multiply the 19 structurally zero blocks too (A/B of the skip)
constexpr bool S2W_SKIP = false;
#else
constexpr bool S2W_SKIP = true;
#endif

// stage k of a channel group: row phase k >> 1, column phase 1 - (k & 1); a one-tap phase has 4 non-zero rows / columns
constexpr int s2w_rp(int k) { return k >> 1; }
constexpr int s2w_cp(int k) { return 1 - (k & 1); }
constexpr int s2w_ni(int k) { return (S2W_SKIP && s2w_rp(k)) ? 4 : 5; }
constexpr int s2w_nj(int k) { return (S2W_SKIP && s2w_cp(k)) ? 4 : 5; }
constexpr int s2w_np(int k) { return s2w_ni(k) * s2w_nj(k); }
constexpr int s2w_e0(int k) { return k == 0 ? 0 : s2w_e0(k - 1) + s2w_np(k - 1); }
constexpr int S2W_NE = s2w_e0(3) + s2w_np(3);      // blocks per 16-channel group: 81 (100)
constexpr int S2W_RING = S2W_SKIP ? 9 : 10;        // filter ring slots (divides S2W_NE) ...
constexpr int S2W_D = 6;                           // ... filled this many blocks ahead of their use
constexpr int S2W_STAGE_F4 = 25 * 4 * 16;          // f32x4 per LDS stage: [block of the stage][4 k-quads][16 tiles]
static_assert(S2W_NE % S2W_RING == 0 && S2W_D < S2W_RING, "ring");

// ---- filter transform: G g G^T of the four phase filters in fp64, rounded once; blocks in consumption order ----
__global__ void skp_s2w_filter_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Cout * Cin) return;
    const int co = idx / Cin, ci = idx - co * Cin;
    const float* p = w + ((size_t)co * Cin + ci) * 9;
    const double G[5][2] = {{0.5, 0.0}, {-0.5, -0.5}, {-1.0 / 6, 1.0 / 6}, {1.0 / 6, 1.0 / 3}, {0.0, 1.0}};
    const int c16 = ci >> 4, kq = (ci >> 2) & 3, m = ci & 3;
    float* dst = U + ((((size_t)c16 * S2W_NE) * 4 + kq) * Cout + co) * 4 + m;
    const size_t blk = (size_t)16 * Cout;           // floats per block
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int rp = s2w_rp(k), cp = s2w_cp(k);
        // taps of the phase: the two-tap phase sees (w0, w2), the one-tap phase (w1, 0)
        double g[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const bool nz = (rp == 0 || a == 0) && (cp == 0 || b == 0);
                const int ra = rp == 0 ? 2 * a : 1, cb = cp == 0 ? 2 * b : 1;
                g[a][b] = nz ? (double)p[ra * 3 + cb] : 0.0;
            }
        double t[5][2];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int b = 0; b < 2; ++b) t[i][b] = G[i][0] * g[0][b] + G[i][1] * g[1][b];
        int e = s2w_e0(k);
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (i >= s2w_ni(k) || j >= s2w_nj(k)) continue;      // structural zero (by phase and position, not by value)
                dst[(size_t)e * blk] = (float)(t[i][0] * G[j][0] + t[i][1] * G[j][1]);
                ++e;
            }
    }
}

// B^T applied to a 5-vector, N outputs (N = 4: a one-tap phase -- neither t[4] nor d[4] exist)
template <int N, class T>
__device__ __forceinline__ void s2w_in1d(const T (&d)[5], T (&t)[5]) {
    const T a = d[3] - d[1];
    t[0] = 2.f * (d[0] - d[2]) + a;
    t[1] = a - (d[1] + d[2]);
    t[2] = 3.f * (d[1] - d[2]) + a;
    t[3] = a;
    if (N == 5) t[4] = (d[4] - d[2]) - 2.f * a;
}
// A^T applied to a 5-vector
__device__ __forceinline__ void s2w_out1d(const float (&m)[5], float (&y)[4]) {
    const float s12 = m[1] + m[2], d12 = m[1] - m[2];
    y[0] = m[0] + s12 + m[3];
    y[1] = d12 + 2.f * m[3];
    y[2] = s12 + 4.f * m[3];
    y[3] = d12 + 8.f * m[3] + m[4];
}

// accumulator tuple T = 2 * position + channel block, position = 5 i + j, in a[4T : 4T + 3]
template <int P, int CB>
__device__ __forceinline__ void s2w_mfma(float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 a[%0:%1], %2, %3, a[%0:%1]" : : "n"(4 * (2 * P + CB)), "n"(4 * (2 * P + CB) + 3), "v"(a), "v"(b) : W4_AGPR_CLOBBERS);
}

// a.H / a.W: INPUT size; tiles are 4x4 OUTPUT pixels (8x8 input pixels, 10x10 window); a.total_steps = Cin / 16 channel groups
template <bool STATS>
__global__ __launch_bounds__(256, 1) void skp_s2w_conv_kernel(Wino4Args a) {
    extern __shared__ f32x4 vst[];                   // [2][25][4][16] stage buffers, then [32][64] float2 statistics slots
    f32x2* const sst = (f32x2*)(vst + 2 * S2W_STAGE_F4);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    const int HW = a.H * a.W, OH = a.H >> 1, OW = a.W >> 1, OHW = OH * OW;
    int tblock, cg, zsplit;
    int wid = blockIdx.x;
    while (wid < a.vtotal && !w4_work(a, wid, tblock, cg, zsplit)) wid += gridDim.x;
    if (wid >= a.vtotal) return;

    // ---- transform role: the window of one channel of one tile ----
    const int tl = tid & 15, tc = tid >> 4;          // tile in the block, channel in the group
    int vA, vC, vA8, vC8;                            // byte offsets of window (row 0, col 0) / (row 0, col 8) for rows 0-7 / rows 8-9, or SKP_OOB
    auto aim_transform = [&](int tb, bool valid) {   // point the transform role at tile block tb (nothing: every load returns 0)
        const int tg = tb * 16 + tl;
        const bool tv = valid && tg < a.nTiles;
        const int tgc = tv ? tg : 0;
        const int b = tgc / a.tilesPerImg, rem = tgc - b * a.tilesPerImg;
        const int ty = rem / a.tilesX, tx = rem - ty * a.tilesX;
        const int pbase = (((b * a.Cin + tc) * a.H + 8 * ty) * a.W + 8 * tx) * 4;
        const bool r8 = 8 * ty + 8 < a.H, c8 = 8 * tx + 8 < a.W;   // else: the zero extension
        vA = tv ? pbase : SKP_OOB;
        vC = (tv && c8) ? pbase + 32 : SKP_OOB;
        vA8 = (tv && r8) ? pbase : SKP_OOB;
        vC8 = (tv && r8 && c8) ? pbase + 32 : SKP_OOB;
    };
    aim_transform(tblock, true);
    const i32x4 xrs = skp_make_rsrc(a.x, a.x_bytes);
    const i32x4 urs = skp_make_rsrc(a.U, a.u_bytes);
    const i32x4 brs = skp_make_rsrc(a.bias, a.bias ? (unsigned)a.Cout * 4u : 0u);
    const i32x4 yrs = skp_make_rsrc(a.y, a.y_bytes);
    f32x2 d[5][5];                                   // [row of the row phase][column pair (2c, 2c+1)]; pair 4 = (col 8, -)
    auto load_row = [&](int cin0, int rp, int k) {   // window row 2 k + rp of channel cin0 + tc
        const int row = 2 * k + rp;
        const int so = (cin0 * HW + row * a.W) * 4;
        const int va = row >= 8 ? vA8 : vA, vc = row >= 8 ? vC8 : vC;
        const f32x4 m0 = skp_buf_load_f32x4(xrs, va, so, 0);
        const f32x4 m1 = skp_buf_load_f32x4(xrs, va + 16, so, 0);
        const float c8 = skp_buf_load_f32(xrs, vc, so, 0);
        d[k][0] = f32x2{m0[0], m0[1]};
        d[k][1] = f32x2{m0[2], m0[3]};
        d[k][2] = f32x2{m1[0], m1[1]};
        d[k][3] = f32x2{m1[2], m1[3]};
        d[k][4] = f32x2{c8, 0.f};
    };
    auto col_pass = [&](int c, auto ni_c) {          // d[:, pair c] <- B^T d[:, pair c]   (vertical pass, both column phases at once)
        constexpr int NI = decltype(ni_c)::value;
        f32x2 v[5], t[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = d[i][c];
        s2w_in1d<NI>(v, t);
#pragma unroll
        for (int i = 0; i < NI; ++i) d[i][c] = t[i];
    };
    auto row_pass_store = [&](int buf, int i, int cp, auto nj_c) {   // blocks (i, 0 .. NJ-1) of column phase cp
        constexpr int NJ = decltype(nj_c)::value;
        float r[5] = {d[i][0][cp], d[i][1][cp], d[i][2][cp], d[i][3][cp], d[i][4][cp]};
        float t[5];
        s2w_in1d<NJ>(r, t);
        float* dst = (float*)(vst + buf * S2W_STAGE_F4) + (((i * NJ) * 4 + (tc >> 2)) * 16 + tl) * 4 + (tc & 3);
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[j * (4 * 16 * 4)] = t[j];
    };

    // first unit: its first stage the plain way (afterwards d holds the vertically transformed rows for the second stage)
    {
        constexpr int NI = s2w_ni(0), NJ = s2w_nj(0);
#pragma unroll
        for (int k = 0; k < NI; ++k) load_row(0, 0, k);
#pragma unroll
        for (int c = 0; c < 5; ++c) col_pass(c, std::integral_constant<int, NI>{});
#pragma unroll
        for (int i = 0; i < NI; ++i) row_pass_store(0, i, s2w_cp(0), std::integral_constant<int, NJ>{});
    }

    const int u_blk = 4 * a.Cout * 16;               // bytes per block
    const int nsteps = a.total_steps;

    for (;;) {
        const int tile0 = tblock * 16;
        const int n0 = (cg * 4 + wave) * 32;         // this wave's 32 output channels (two 16-row MFMA blocks)
        int uvo[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) uvo[cb] = (kq * a.Cout + n0 + cb * 16 + i16) * 16;
        f32x4 ua[S2W_RING][2];
#pragma unroll
        for (int q = 0; q < S2W_D; ++q)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) ua[q][cb] = skp_buf_load_f32x4(urs, uvo[cb], q * u_blk, 0);

        // the unit after this one
        int wnext = wid + gridDim.x, tb_n = 0, cg_n = 0, z_n = 0;
        while (wnext < a.vtotal && !w4_work(a, wnext, tb_n, cg_n, z_n)) wnext += gridDim.x;
        const bool has_next = wnext < a.vtotal;

        w4_unroll([&](auto rc) { asm volatile("v_accvgpr_write_b32 a[%0], 0" : : "n"(decltype(rc)::value) : W4_AGPR_CLOBBERS); },
                  std::make_integer_sequence<int, 200>{});
        __syncthreads();

        // MODE 0: a channel group of the unit with another one behind it; MODE 1: the unit's last group -- the side jobs of its last
        // stage work on the first stage of the NEXT unit (the transform role is retargeted before that stage; nothing -> zeros)
        auto run_group = [&](int s, auto mode_c) {
            constexpr int MODE = decltype(mode_c)::value;
            const int ub = s * S2W_NE * u_blk;
            w4_unroll([&](auto kc) {
                constexpr int k = decltype(kc)::value, kn = (k + 1) & 3;
                constexpr int NJ = s2w_nj(k), NP = s2w_np(k), E0 = s2w_e0(k);
                constexpr int NIn = s2w_ni(kn), NJn = s2w_nj(kn);
                constexpr bool heavy = (k & 1) == 1;     // the next stage starts a row phase: load its rows, vertical pass
                if (MODE == 1 && k == 3) aim_transform(tb_n, has_next);
                const int cin_side = k == 1 ? s * 16 : (MODE == 0 ? (s + 1) * 16 : 0);
                const f32x4* vb = vst + (k & 1) * S2W_STAGE_F4 + kq * 16 + i16;
                f32x4 va[3];                             // LDS operands two blocks ahead
                va[0] = vb[0];
                va[1] = vb[64];
                w4_unroll([&](auto ec) {
                    constexpr int e = decltype(ec)::value, p = 5 * (e / NJ) + (e % NJ);
                    {   // filter operands S2W_D blocks ahead (the layout is the consumption order: the next group simply follows)
                        constexpr int q = E0 + e + S2W_D;
                        if (MODE == 0 || q < S2W_NE) {
#pragma unroll
                            for (int cb = 0; cb < 2; ++cb) ua[q % S2W_RING][cb] = skp_buf_load_f32x4(urs, uvo[cb], ub + q * u_blk, 0);
                        }
                    }
                    if constexpr (heavy && e < NIn) load_row(cin_side, s2w_rp(kn), e);
                    else if constexpr (heavy && e >= NP - NIn - 5 && e < NP - NIn) col_pass(e - (NP - NIn - 5), std::integral_constant<int, NIn>{});
                    else if constexpr (e >= NP - NIn) row_pass_store((k + 1) & 1, e - (NP - NIn), s2w_cp(kn), std::integral_constant<int, NJn>{});
                    if (e + 2 < NP) va[(e + 2) % 3] = vb[(e + 2) * 64];
                    w4_unroll([&](auto mc) {
                        constexpr int m = decltype(mc)::value;
                        s2w_mfma<p, 0>(ua[(E0 + e) % S2W_RING][0][m], va[e % 3][m]);
                        s2w_mfma<p, 1>(ua[(E0 + e) % S2W_RING][1][m], va[e % 3][m]);
                    }, std::make_integer_sequence<int, 4>{});
                    __builtin_amdgcn_sched_barrier(0);
                }, std::make_integer_sequence<int, NP>{});
                if (!(MODE == 1 && k == 3)) __syncthreads();
            }, std::make_integer_sequence<int, 4>{});
        };
        for (int s = 0; s + 1 < nsteps; ++s) run_group(s, std::integral_constant<int, 0>{});
        run_group(nsteps - 1, std::integral_constant<int, 1>{});

        // ---- epilogue: output role (lane = tile of the block, registers = 4 output channels per channel block) ----
        int o_base;
        bool t_ok;
        {
            const int tg = tile0 + i16;
            t_ok = tg < a.nTiles;
            const int tgc = t_ok ? tg : 0;
            const int b = tgc / a.tilesPerImg, rem = tgc - b * a.tilesPerImg;
            const int ty = rem / a.tilesX, tx = rem - ty * a.tilesX;
            o_base = ((b * a.Cout) * OH + 4 * ty) * OW + 4 * tx;
        }
        float bvs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) bvs[e] = skp_buf_load_f32(brs, (n0 + (e >> 2) * 16 + 4 * kq + (e & 3)) * 4, 0, 0);
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // the last MFMAs' results are in the register file before the first read
        __builtin_amdgcn_sched_barrier(0);
        w4_unroll([&](auto ec) {
            constexpr int e = decltype(ec)::value, cb = e >> 2, r = e & 3;
            const int co = n0 + cb * 16 + 4 * kq + r;
            const int vo = (o_base + co * OHW) * 4;
            const float bv = bvs[e];
            float t[5][4];                           // T = M A : rows of the 5x5 tile -> 4 columns
            w4_unroll([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                float m[5];
                w4_unroll([&](auto jc) { constexpr int j = decltype(jc)::value; m[j] = w4_acc_read<4 * (2 * (5 * i + j) + cb) + r>(); },
                          std::make_integer_sequence<int, 5>{});
                s2w_out1d(m, t[i]);
            }, std::make_integer_sequence<int, 5>{});
            f32x4 o[4];
#pragma unroll
            for (int ox = 0; ox < 4; ++ox) {
                float m[5], yv[4];
#pragma unroll
                for (int i = 0; i < 5; ++i) m[i] = t[i][ox];
                s2w_out1d(m, yv);
#pragma unroll
                for (int oy = 0; oy < 4; ++oy) o[oy][ox] = yv[oy] + bv;
            }
#pragma unroll
            for (int oy = 0; oy < 4; ++oy) skp_buf_store_f32x4(o[oy], yrs, t_ok ? vo + oy * OW * 4 : SKP_OOB, 0, 0);
            if (STATS) w4_park_stats(sst, wave * 8 + e, lane, o, t_ok);
            __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, 8>{});
        if (STATS) {                                 // 128 channels of one tile block
            __syncthreads();
            if (tid < 128) {
                const int wv = tid >> 5, lc = tid & 31;
                w4_store_stats(a, sst, wv * 8 + ((lc >> 4) << 2) + (lc & 3), (lc >> 2) & 3, tile0, (cg * 4 + wv) * 32 + lc);
            }
        }
        if (!has_next) break;
        wid = wnext; tblock = tb_n; cg = cg_n; zsplit = z_n;
    }
}

// Shapes the kernel can run: the VAE's padding, whole channel groups, whole 4x4 output tiles, 32-bit byte offsets.
static bool s2w_layout_ok(int B, int Cin, int Cout, int H, int W, int pad) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || pad != 0) return false;
    if ((Cin % 16) || (Cout % 128) || (H % 8) || (W % 8)) return false;
    const unsigned long long xb = (unsigned long long)B * Cin * H * W * 4, ub = (unsigned long long)S2W_NE * Cin * Cout * 4,
                             yb = (unsigned long long)B * Cout * (H / 2) * (W / 2) * 4;
    return xb < 0x80000000ull && ub < 0x80000000ull && yb < 0x80000000ull;
}

// Where the form pays (tools/conv_s2w_bench.py, profiles/r07_conv_s2w.md; same process, interleaved rounds, median us with the
// statistics epilogue, direct -> this kernel, Cin = Cout, pad 0): a launch of at least one work unit (16 tiles x 128 channels)
// per CU.
//   units >= 256:  128 @512^2  1 row  178 -> 109,  2 rows 340 -> 219,  4 rows 661 -> 436,  8 rows 1300 -> 870
//                  256 @256^2  2 rows 334 -> 193,  4 rows 649 -> 403,  8 rows 1263 -> 815
//                  512 @128^2  4 rows 621 -> 374,  8 rows 1265 -> 801                                  (0.58 .. 0.67 of the direct time)
//   units <  256:  256 @256^2  1 row  188 -> 180 (128 units);  512 @128^2  1 row 365 -> 357 (64), 2 rows 387 -> 368 (128):
//                  0.95 .. 0.98, inside or next to the run-to-run spread -- part of the chip idles either way; those stay direct.
// Below 128 input channels nothing was measured (a unit is then shorter than its prologue + epilogue): direct.
static bool s2w_shape_ok(int B, int Cin, int Cout, int H, int W) {
    const long long units = (((long long)B * (H / 8) * (W / 8) + 15) / 16) * (Cout / 128);
    return Cin >= 128 && units >= 256;
}

}  // namespace

// 1 where skp_conv3x3_s2w_f32 is the faster stride-2 kernel.  skp_tune_set("conv_s2w", 1): every shape the kernel can run;
// 2: none (tests, A/B runs).  Symmetric padding 1 (the UNet's layers: small K-split grids, with gradients) stays on the direct kernel.
extern "C" int skp_conv3x3_s2w_ok(int B, int Cin, int Cout, int H, int W, int pad) {
    if (!s2w_layout_ok(B, Cin, Cout, H, W, pad)) return 0;
    const int force = skp_tune(SKP_TUNE_CONV_S2W);
    if (force) return force == 1 ? 1 : 0;
    return s2w_shape_ok(B, Cin, Cout, H, W) ? 1 : 0;
}

// U: 81 * Cin * Cout floats, [Cin/16][81][4][Cout][4].  pad selects which pixel phase is the two-tap one (0: even, 1: odd,
// shifted); the transformed filter is the same for both, so only its range is checked.
extern "C" int skp_conv3x3_s2w_filter_f32(const void* w, void* U, int Cout, int Cin, int pad, void* stream) {
    if (!w || !U || Cout <= 0 || Cin <= 0 || (pad != 0 && pad != 1)) return SKP_E_BADARG;
    if ((Cin & 15) || (unsigned long long)S2W_NE * Cin * Cout * 4 >= 0x80000000ull) return SKP_E_RANGE;
    const int n = Cout * Cin;
    hipLaunchKernelGGL(skp_s2w_filter_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)w, (float*)U,
                       Cout, Cin);
    return skp_launch_status();
}

static int s2w_run(const void* x, const void* U, const void* bias, void* y, float* stats, int B, int Cin, int Cout, int H, int W,
                   int pad, void* stream) {
    if (!x || !U || !y || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (pad != 0 && pad != 1)) return SKP_E_BADARG;
    if (!s2w_layout_ok(B, Cin, Cout, H, W, pad)) return SKP_E_RANGE;
    Wino4Args a = {};
    a.x = (const float*)x; a.U = (const float*)U; a.bias = (const float*)bias; a.y = (float*)y;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.tilesX = W / 8;
    a.tilesPerImg = a.tilesX * (H / 8);
    a.nTiles = B * a.tilesPerImg;
    if (stats && (a.tilesPerImg % 16)) return SKP_E_RANGE;      // statistics blocks (16 tiles) must not straddle images
    a.x_bytes = (unsigned)((size_t)B * Cin * H * W * 4);
    a.u_bytes = (unsigned)((size_t)S2W_NE * Cin * Cout * 4);
    a.y_bytes = (unsigned)((size_t)B * Cout * (H / 2) * (W / 2) * 4);
    a.total_steps = a.steps = Cin / 16;
    a.splits = 1;
    a.stats = stats;
    a.sblk = a.tilesPerImg / 16;
    a.ntb = (a.nTiles + 15) / 16;
    a.ncg = Cout / 128;
    a.tb_per_xcd = a.ntb >= 64 ? (a.ntb + 7) / 8 : 0;           // work order: see w4_work
    a.gx = a.tb_per_xcd ? 8 * a.tb_per_xcd * a.ncg : 8 * ((a.ncg + 7) / 8) * a.ntb;
    a.vtotal = a.gx;
    const size_t lds = (size_t)2 * S2W_STAGE_F4 * sizeof(f32x4) + 32 * 64 * sizeof(f32x2);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute((const void*)skp_s2w_conv_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        e = hipFuncSetAttribute((const void*)skp_s2w_conv_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    static const int persist = [] {                 // one workgroup per CU of this device
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 256;
        return ncu;
    }();
    // persistent workgroups: the ids are multiples of 8 apart, so a workgroup stays on its XCD's band
    const dim3 grid((unsigned)(persist >= 8 ? std::min(a.vtotal, persist & ~7) : a.vtotal), 1, 1);
    if (stats) hipLaunchKernelGGL(skp_s2w_conv_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(skp_s2w_conv_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
    return skp_launch_status();
}

extern "C" int skp_conv3x3_s2w_f32(const void* x, const void* U, const void* bias, void* y, int B, int Cin, int Cout, int H, int W,
                                   int pad, void* stream) {
    return s2w_run(x, U, bias, y, nullptr, B, Cin, Cout, H, W, pad, stream);
}

// + stats [B][Cout][(H/8)*(W/8)/16][2]: {mean, sum of squared deviations} of y over each block of 16 consecutive 4x4 tiles
extern "C" int skp_conv3x3_s2w_stats_f32(const void* x, const void* U, const void* bias, void* y, float* stats, int B, int Cin,
                                         int Cout, int H, int W, int pad, void* stream) {
    if (!stats) return SKP_E_BADARG;
    return s2w_run(x, U, bias, y, stats, B, Cin, Cout, H, W, pad, stream);
}
