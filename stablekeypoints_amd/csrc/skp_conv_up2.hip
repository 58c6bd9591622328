// Nearest-neighbour 2x up-sampling followed by a 3x3 / stride 1 / padding 1 convolution (diffusers Upsample2D: the VAE decoder's
// three up-samplers and the UNet's three, reached from the sampling loop of ptp_utils.py `text2image_ldm_stable`), forward,
// frozen weights, WITHOUT writing the up-sampled tensor: a direct POLYPHASE implicit GEMM on the fp32 matrix cores.
//
// Every up-sampled pixel repeats a low-resolution one, so the three taps of a row fall on two low-resolution rows only.  With
// output row 2 i + a (a = row phase) and taps w0 w1 w2:
//     a = 0:  rows {i - 1: w0,       i: w1 + w2}          a = 1:  rows {i: w0 + w1,   i + 1: w2}
// and the same along columns: output pixel (2 i + a, 2 j + c) is a 2x2 convolution of the low-resolution input with the phase
// filter F[a][c], window rows i + a - 1 + dr, columns j + c - 1 + dc (dr, dc in {0, 1}; out of range = 0: the zero padding of the
// up-sampled image falls exactly on the low-resolution border).  16 multiplies per four outputs and channel pair = 4 per output
// against 9 for the direct convolution of the up-sampled tensor, whose 4x larger input is never written or read.
//
//   y[b,co,2i+a,2j+c] = bias[co] + sum_{ci,dr,dc} F[a][c][dr][dc][co][ci] * x[b,ci,i+a-1+dr,j+c-1+dc]
//
// GEMM view (the operand order of skp_conv_s2.hip): M = Cout, N = low-resolution pixels, K = (tap, ci); v_mfma_f32_16x16x4_f32,
// k-slot kq = lane >> 4 and MFMA step m contract input channel 4 kq + m of the current 16-channel stage.
//   A  phase filters, folded once per frozen weight in fp64: U[phase 2a+c][tap 2dr+dc][ci/16][kq][co][m] -> one 16-byte load
//   B  input patch in LDS, channel-interleaved [kq][row][col][m]                                          -> one ds_read_b128
// Workgroup = 8 x 16 low-resolution pixels (16 x 32 outputs) x 32 output channels; wave = (row phase a, 16-channel block) x BOTH
// column phases x 8 rows of 16 pixels = 16 accumulator tiles, so a lane ends with the horizontally adjacent outputs (2j, 2j+1)
// of its pixel and stores them as one 8-byte word: 16 lanes write 128 contiguous bytes.  Per 16-channel stage a wave issues 256
// MFMAs for 48 LDS reads and 8 filter loads (fetched one stage ahead); the next stage's 10 x 18 x 16 patch is fetched with 16
// buffer_load_dword per thread (position fixed per thread, channel = scalar offset; out-of-range offsets return 0) while the
// current stage computes.  Ragged tiles: loads are bounded by the image, stores by a dropped offset.  fp32 throughout, no K
// split, no atomics, no workspace: bit-identical from call to call.
#include "skp_common.h"

namespace {

constexpr int UP_TH = 8, UP_TW = 16;                      // low-resolution tile
constexpr int UP_ROWS = UP_TH + 2, UP_COLS = UP_TW + 2;   // 10 x 18 input patch
constexpr int UP_POS = UP_ROWS * UP_COLS;                 // 180 positions per channel (one per thread, 76 threads idle)
constexpr int UP_STAGE = 4 * UP_POS * 4;                  // floats per LDS stage: [kq][pos][m]
static_assert(UP_POS <= 256, "one patch position per thread");

// taps of the 3-tap filter that fall on low-resolution tap d of phase p: (p, d) = (0,0): {0}, (0,1): {1,2}, (1,0): {0,1}, (1,1): {2}
__device__ __forceinline__ double up2_fold1(const double (&t)[3], int p, int d) {
    return p == 0 ? (d == 0 ? t[0] : t[1] + t[2]) : (d == 0 ? t[0] + t[1] : t[2]);
}

__global__ void skp_up2_filter_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Cout * Cin) return;
    const int co = idx / Cin, ci = idx - co * Cin;
    const int c16 = ci >> 4, kq = (ci >> 2) & 3, m = ci & 3, C16 = Cin >> 4;
    const float* p = w + ((size_t)co * Cin + ci) * 9;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int dr = 0; dr < 2; ++dr) {
            double rowf[3];                                 // the three column taps, rows folded
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const double col[3] = {(double)p[s], (double)p[3 + s], (double)p[6 + s]};
                rowf[s] = up2_fold1(col, a, dr);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int dc = 0; dc < 2; ++dc) {
                    const int blk = (a * 2 + c) * 4 + dr * 2 + dc;
                    U[((((size_t)blk * C16 + c16) * 4 + kq) * Cout + co) * 4 + m] = (float)up2_fold1(rowf, c, dc);
                }
        }
}

struct Up2Args {
    const float* x; const float* U; const float* bias; float* y;
    int B, Cin, Cout, H, W;                               // H, W: the LOW-resolution input; the output is 2H x 2W
    int tilesX, tilesPerImg;
    unsigned x_bytes, u_bytes, y_bytes;
};

__global__ __launch_bounds__(256, 2) void skp_conv_up2_kernel(Up2Args a) {
    __shared__ __attribute__((aligned(16))) float xs[2 * UP_STAGE];      // [2][4 kq][180 pos][4 m]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), i16 = lane & 15, kq = lane >> 4;
    const int ra = wave >> 1, mt = wave & 1;              // row phase, 16-channel block of the workgroup's 32 channels
    const int tile = blockIdx.x, cg = blockIdx.y;
    const int b = tile / a.tilesPerImg, rem = tile - b * a.tilesPerImg;
    const int ty = rem / a.tilesX, tx = rem - ty * a.tilesX;
    const int i0 = ty * UP_TH, j0 = tx * UP_TW;
    const int HW = a.H * a.W, OH = 2 * a.H, OW = 2 * a.W;
    const int co0 = cg * 32 + mt * 16;
    const int C16 = a.Cin >> 4;

    // ---- staging role: thread -> one fixed position of the 10 x 18 patch; the channel is a scalar offset ----
    int goff, loff;
    {
        const int row = tid / UP_COLS, col = tid - row * UP_COLS;
        const int iy = i0 + row - 1, ix = j0 + col - 1;
        const bool ok = tid < UP_POS && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        goff = ok ? ((b * a.Cin) * HW + iy * a.W + ix) * 4 : SKP_OOB;
        loff = tid < UP_POS ? tid * 4 : -1;
    }
    const i32x4 xrs = skp_make_rsrc(a.x, a.x_bytes);
    const i32x4 urs = skp_make_rsrc(a.U, a.u_bytes);
    float pre[16];
    auto fetch = [&](int s) {
#pragma unroll
        for (int c = 0; c < 16; ++c) pre[c] = skp_buf_load_f32(xrs, goff, (s * 16 + c) * HW * 4, 0);
    };
    auto put = [&](int buf) {
        if (loff >= 0) {
            float* dst = xs + buf * UP_STAGE + loff;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *(f32x4*)(dst + q * (UP_POS * 4)) = f32x4{pre[4 * q], pre[4 * q + 1], pre[4 * q + 2], pre[4 * q + 3]};
        }
    };

    f32x4 acc[2][UP_TH];                                  // [column phase][row of the tile]
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int nt = 0; nt < UP_TH; ++nt) acc[c][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // filter operand: U[blk = (2 ra + c) * 4 + 2 dr + dc][c16][kq][co][m]; slot f = 4 c + 2 dr + dc of this wave's row phase
    const int uvo = (kq * a.Cout + co0 + i16) * 16;
    const int u_c16 = 4 * a.Cout * 16, u_blk = C16 * u_c16;
    f32x4 ua[8], un[8];
    auto fetch_filters = [&](f32x4 (&dst)[8], int s) {
#pragma unroll
        for (int f = 0; f < 8; ++f) dst[f] = skp_buf_load_f32x4(urs, uvo, ((ra * 2 + (f >> 2)) * 4 + (f & 3)) * u_blk + s * u_c16, 0);
    };

    fetch(0);
    fetch_filters(ua, 0);
    put(0);
    __syncthreads();

    for (int s = 0; s < C16; ++s) {
        if (s + 1 < C16) {
            fetch(s + 1);
            fetch_filters(un, s + 1);
        }
        // patch row of (tile row nt, tap dr) = nt + ra + dr; patch column of (pixel i16, column phase c, tap dc) = i16 + c + dc
        const float* xb = xs + (s & 1) * UP_STAGE + kq * (UP_POS * 4) + (ra * UP_COLS + i16) * 4;
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
            for (int cs = 0; cs < 3; ++cs) {              // cs = c + dc
                f32x4 bv[UP_TH];
#pragma unroll
                for (int nt = 0; nt < UP_TH; ++nt) bv[nt] = *(const f32x4*)(xb + ((nt + dr) * UP_COLS + cs) * 4);
#pragma unroll
                for (int m = 0; m < 4; ++m)                // an accumulator is revisited after >= 7 other MFMAs
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int dc = cs - c;
                        if (dc < 0 || dc > 1) continue;
#pragma unroll
                        for (int nt = 0; nt < UP_TH; ++nt)
                            acc[c][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[c * 4 + dr * 2 + dc][m], bv[nt][m], acc[c][nt], 0, 0, 0);
                    }
            }
        if (s + 1 < C16) {
            put((s + 1) & 1);
#pragma unroll
            for (int f = 0; f < 8; ++f) ua[f] = un[f];
        }
        __syncthreads();
    }

    // ---- epilogue: lane = low-resolution pixel (column j0 + i16 of row i0 + nt), registers = 4 output channels; the two column
    // phases of the pixel are adjacent in the output row 2 i + ra ----
    const i32x4 yrs = skp_make_rsrc(a.y, a.y_bytes);
    const i32x4 brs = skp_make_rsrc(a.bias, a.bias ? (unsigned)a.Cout * 4u : 0u);
    const int j = j0 + i16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = co0 + 4 * kq + r;
        const float bvv = skp_buf_load_f32(brs, co * 4, 0, 0);
        const int base = ((b * a.Cout + co) * OH + 2 * i0 + ra) * OW + 2 * j;
#pragma unroll
        for (int nt = 0; nt < UP_TH; ++nt) {
            const bool ok = j < a.W && i0 + nt < a.H;
            skp_buf_store_f32x2(f32x2{acc[0][nt][r] + bvv, acc[1][nt][r] + bvv}, yrs, ok ? (base + 2 * nt * OW) * 4 : SKP_OOB, 0, 0);
        }
    }
}

// Shapes the kernel can run: whole 16-channel stages, whole 32-channel output blocks, 32-bit byte offsets.  Any H, W.
static bool up2_layout_ok(int B, int Cin, int Cout, int H, int W) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return false;
    if ((Cin % 16) || (Cout % 32)) return false;
    const unsigned long long xb = (unsigned long long)B * Cin * H * W * 4, ub = (unsigned long long)16 * Cin * Cout * 4,
                             yb = (unsigned long long)B * Cout * H * W * 16;
    const unsigned long long tiles = (unsigned long long)B * ((H + UP_TH - 1) / UP_TH) * ((W + UP_TW - 1) / UP_TW);
    return xb < 0x80000000ull && ub < 0x80000000ull && yb < 0x80000000ull && tiles < 0x7fffffffull && Cout / 32 <= 65535;
}

// Where the form pays against F.interpolate + the F(4x4,3x3) Winograd kernels on the up-sampled tensor (tools/conv_up2_bench.py,
// profiles/generate_decoder.md): see the table there.  This direct form does 4 multiplies per output where Winograd on the
// up-sampled tensor does 2.25, and wins only what the skipped interpolate pass and the 4x smaller input are worth.
static bool up2_shape_ok(int B, int Cin, int Cout, int H, int W) {
    (void)B; (void)Cin; (void)Cout; (void)H; (void)W;
    return false;                                         // no measured shape yet: forced only ("conv_up2" = 1)
}

}  // namespace

// 1 where skp_conv3x3_up2_f32 is the route of choice.  skp_tune_set("conv_up2", 1): every shape the kernel can run; 2: none.
extern "C" int skp_conv3x3_up2_ok(int B, int Cin, int Cout, int H, int W) {
    if (!up2_layout_ok(B, Cin, Cout, H, W)) return 0;
    const int force = skp_tune(SKP_TUNE_CONV_UP2);
    if (force) return force == 1 ? 1 : 0;
    return up2_shape_ok(B, Cin, Cout, H, W) ? 1 : 0;
}

// U: 16 * Cin * Cout floats, [4 phases][4 taps][Cin/16][4][Cout][4]
extern "C" int skp_conv3x3_up2_filter_f32(const void* w, void* U, int Cout, int Cin, void* stream) {
    if (!w || !U || Cout <= 0 || Cin <= 0) return SKP_E_BADARG;
    if ((Cin & 15) || (unsigned long long)16 * Cin * Cout * 4 >= 0x80000000ull) return SKP_E_RANGE;
    const int n = Cout * Cin;
    hipLaunchKernelGGL(skp_up2_filter_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)w, (float*)U,
                       Cout, Cin);
    return skp_launch_status();
}

extern "C" int skp_conv3x3_up2_f32(const void* x, const void* U, const void* bias, void* y, int B, int Cin, int Cout, int H, int W,
                                   void* stream) {
    if (!x || !U || !y || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return SKP_E_BADARG;
    if (!up2_layout_ok(B, Cin, Cout, H, W)) return SKP_E_RANGE;
    Up2Args a;
    a.x = (const float*)x; a.U = (const float*)U; a.bias = (const float*)bias; a.y = (float*)y;
    a.B = B; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.tilesX = (W + UP_TW - 1) / UP_TW;
    a.tilesPerImg = a.tilesX * ((H + UP_TH - 1) / UP_TH);
    a.x_bytes = (unsigned)((size_t)B * Cin * H * W * 4);
    a.u_bytes = (unsigned)((size_t)16 * Cin * Cout * 4);
    a.y_bytes = (unsigned)((size_t)B * Cout * H * W * 16);
    hipLaunchKernelGGL(skp_conv_up2_kernel, dim3((unsigned)(B * a.tilesPerImg), Cout / 32, 1), dim3(256), 0, (hipStream_t)stream, a);
    return skp_launch_status();
}
