// Causal self-attention forward of the CLIP text towers: N <= 128 tokens, heads of 32 or 64 channels, exact fp32 products on the
// fp32 matrix cores (v_mfma_f32_32x32x2_f32), the staging and product pieces of skp_cross_attn.hip (skp_attn_tiles.h).
//
//   out[b,i,h*d+c] = sum_{j<=i} softmax_{j<=i}(scale q[b,i,h,:].k[b,j,h,:]) v[b,j,h*d+c]
//
// One workgroup of four waves = one (batch, head); wave w owns the queries 32w .. 32w+31.  K (then V) of the head is staged once in
// LDS ([t][d+4]).  S^T = K.Q^T puts query i = lane&31 in a lane and its keys in the lane's accumulator registers (+ the partner
// lane^32), so the causal mask is a compare of the register's key index with the lane's query index BEFORE the row maximum, and the
// softmax stays in registers; the probabilities are then the A operand of P.V.  Key 0 is visible to every row, so the row sum is
// >= 1 (row 0: exactly the one term exp2(0)) and the division is safe.  Rows of K / V beyond N are staged as zeros and masked.
//
// The mask saves no work: every wave with queries runs both products and the exponentials over all ceil(N/32) key tiles, also those
// wholly in its masked future (wave 0 needs one of up to four).  An encode is launch-bound (profiles/text_encoder.md), and a
// per-wave tile bound needs product loops of its own instead of the shared helpers; it is not built.
//
// q, k, v are read with a row stride `ld` floats: three column bands of one stacked [B*N, 3*H*d] projection output need no split
// copy.  No log-sum-exp output and no backward: the towers are frozen and run without gradients.
#include "skp_attn_tiles.h"

template <int D8, int TT>
__global__ __launch_bounds__(256) void skp_text_attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                const float* __restrict__ v, float* __restrict__ out,
                                                                int H, int N, int ld, float scale) {
    using S = CAShape<D8, TT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, hi = lane >> 5;
    const int h = blockIdx.x, b = blockIdx.y, C = H * S::D;
    const int n0 = wave * 32;
    const bool active = n0 < N;                                // (wave-uniform; a wave without queries only helps staging)
    const int nq = n0 + i < N ? n0 + i : N - 1;                // query row of this lane, clamped: lanes past N repeat row N-1
    const size_t base = (size_t)b * N * ld + (size_t)h * S::D;
    ca_stage<D8, TT>(smem, k + base, N, ld, tid);
    __syncthreads();
    f32x16 acc[TT];
    if (active) {
        const float* qrow = q + base + (size_t)nq * ld;
        const float sl2 = scale * SKP_LOG2E;
        f32x4 qv[D8];
#pragma unroll
        for (int j = 0; j < D8; ++j) qv[j] = *(const f32x4*)(qrow + 8 * j + 4 * hi) * sl2;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] = 0.f;
        ca_swapped_product<D8, TT>(smem, qv, acc, i, hi);
        float m = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (ca_tok(tt, r, hi) > nq) acc[tt][r] = -INFINITY;    // future keys (and, as nq < N, the zero rows past N)
                m = fmaxf(m, acc[tt][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                   // key 0 sits in the hi = 0 half: finite for every row
        float l = 0.f;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[tt][r] = __builtin_amdgcn_exp2f(acc[tt][r] - m); l += acc[tt][r]; }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tt][r] *= inv;
    }
    __syncthreads();                                           // everyone done with K
    ca_stage<D8, TT>(smem, v + base, N, ld, tid);
    __syncthreads();
    if (active) {
        f32x16 o[S::CT];
        ca_reg_product<D8, TT>(smem, acc, o, i, hi);
#pragma unroll
        for (int ct = 0; ct < S::CT; ++ct) {
            const int c = ct * 32 + i;                         // (d = 32 / 64: whole channel tiles)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = n0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (nn < N) out[((size_t)b * N + nn) * C + h * S::D + c] = o[ct][r];
            }
        }
    }
}

extern "C" int skp_text_attn_fwd_ok(int B, int H, int N, int d, int ld) {
    if (B <= 0 || H <= 0 || N <= 0 || d <= 0 || ld <= 0) return 0;
    if (N > 128 || (d != 32 && d != 64) || B > 65535 || H > 65535) return 0;
    return (int64_t)ld >= (int64_t)H * d && ld % 4 == 0;
}

#define SKP_TA_CASE(D8V, TTV)                                                                              \
    if (d == D8V * 8 && tt == TTV) {                                                                       \
        const size_t lds = CAShape<D8V, TTV>::LDS_FLOATS * sizeof(float);                                  \
        hipLaunchKernelGGL((skp_text_attn_fwd_kernel<D8V, TTV>), dim3(H, B), dim3(256), lds, (hipStream_t)stream,  \
                           q, k, v, out, H, N, ld, scale);                                                 \
        return skp_launch_status();                                                                        \
    }

extern "C" int skp_text_attn_fwd_f32(const float* q, const float* k, const float* v, float* out,
                                     int B, int H, int N, int d, int ld, float scale, void* stream) {
    if (!q || !k || !v || !out || B <= 0 || H <= 0 || N <= 0 || d <= 0 || ld <= 0) return SKP_E_BADARG;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) != 0) return SKP_E_BADARG;
    if (!skp_text_attn_fwd_ok(B, H, N, d, ld)) return SKP_E_RANGE;
    const int tt = (N + 31) / 32;                              // 1 .. 4 key tiles; <= 128 x 68 floats of LDS
    SKP_TA_CASE(4, 1) SKP_TA_CASE(4, 2) SKP_TA_CASE(4, 3) SKP_TA_CASE(4, 4)
    SKP_TA_CASE(8, 1) SKP_TA_CASE(8, 2) SKP_TA_CASE(8, 3) SKP_TA_CASE(8, 4)
    return SKP_E_RANGE;
}
