// Flash attention FORWARD for one wide head, d = 512 (the VAE mid-block's AttentionBlock):  out = softmax(scale q k^T) v,
// fp32 in / out, exact fp32 products (v_mfma_f32_16x16x4_f32), fp32 online softmax, scores never written to memory.
//
// Shape of the kernel.  A query row owns 512 output channels, so nothing like skp_flash_attn.hip's "Q and O of 32 queries in one
// wave" fits.  Here a workgroup of 4 waves (one per SIMD, 512 registers per lane each) takes 64 queries and EVERY WAVE OWNS 16
// OF THEM WHOLE: its lanes hold those 16 query rows (16 x 512 fp32 = 128 registers) and their 16 x 512 output accumulator (128
// registers).  The four waves share nothing but the K / V tiles in LDS, so there is no cross-wave reduction of S and no P
// exchange, and one barrier per key tile.
//
//   key tile    16 keys: K and V tile 32 KB each, two buffers = 128 KB LDS.  Tile t+1 goes global -> LDS by DMA (no staging
//               registers: the lanes are full) while tile t is computed: 64 pieces of 1 KB (half a key row), 16 per wave.
//   S^T = K Q^T A = K (row = key, lane & 15), B = Q^T (column = query, lane & 15); lane (g = lane >> 4, c = lane & 15) ends with
//               S[query c][keys 4g .. 4g+3].  The 512-channel sum runs in the order the lanes read K: ds_read_b128 gives lane
//               (g, c) channels 16j + 4g .. +3 of key c, four MFMA k-steps; the Q registers hold the same channels.
//               The K image is XOR-swizzled in 16-byte slots (slot ^ key) so that the 16 rows of one read hit 16 different slots.
//   softmax     row maximum over the lane's 4 keys and over g (two shuffles); the row sum stays per lane until the end.
//   O += P V    A = P with k-step r taking key 4g + r: exactly register r of the S^T result, no lane movement; B = V rows
//               4g + r, ds_read_b128 of channels 64t + 4c .. +3, one MFMA each into tiles (t, 0..3).  Tile (t, i) column c is
//               channel 64t + 4c + i, so a lane's four tiles of one t are four consecutive channels: float4 stores.
//               O is held as [query 4g + r][channel column c]; its rescale factor comes from lane 4g + r by shuffle.
//
// Keys past the row's end are staged from the last real row (nothing is read past the tensor) and their logit is set to -inf, so
// their weight is exactly 0; queries past the end are zero rows that are never stored.  The first tile always holds a real key, so the running maximum is finite from the first update on and no exp sees
// inf - inf.
#include "skp_common.h"

#define FAW_D 512
#define FAW_BQ 64                         /* queries per workgroup, 16 per wave */
#define FAW_BK 16                         /* keys per tile */
#define FAW_ROW (FAW_D * 4)               /* bytes of one key row in LDS */
#define FAW_TILE (FAW_BK * FAW_ROW)       /* 32 KB */
#define FAW_LDS (4 * FAW_TILE)            /* [2 buffers][K | V] */

// LDS DMA of one tile: piece (key row kr, half hf) = 64 slots of 16 bytes, LDS position = lane.  Wave w takes half w & 1 of key rows
// 2j + (w >> 1).  The K image is swizzled (slot ^ kr, low 4 slot bits) through the SOURCE address; V is linear.
__device__ __forceinline__ void faw_stage(i32x4 krs, i32x4 vrs, unsigned char* buf, int key0, int Nk, int rowbytes, int lane, int w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kr = 2 * j + (w >> 1), hf = w & 1;
        const int key = min(key0 + kr, Nk - 1);
        const int so = key * rowbytes + hf * 1024;
        unsigned char* dst = buf + kr * FAW_ROW + hf * 1024;
        skp_buf_load_lds(krs, (skp_lds_ptr)dst, 16, (lane ^ kr) << 4, so, 0, 0);
        skp_buf_load_lds(vrs, (skp_lds_ptr)(dst + FAW_TILE), 16, lane << 4, so, 0, 0);
    }
}

__global__ __launch_bounds__(256) void skp_faw_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                          const float* __restrict__ v, float* __restrict__ out, int H, int N,
                                                          int Nk, int qtiles, float scale) {
    extern __shared__ __attribute__((aligned(16))) unsigned char faw_smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c = lane & 15;
    int bid = blockIdx.x;
    const int qt = bid % qtiles;
    bid /= qtiles;
    const int h = bid % H, b = bid / H;
    const size_t C = (size_t)H * FAW_D;
    const float* qb = q + (size_t)b * N * C + (size_t)h * FAW_D;
    const float* kb = k + (size_t)b * Nk * C + (size_t)h * FAW_D;
    const float* vb = v + (size_t)b * Nk * C + (size_t)h * FAW_D;
    float* ob = out + (size_t)b * N * C + (size_t)h * FAW_D;

    const int rowbytes = (int)(C * 4);
    const unsigned kvbytes = (unsigned)(Nk - 1) * (unsigned)rowbytes + FAW_ROW;        // this head's slice of the last row ends here
    const i32x4 krs = skp_make_rsrc(kb, kvbytes), vrs = skp_make_rsrc(vb, kvbytes);
    faw_stage(krs, vrs, faw_smem, 0, Nk, rowbytes, lane, w);

    // the wave's 16 queries: lane (g, c) holds channels 16j + 4g .. +3 of query c in qr[4j .. 4j+3]
    float qr[128];
    {
        const int qrow = qt * FAW_BQ + w * 16 + c;
        const bool live = qrow < N;
        const float* qp = qb + (size_t)(live ? qrow : N - 1) * C + 4 * g;          // clamped row, zeroed below
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const f32x4 x = *(const f32x4*)(qp + 16 * j);
            qr[4 * j + 0] = live ? x[0] : 0.f;
            qr[4 * j + 1] = live ? x[1] : 0.f;
            qr[4 * j + 2] = live ? x[2] : 0.f;
            qr[4 * j + 3] = live ? x[3] : 0.f;
        }
    }

    f32x4 o[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // byte offsets of the lane's K reads (slot 4j + g of key row c, swizzled: the XOR touches the low 4 slot bits only) and V reads
    int koff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) koff[j] = c * FAW_ROW + (((4 * j + g) ^ c) << 4);
    const int voff = FAW_TILE + 4 * g * FAW_ROW + (c << 4);

    const int ntiles = (Nk + FAW_BK - 1) / FAW_BK;
    for (int t = 0; t < ntiles; ++t) {
        const unsigned char* buf = faw_smem + (t & 1) * (2 * FAW_TILE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's pieces of tile t have landed ...
        __syncthreads();                                          // ... and everybody's; nobody reads the other buffer any more
        if (t + 1 < ntiles) faw_stage(krs, vrs, faw_smem + ((t + 1) & 1) * (2 * FAW_TILE), (t + 1) * FAW_BK, Nk, rowbytes, lane, w);

        // ---- S^T = K Q^T over 512 channels, four accumulators (the dependent-accumulator latency of 16x16x4 exceeds its issue time).
        // LDS reads run one group of four ahead of the 16 MFMAs that use them; the scheduling barriers keep that order (left to
        // itself the compiler issues every read right before its use and waits for it).
        f32x4 sa[4], kv[2][4], vv[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sa[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            kv[0][i] = *(const f32x4*)(buf + koff[i]);
        }
#pragma unroll
        for (int G = 0; G < 8; ++G) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (G + 1 < 8) kv[(G + 1) & 1][i] = *(const f32x4*)(buf + koff[i] + (G + 1) * 256);
                else vv[0][i] = *(const f32x4*)(buf + voff + i * 256);                     // the first V group
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    sa[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[G & 1][jj][i], qr[4 * (4 * G + jj) + i], sa[i], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const f32x4 s01 = (sa[0] + sa[1]) + (sa[2] + sa[3]);

        // ---- online softmax of query c over keys t*16 + 4g + r
        float sv[4], p[4];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = s01[r] * scale;
            sv[r] = (t * FAW_BK + 4 * g + r < Nk) ? s : -INFINITY;
            mx = fmaxf(mx, sv[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(m, mx);                               // finite: tile 0 holds key 0
        const float alpha = __builtin_amdgcn_exp2f((m - mnew) * SKP_LOG2E);   // m = -inf on the first tile: exp2(-inf) = 0
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = __builtin_amdgcn_exp2f((sv[r] - mnew) * SKP_LOG2E);
            psum += p[r];
        }
        l = l * alpha + psum;
        m = mnew;
        if (!__all(alpha == 1.0f)) {                                   // wave-uniform: O rows are queries 4g + r, not c
            float ar[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * g + r, 64);
#pragma unroll
            for (int tt = 0; tt < 32; ++tt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[tt][r] *= ar[r];
            }
        }

        // ---- O += P V: k-step r sums keys 4g + r over g.  Group P = V row r = P >> 1, channel blocks tt = 4 (P & 1) .. +3
#pragma unroll
        for (int P = 0; P < 8; ++P) {
            if (P + 1 < 8) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    vv[(P + 1) & 1][i] = *(const f32x4*)(buf + voff + ((P + 1) >> 1) * FAW_ROW + (4 * ((P + 1) & 1) + i) * 256);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tt = 4 * (P & 1) + i;
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
                    o[4 * tt + ii] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[P >> 1], vv[P & 1][i][ii], o[4 * tt + ii], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ir = __shfl(inv, 4 * g + r, 64);
        const int qo = qt * FAW_BQ + w * 16 + 4 * g + r;
        if (qo < N) {
            float* op = ob + (size_t)qo * C + 4 * c;
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) {
                const f32x4 y = {o[4 * tt + 0][r] * ir, o[4 * tt + 1][r] * ir, o[4 * tt + 2][r] * ir, o[4 * tt + 3][r] * ir};
                *(f32x4*)(op + 64 * tt) = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int skp_flash_attn_fwd_wide_ok(int B, int Bk, int H, int N, int Nk, int d) {
    if (B <= 0 || H <= 0 || N <= 0 || Nk <= 0 || Bk != B || d != FAW_D) return 0;
    if ((long long)Nk * H * FAW_ROW > 0x7fffffffll) return 0;                           // 32-bit offsets inside one batch row of k / v
    return (long long)((N + FAW_BQ - 1) / FAW_BQ) * H * B <= 0x7fffffffll ? 1 : 0;      // one workgroup per 64 queries, 1-D grid
}

// No key-range split is planned: the kernel needs no workspace.
extern "C" int64_t skp_flash_attn_fwd_wide_workspace(int B, int Bk, int H, int N, int Nk, int d) {
    if (B <= 0 || Bk <= 0 || H <= 0 || N <= 0 || Nk <= 0 || d <= 0) return SKP_E_BADARG;
    return skp_flash_attn_fwd_wide_ok(B, Bk, H, N, Nk, d) ? 0 : SKP_E_RANGE;
}

extern "C" int skp_flash_attn_fwd_wide_f32(const float* q, const float* k, const float* v, float* out, void* workspace, int B, int Bk,
                                           int H, int N, int Nk, int d, float scale, void* stream) {
    (void)workspace;
    if (!q || !k || !v || !out) return SKP_E_BADARG;
    if (B <= 0 || Bk <= 0 || H <= 0 || N <= 0 || Nk <= 0 || d <= 0) return SKP_E_BADARG;
    if (!skp_flash_attn_fwd_wide_ok(B, Bk, H, N, Nk, d)) return SKP_E_RANGE;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return SKP_E_BADARG;   // float4 rows
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute((const void*)skp_faw_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FAW_LDS);
        if (e != hipSuccess) return (int)e;
        attr = true;
    }
    const int qtiles = (N + FAW_BQ - 1) / FAW_BQ;
    hipLaunchKernelGGL(skp_faw_fwd_kernel, dim3((unsigned)(qtiles * H * B)), dim3(256), FAW_LDS, (hipStream_t)stream, q, k, v, out, H,
                       N, Nk, qtiles, scale);
    return skp_launch_status();
}
