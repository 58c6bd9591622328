/* C ABI of libskp_hip.so, pose transfer of image sampling: keypoint guidance toward target MAPS (stablekeypoints_amd/ptp_utils.py
 * `keypoint_energy_grad` with `MapTargets`, `text2image_ldm_stable(target_maps=...)`).  The conventions are those of skp.h: device
 * pointers, dense row-major fp32, launch on `stream`, 0 / hipError_t / SKP_E_* as the return value, nothing written on error.  These
 * entries live in a header of their own because the tests hold skp.h and skp_keypoints.h to the exact contents of their tables; the
 * binding's table for this header is `_native.TARGET_SIGNATURES`, and tests/test_pose_transfer_host.py holds the two together type
 * by type.
 *
 * Reference interfaces replaced (paths relative to the reference's unsupervised_keypoints/): optimize.py:182-206
 * `find_gaussian_loss_at_point` with the target handed in instead of drawn (mode 0); the cosine form has no counterpart -- the
 * reference's generation script loads the example's maps ("example_attn_maps_indices.pt") and never uses them.
 */
#ifndef SKP_TARGETS_H
#define SKP_TARGETS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch bytes of skp_map_target_loss_f32: 0 in mode 0, 24 * B * K * ceil(R*R / 1024) in mode 1 (three doubles per chunk);
 * negative: SKP_E_BADARG (B / K / R <= 0, a mode that is not 0 or 1), SKP_E_RANGE (R > 32768 or more than 2^31 - 1 workgroups). */
int64_t skp_map_target_loss_workspace(int B, int K, int R, int mode);

/* Energy of K maps per image against K target maps, and its unit gradient (skp_target_loss.hip).  M, G: [B,K,R,R]; Tg: [Bt,K,R,R]
 * with Bt == B (a target per image) or Bt == 1 (one target for every image, read in place); partial: [B,K,nchunk],
 * nchunk = ceil(R*R / 1024).  Per map (b, k), sums over its R*R elements, T = Tg[Bt == 1 ? 0 : b, k]:
 *   mode 0 (mse)
 *     partial[b,k,j] = sum over the j-th 1024 elements of (M - T)^2   (the caller sums and divides by K*R*R:
 *                      E[b] = mean_{k,r,c} (M - T)^2)
 *     G[b,k,r,c]     = 2 (M - T) / (K R^2)                                                            = dE[b] / dM[b,k,r,c]
 *   mode 1 (cosine), with a = sum M^2, c = sum T^2, d = sum M T, mh = M / sqrt(a), th = T / sqrt(c), cos = d / sqrt(a c)
 *     partial[b,k,j] = sum over the j-th 1024 elements of (mh - th)^2   (the caller sums, halves and divides by K:
 *                      E[b] = (1/K) sum_k 1/2 sum (mh - th)^2 = (1/K) sum_k (1 - cos), formed from the squared differences, which do
 *                      not cancel where the maps agree)
 *     G[b,k,r,c]     = (cos mh - th) / (K sqrt(a))                                                    = dE[b] / dM[b,k,r,c]
 *     a map with a == 0 or c == 0 (all zeros) has no direction: it contributes E_k = 1 (partial[b,k,0] = 2, the other chunks 0) and
 *     G[b,k] = 0.  The energy does not change when either map is scaled by a positive number.
 * Mode 1 takes two passes: the first writes (a, c, d) of every chunk to `workspace`, the second folds the chunk sums of its own map in
 * a fixed order and writes G and partial.  All sums, the normalisation and the differences are fp64 on the float inputs (a product of
 * two floats is exact there); every element of G and of partial is rounded to fp32 once.  One workgroup per (image, map, chunk), the
 * plan a function of (B, K, R) alone, no atomics: bit-identical from call to call.  Any R >= 1 (R <= 32768), any K >= 1.  Tg, like M,
 * is read by the kernel, not at launch; G and partial overlap nothing that is read.
 * SKP_E_BADARG: M, Tg, partial or G NULL; B / K / R <= 0; Bt neither 1 nor B; a mode that is not 0 or 1; `workspace` NULL in mode 1.
 * SKP_E_RANGE: as the query. */
int skp_map_target_loss_f32(const float* M, const float* Tg, int B, int Bt, int K, int R, int mode, float* partial, float* G,
                            void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
