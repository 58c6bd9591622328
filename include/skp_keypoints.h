/* C ABI of libskp_hip.so, keypoint guidance of image sampling (stablekeypoints_amd/ptp_utils.py `keypoint_energy_grad`,
 * `text2image_ldm_stable(keypoints=...)`).  The conventions are those of skp.h: device pointers, dense row-major fp32, launch on
 * `stream`, 0 / hipError_t / SKP_E_* as the return value, nothing written on error.  These entries live in a header of their own
 * because tests/test_host_logic.py holds skp.h to a census of its pointer parameters; the binding's table for this header is
 * `_native.KEYPOINT_SIGNATURES`, and tests/test_keypoint_guidance_host.py holds the two together type by type.
 *
 * Reference interfaces replaced (paths relative to the reference's unsupervised_keypoints/):
 *   skp_point_loss_f32        optimize.py:182-206 `find_gaussian_loss_at_point` + optimize_token.py:203-225 `gaussian_circle`, one
 *                             point per token, positions in device memory
 *   skp_sampler_step_kp_f32   no counterpart: the reference's generation script loads its target maps and never uses them
 */
#ifndef SKP_KEYPOINTS_H
#define SKP_KEYPOINTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Energy of K maps per image against gaussian targets at caller-given positions, and its unit gradient (skp_point_loss.hip):
 *   t[b,k,r,c] = exp(-((c + 0.5 - R pos[b,k,1])^2 + (r + 0.5 - R pos[b,k,0])^2) / (2 sigma^2))      pos = (row, col) in image fractions
 *   partial[b,k,j] = sum over the j-th 1024 elements of (M[b,k] - t[b,k])^2,  nchunk = ceil(R*R / 1024)  (the caller sums and
 *                    divides by K*R*R: E[b] = mean_{k,r,c} (M - t)^2)
 *   G[b,k,r,c] = 2 (M - t) / (K R^2)                                                                   = dE[b] / dM[b,k,r,c]
 * M, G: [B,K,R,R]; pos: [B,K,2] in DEVICE memory (read by the kernel, not at launch), any finite value -- positions outside [0, 1] are
 * legal; partial: [B,K,nchunk].  The exponent is evaluated in fp64 and t = expf(-hi) (1 - lo) with hi + lo the exponent split into
 * two floats (capped at 200, where t is 0 in fp32 either way, so a position however far away gives t = 0).  Fixed summation
 * order, no atomics: bit-identical from call to call.  Any R >= 1 (R <= 32768), any K >= 1.
 * SKP_E_BADARG: a NULL pointer, B / K / R <= 0, sigma not > 0.  SKP_E_RANGE: R > 32768 or more than 2^31 - 1 workgroups. */
int skp_point_loss_f32(const float* M, const float* pos, int B, int K, int R, float sigma, float* partial, float* G, void* stream);

/* skp_sampler_step_f32 (skp.h) with the gradient term of keypoint guidance (skp_sampler_step.hip, the same kernel with one more
 * compile-time flag).  Per element i < n, with row = i / (n / rows) and s = gs[row]:
 *   m         = m_u ? m_u + guidance * (m_c - m_u) : m_c
 *   (x0, eps) = prediction 0 (epsilon): ((x - sb m) / sa, m)
 *               prediction 1 (v):       (sa x - sb m, sa m + sb x)
 *               prediction 2 (sample):  (m, (x - sa m) / sb)
 *   eps       = eps + s g[i]
 *   x0        = x0 - (sb / sa) s g[i]           (the same shift in both parametrisations: sa x0 + sb eps stays x)
 *   x0        = clamp(x0, -1, 1) if clip
 *   y         = cx x + c0 x0 + ce eps + c1 x0_prev + cn noise
 *   x0_out    = x0
 * g: n floats, the gradient of the energy by x; gs: `rows` floats in DEVICE memory (read by the kernel: the loop computes them on the
 * device and never reads them back); n % rows == 0.  sb / sa is formed in fp64 from the two floats and rounded once.  Everything
 * else -- x0_prev / noise / x0_out, copies, aliasing (g and gs overlap nothing that is written), alignment (g counts among the
 * pointers that must be 16-byte aligned for 16-byte accesses), no atomics -- as for skp_sampler_step_f32.
 * SKP_E_BADARG: as there, and g or gs NULL, rows <= 0, n % rows != 0. */
int skp_sampler_step_kp_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise, float* y,
                            float* x0_out, int64_t n, int copies, float guidance, int prediction, float sa, float sb, float cx,
                            float c0, float ce, float c1, float cn, int clip, const float* g, const float* gs, int rows,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
