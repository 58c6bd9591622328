/* C ABI of libskp_hip.so, device-row forms of the sampling step (stablekeypoints_amd/ptp_utils.py
 * `text2image_ldm_stable(capture=True)`): the step kernels of skp.h and skp_keypoints.h with what changes from step to step read
 * from DEVICE memory instead of the argument list, so that one recorded launch serves every step of a loop that is replayed as a
 * graph.  The conventions are those of skp.h: device pointers, dense row-major fp32, launch on `stream`, 0 / hipError_t / SKP_E_* as
 * the return value, nothing written on error.  These entries live in a header of their own because the tests hold skp.h,
 * skp_keypoints.h, skp_overlay.h and skp_locate.h to the exact contents of their tables; the binding's table for this header is
 * `_native.SAMPLER_GRAPH_SIGNATURES`, and tests/test_sample_graph_host.py holds the two together type by type.
 *
 * The table.  `table` is [steps, SKP_STEP_ROW] fp32; row s holds the numbers of step s, each computed by the host in fp64 and
 * rounded once (what the by-value entries receive as floats):
 *     column   0   1   2   3   4   5   6   7
 *              sa  sb  cx  c0  ce  c1  cn  guidance
 * skp_ddim_step_dev_f32 reads (sa, sb, c0, ce, guidance) with c0 = pa and ce = pb; skp_axpby_dev_f32 reads a = cx and b = ce.
 * `step` points to ONE int32 in device memory, the row to use; the kernel reads it when it runs, not at launch.  A kernel whose
 * counter is outside [0, steps) writes nothing and reads neither the table nor the noise.  No step kernel writes the counter:
 * skp_step_advance does, as a launch of its own, and the order of the launches in the stream is what orders the two.
 *
 * Same arithmetic.  Each entry instantiates the same device function as its by-value sibling (skp_sampler_step.hip `step_one`)
 * under the same contraction rule: for equal inputs and equal floats in the row the results are the sibling's, bit for bit.
 */
#ifndef SKP_SAMPLER_GRAPH_H
#define SKP_SAMPLER_GRAPH_H

#include <stdint.h>

#define SKP_STEP_ROW 8 /* floats per row of `table` */

#ifdef __cplusplus
extern "C" {
#endif

/* skp_axpby_f32 with a = table[*step][2] (cx) and b = table[*step][4] (ce): y[i] = a x[i] + b z[i], i < n (y may alias x or z).
 * SKP_E_BADARG: x / z / y / table / step NULL, n <= 0, steps <= 0.  SKP_E_RANGE: as skp_axpby_f32. */
int skp_axpby_dev_f32(const float* x, const float* z, float* y, int64_t n, const float* table, const int32_t* step, int steps,
                      void* stream);

/* skp_ddim_step_f32 with (sa, sb, pa, pb, guidance) = columns (0, 1, 3, 4, 7) of row *step.  y, copies, aliasing and alignment as
 * there (table and step are only read and overlap nothing that is written).
 * SKP_E_BADARG: as skp_ddim_step_f32, and table or step NULL, steps <= 0. */
int skp_ddim_step_dev_f32(const float* x, const float* m_c, const float* m_u, float* y, int64_t n, int copies, int prediction,
                          int clip, const float* table, const int32_t* step, int steps, void* stream);

/* skp_sampler_step_f32 with (sa, sb, cx, c0, ce, c1, cn, guidance) = row *step.
 *   noise    the base of [steps, n]: this step's gaussian is noise + *step * n.  16-byte accesses need n % 4 == 0 with it (every
 *            row aligned), besides the sibling's rule.
 *   absent terms  a term is absent where its COEFFICIENT in the row is exactly 0, not where its pointer is NULL: with c1 == 0
 *            x0_prev is not read and with cn == 0 noise is not read, whatever the buffers hold (the history of a multistep solver
 *            is uninitialised at its first step, and 0 * NaN must not reach y).  The test is on a value every lane of the grid
 *            shares, so the branch is uniform.  A NULL x0_prev / noise is the caller's statement that no row has a nonzero c1 / cn
 *            (the host cannot check a device table at launch): the term is absent on every step.
 * x0_out, y, copies, aliasing (y may alias x, x0_out may alias x0_prev), alignment and determinism as for the sibling.
 * SKP_E_BADARG: as skp_sampler_step_f32 without its coefficient rules, and table or step NULL, steps <= 0. */
int skp_sampler_step_dev_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise, float* y,
                             float* x0_out, int64_t n, int copies, int prediction, int clip, const float* table,
                             const int32_t* step, int steps, void* stream);

/* skp_sampler_step_kp_f32 (skp_keypoints.h) in the same form: the gradient term eps += s g, x0 -= (sb / sa) s g with s = gs[row of
 * the element], sb / sa formed in fp64 from the row's two floats and rounded once, as the sibling forms it on the host.
 * SKP_E_BADARG: as skp_sampler_step_dev_f32, and g or gs NULL, rows <= 0, n % rows != 0. */
int skp_sampler_step_kp_dev_f32(const float* x, const float* m_c, const float* m_u, const float* x0_prev, const float* noise,
                                float* y, float* x0_out, int64_t n, int copies, int prediction, int clip, const float* table,
                                const int32_t* step, int steps, const float* g, const float* gs, int rows, void* stream);

/* *step += 1: one lane, a plain vector load and store.  The last launch of a recorded step; every kernel of the next replay reads the
 * counter after it, by stream order.  SKP_E_BADARG: step NULL. */
int skp_step_advance(int32_t* step, void* stream);

#ifdef __cplusplus
}
#endif
#endif
