/* C ABI of libskp_hip.so, evaluation stage: attention maps to keypoint locations (stablekeypoints_amd/eval.py `locate_keypoints`,
 * `evaluate`; keypoint_regressor.py `precompute_all_keypoints(batched_locator=True)`).  The conventions are those of skp.h: device
 * pointers, dense row-major fp32, launch on `stream`, 0 / hipError_t / SKP_E_* as the return value, nothing written on error.  These
 * entries live in a header of their own because the tests hold skp.h, skp_keypoints.h and skp_overlay.h to the exact contents of
 * their tables; the binding's table for this header is `_native.LOCATE_SIGNATURES`, and tests/test_locate_host.py holds the two
 * together type by type.
 *
 * Reference interfaces replaced (paths relative to the reference's unsupervised_keypoints/): eval.py:39-60 `find_max_pixel` and
 * eval.py:113-155 `pixel_from_weighted_avg`, called once per image on [K,512,512] maps (keypoint_regressor.py:191-196,
 * eval.py:447-450): an arg-max, then about fifteen elementwise passes over the maps, the far pixels zeroed in place.  Here a whole
 * group of images' maps becomes locations in one pass that reads every map once and writes nothing into it.
 */
#ifndef SKP_LOCATE_H
#define SKP_LOCATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch bytes of skp_locate_f32 for N maps of H x W (0: no map is split over workgroups and `ws` may be NULL);
 * negative: SKP_E_BADARG (N / H / W <= 0), SKP_E_RANGE (H or W > 4096).
 * The plan is a function of (N, H, W) alone:
 *   maps of at most 1024 elements      one wave per map, four maps per workgroup
 *   larger maps                        one 256-thread workgroup per map, or, from 8192 elements on, a map cut into `splits`
 *                                      equal segments (a multiple of 4 elements, at least 4096 each, at most 256 of them, about
 *                                      2048 workgroups over all maps) with one workgroup per segment; 32 bytes of scratch per segment. */
int64_t skp_locate_workspace(int N, int H, int W);

/* Location of the peak of every map (skp_locate.hip): M [N,H,W] -> loc [N,2] = (row, col) in pixels, flat [N].
 * Per map m:
 *   flat = the row-major index of the first maximal element (value descending, index ascending: the order of skp_token_stats_f32
 *          and of torch.argmax);  (r*, c*) = (flat / W, flat % W)
 *   mode 0 (arg-max):   loc = (r* + 0.5, c* + 0.5)
 *   mode 1 (weighted):  the window is every pixel (r, c) of the map with sqrtf((float)((r - r*)^2 + (c - c*)^2)) <= distance, the
 *                       square root correctly rounded (the reference's expression: its squares and their sum are exact integers in
 *                       fp32 up to 4096 rows and columns, then rounded once); distance == -1 takes the whole map;
 *                       T = sum of m over the window;  loc = (sum of r m, sum of c m) / (T + 1e-6) + 0.5
 *                       The three sums are taken in fp64 (every product r m is exact there) and the quotient is rounded to fp32 once
 *                       at the end, so the plain form stands and no coordinate is subtracted first: the result is the definition to
 *                       within an fp32 rounding of a well-conditioned map, whatever the order of summation.
 * M is only read.  The partial (maximum, index) pairs of a split map go to `ws` and a second small kernel folds them: the order
 * (value, index) is total, so `flat` does not depend on the split; no atomics.  For distance >= 0 only the pixels of the window's
 * bounding box, at most (2 floor(distance) + 1)^2, are read again, by the 256 threads of one workgroup (64 of one wave for maps of at
 * most 1024 elements) in one fixed order, split or not.  For distance == -1 the sums ride along with the arg-max pass and are folded in the order
 * the plan fixes.  Two calls with the same arguments give the same bits.  16-byte loads where H W is a multiple of 4 and M is
 * 16-byte aligned.
 * NaN: a NaN element never wins the arg-max; a map of only NaN gives flat = 0; with NaN in a window the location is NaN.  Every
 * index and every read stays inside the map.
 * SKP_E_BADARG: M, loc or flat NULL; N / H / W <= 0; mode not 0 or 1; in mode 1 a distance that is NaN or negative and not -1;
 * `ws` NULL or ws_bytes too small where the query asks for bytes.  SKP_E_RANGE: as the query. */
int skp_locate_f32(const float* M, int N, int H, int W, int mode, float distance, float* loc, int* flat, void* ws,
                   int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
