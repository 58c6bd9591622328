/* C ABI of libskp_hip.so, keypoint visualisation (stablekeypoints_amd/visualize.py `overlay`, `save_grid`,
 * `plot_point_correspondences`).  The conventions are those of skp.h: device pointers, dense row-major fp32, launch on `stream`,
 * 0 / hipError_t / SKP_E_* as the return value, nothing written on error.  These entries live in a header of their own because the
 * tests hold skp.h and skp_keypoints.h to the exact contents of their tables; the binding's table for this header is
 * `_native.OVERLAY_SIGNATURES`, and tests/test_render_host.py holds the two together type by type.
 *
 * Reference interfaces replaced (paths relative to the reference's unsupervised_keypoints/): visualize.py:40-138 `save_grid`,
 * `plot_point_single`, `plot_point_correspondences`, which draw with matplotlib on the host; here (images, maps, points) become
 * bytes in one pass on the device.
 */
#ifndef SKP_OVERLAY_H
#define SKP_OVERLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Scratch bytes of skp_map_range_f32 for N maps of `plane` elements (0: the maps are not split and `workspace` may be NULL);
 * negative: SKP_E_BADARG (N / plane <= 0), SKP_E_RANGE (more than 2^31 - 1 workgroups). */
int64_t skp_map_range_workspace(int N, int64_t plane);

/* (min, max) of every map (skp_overlay.hip): M [N, plane] -> range [N, 2].  A NaN element is ignored; a map of only NaN gives
 * (0, 0).  Minimum and maximum are exact and taken in the total order of the bit patterns (-0 < +0), so the result does not
 * depend on how a map is split: a map is cut into equal segments over several workgroups (the machine is filled for N = 1 as for
 * N = 990), each writes its pair to `workspace`, and a second small kernel folds the pairs.  No atomics.  16-byte loads where
 * `plane` is a multiple of 4 and M is 16-byte aligned.
 * SKP_E_BADARG: M or range NULL, N / plane <= 0, workspace NULL where the query asks for bytes. */
int skp_map_range_f32(const float* M, float* range, void* workspace, int N, int64_t plane, void* stream);

/* Images, optionally under a colour-mapped heat map and numbered markers, to bytes in a canvas (skp_overlay.hip).
 *   img [B,3,H,W]; map [B,S,S] with range [B,2] = (lo, hi) per map, or NULL; lut [L,3], L >= 2; pts [B,K,2] = (row, col) in image
 *   fractions, or NULL with K = 0; colors [K,3]; glyphs uint8 [10,7]: digit d, row r of a 5 x 7 font in the low 5 bits of
 *   glyphs[7 d + r], the leftmost column in bit 4 (needed when `labels` and K > 0).
 *   out: uint8 pixels, 3 bytes each, of a canvas `ld` pixels wide and `canvas_h` high; image b is written at
 *   (y0 + (b / cols) (H + gap), x0 + (b % cols) (W + gap)).  Only tile pixels are written.
 * Per pixel (y, x) of image b, centre (y + 0.5, x + 0.5), in fp32:
 *   c = clamp(img[b,:,y,x], 0, 1)
 *   with a map: m = map[b,y,x] when S = H = W, else the bilinear sample at ((y + 0.5) S / H - 0.5, (x + 0.5) S / W - 0.5), the
 *               coordinate clamped at 0 and the indices at S - 1 (F.interpolate, align_corners = False);
 *               n = clamp((m - lo) / (hi - lo), 0, 1), 0 when hi <= lo or m is NaN;  t = n (L - 1), i = min(int(t), L - 2),
 *               colour = lut[i] + (t - i) (lut[i+1] - lut[i]);  c = (1 - alpha) c + alpha colour
 *   for j = 0 .. K-1 in order: (py, px) = (pts[b,j,0] H, pts[b,j,1] W), skipped when either is NaN; d = the distance of the pixel
 *               centre from it; a = clamp(radius + ring + 0.5 - d, 0, 1), c = c + a (1 - c);
 *               a = clamp(radius + 0.5 - d, 0, 1), c = c + a (colors[j] - c);
 *               with `labels`, the decimal digits of j (one or two) from `glyphs` at scale fs = max(1, int(radius / (0.5 sqrt(bw^2 + 49)))),
 *               bw = 5 for one digit and 11 for two (5 + 1 + 5 columns): a box of bw fs x 7 fs pixels with its top-left at
 *               (floor(py - 3.5 fs + 0.5), floor(px - bw fs / 2 + 0.5)); a pixel on a set glyph bit gets c = c + a (1 - c) with the
 *               disc's a.
 *   byte = (int)(c 255)        -- with neither map nor points this is skp_image_u8_nhwc_f32 for images in [0, 1]
 * One lane takes four consecutive pixels (16-byte loads, three dwords out) where W % 4 == 0, img (and map, when S = W) are 16-byte
 * aligned and out, ld, x0 and the tile pitch W + gap (for cols > 1) keep every group of four pixels 4-byte aligned; one pixel per
 * lane otherwise.  Markers that cannot touch the rows a workgroup covers are skipped for the whole workgroup.
 * SKP_E_BADARG: a needed pointer NULL; B / H / W <= 0; with a map S <= 0 or L < 2; K < 0; radius / ring not >= 0; cols < 1,
 * gap < 0, y0 / x0 < 0, or a tile outside the ld x canvas_h canvas.  SKP_E_RANGE: H, W or S > 4096, K > 100, L > 1024. */
int skp_overlay_u8_f32(const float* img, const float* map, const float* range, const float* lut, const float* pts,
                       const float* colors, const unsigned char* glyphs, unsigned char* out, int B, int H, int W, int S, int L,
                       int K, float alpha, float radius, float ring, int labels, int ld, int canvas_h, int y0, int x0, int cols,
                       int gap, void* stream);

#ifdef __cplusplus
}
#endif
#endif
