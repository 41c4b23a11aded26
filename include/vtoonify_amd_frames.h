/* vtoonify_amd_frames.h -- entry points of libvtoonify_amd.so for source-size frames: --scale_image on the GPU
 * (vtoonify_amd/scale.py ScaleCrop; tools/style_transfer_amd.py --scale_on gpu).  Included by vtoonify_amd.h: same library,
 * same return codes, vt_last_error and stream conventions.  Additive to ABI version 5: nothing declared in vtoonify_amd.h
 * changes.  Bound by vtoonify_amd/_lib.py (_FRAMES_SIGS); tests/test_frame_scale.py checks declaration, binding and export of
 * every entry declared here. */
#ifndef VTOONIFY_AMD_FRAMES_H
#define VTOONIFY_AMD_FRAMES_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * Blur, resize and crop of uint8 frames in one launch: what style_transfer.py:113-127,150-155 does per frame on the host
 * (cv2.sepFilter2D once at scale <= 0.75, twice at <= 0.375, cv2.resize of the whole frame, a slice).
 *   out    (n,H,W,3)      the crop
 *   src    (n,rows,Ws,3)  source rows [row0, row0+rows) of each Hs x Ws frame: the slab the crop needs, blur halo included
 *   passes 0..2           blur passes, each  B[y,x] = (sum_ij k_i k_j P[r(y+o_i), r(x+o_j)] + 32768) >> 16  with
 *                         k = (32,96,96,32) at offsets (-2,-1,0,+1) and r = reflect-101 in full-frame coordinates
 *                         (r(-1) = 1, r(n) = n-2); a second pass filters the uint8 result of the first.  Frames >= 3 x 3.
 *   xtab   (W,4) int32    per output column x0, x1, a0, a1;   ytab (H,4) int32   per output row y0, y1, b0, b1
 *                         (full-frame indices, weights 0..2048; vtoonify_amd/scale.py resize_tables builds them), in memory
 *                         the GPU reads.  With Q the frame after `passes` passes, per channel
 *                           h_r = a0 Q[r,x0] + a1 Q[r,x1]
 *                           out = (((b0 (h_y0 >> 4)) >> 16) + ((b1 (h_y1 >> 4)) >> 16) + 2) >> 2
 * Integer arithmetic throughout: bit-exact against the numpy restatement of tests/test_frame_scale.py.
 * The launcher copies the two tables to the host (a synchronous copy: not capturable into a graph) and returns VT_ERR_ARG
 * without launching when an index lies outside the frame, a weight outside 0..2048, or a row that the tables or the blur
 * halo reach (reflected rows at a frame border included) outside the slab; VT_ERR_UNSUPPORTED when the source footprint of
 * an 8 x 8 output tile does not fit the kernel's LDS (scales down to 1/8 with two passes fit).
 * --------------------------------------------------------------------------------- */
int vt_frame_scale_crop(uint8_t* out, const uint8_t* src, int n, int rows, int row0, int Hs, int Ws, int passes,
                        const int32_t* xtab, const int32_t* ytab, int H, int W, vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_FRAMES_H */
