/* vtoonify_amd_align.h -- entry points of libvtoonify_amd.so for the face alignment of the style encoder's input
 * (model/encoder/align_all_parallel.py:59-150 after get_landmark; vtoonify_amd/align.py FaceAligner;
 * tools/style_transfer_amd.py --landmarks).  Included by vtoonify_amd.h: same library, same return codes, vt_last_error and
 * stream conventions.  Additive to ABI version 5: nothing declared in vtoonify_amd.h changes.  Bound by vtoonify_amd/_lib.py
 * (_ALIGN_SIGS); tests/test_face_align.py checks declaration, binding and export of every entry declared here.
 * The plan (quad, shrink, crop box, pads, sigma) is host work in float64: vtoonify_amd/align.py align_parameters.
 * Images are 8-bit RGB, 3 bytes per pixel.  A "view" is a sub-rectangle of an image: a pointer to its first pixel and the
 * distance `pitch` in bytes between its rows -- the crop of the reference costs no copy.  Nothing is launched when an
 * entry returns an error. */
#ifndef VTOONIFY_AMD_ALIGN_H
#define VTOONIFY_AMD_ALIGN_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VT_ALIGN_MAX_RADIUS 128 /* largest blur radius of the pad branch (the reference's sigma stays below 21: radius 82) */

/* ---------------------------------------------------------------------------------
 * The shrink (align_all_parallel.py:109-112): Pillow's resize(..., LANCZOS) of an 8-bit image, restricted to a region of
 * the output.  Two passes, horizontal first, a uint8 image between them, integer arithmetic:
 *     pixel = clip8((2^21 + sum_i k_i p_i) >> 22)
 *   out     (H,W,3)        the region of the resized image
 *   src     (rows,Ws,3)    source rows [row0, row0+rows) of the Hs x Ws image: the slab that the region reads
 *   xbound  (W,2) int32    per output column: first source column, number of taps;   xcoef (W,kx) int32: the weights of 2^22
 *   ybound  (H,2) int32    per output row: first source row (full-image index), taps;  ycoef (H,ky) int32
 *                          (vtoonify_amd/align.py lanczos_tables builds them), in memory the GPU reads.
 * The launcher copies the tables to the host (a synchronous copy: not capturable into a graph) and returns VT_ERR_ARG when a
 * count is < 1 or exceeds the table width, or an index leaves the image or the slab; VT_ERR_UNSUPPORTED when the source
 * footprint of a 4 x 8 output tile does not fit the kernel's LDS (shrink factors up to 8 fit).
 * --------------------------------------------------------------------------------- */
int vt_align_resample_u8(uint8_t* out, const uint8_t* src, int rows, int row0, int Hs, int Ws, const int32_t* xbound,
                         const int32_t* xcoef, int kx, const int32_t* ybound, const int32_t* ycoef, int ky, int H, int W,
                         vt_stream stream);

/* ---------------------------------------------------------------------------------
 * The pad branch (align_all_parallel.py:133-141) on a view of h0 x w0 pixels, float32 without fused multiply-add:
 *   img   = the view extended by pad_l, pad_t, pad_r, pad_b pixels, reflected without repeating the edge sample: h x w with
 *           h = h0 + pad_t + pad_b, w = w0 + pad_l + pad_r
 *   mask  = max(1 - min(x/pad_l, (w-1-x)/pad_r), 1 - min(y/pad_t, (h-1-y)/pad_b))
 *   blur  = Gaussian of radius r over rows, then over columns, boundary sample repeated (d c b a | a b c d); a line is
 *           summed in float64 -- centre tap, then pairs (p[-j] + p[+j]) taps[j] for j = r .. 1 -- and stored as float32
 *   img  += (blur - img) clip(3 mask + 1, 0, 1);   img += (median - img) clip(mask, 0, 1)
 *           median per channel over all h w pixels: the exact order statistic, for an even count the float32 mean of the
 *           two middle values (a radix select on the ordered float bits, one histogram per byte)
 *   out   (h,w,3) uint8 = clip(rint(img), 0, 255), halves to even
 *   taps  (r+1) float64 in memory the GPU reads: taps[j] weighs offsets +-j (vtoonify_amd/align.py gaussian_taps)
 *   ws    vt_align_pad_blend_workspace(h, w, r) bytes of scratch memory the GPU reads and writes
 * VT_ERR_ARG when a pad is < 1 (the mask divides by it) or not smaller than the side of the view it reflects, when r < 0 or
 * r is not smaller than h and w, or when ws_bytes is too small; VT_ERR_UNSUPPORTED when r > VT_ALIGN_MAX_RADIUS.
 * vt_align_pad_blend_workspace returns 0 (and sets vt_last_error) for sizes it cannot serve.
 * --------------------------------------------------------------------------------- */
int64_t vt_align_pad_blend_workspace(int h, int w, int r);
int vt_align_pad_blend(uint8_t* out, const uint8_t* src, int h0, int w0, int pitch, int pad_l, int pad_t, int pad_r,
                       int pad_b, const double* taps, int r, void* ws, int64_t ws_bytes, vt_stream stream);

/* ---------------------------------------------------------------------------------
 * The transform (align_all_parallel.py:145): Pillow's transform((S,S), QUAD, ..., BILINEAR) of an h x w view, in float64
 * without contraction.  Output pixel (x, y), with xo = x + 0.5 and yo = y + 0.5, samples
 *     xin = a[0] + a[1] xo + a[2] yo + a[3] xo yo,   yin = a[4] + a[5] xo + a[6] yo + a[7] xo yo
 * and is 0 in every channel when xin < 0, xin >= w, yin < 0 or yin >= h.  Otherwise 0.5 is subtracted from both, the four
 * neighbours of the floor (indices clamped to the view) are blended -- v1 = p00 + (p01 - p00) dx, v2 likewise,
 * v = v1 + (v2 - v1) dy -- and v is TRUNCATED to uint8.
 *   out_u8   (S,S,3) uint8
 *   out_f32  (3,S,S) float32 or NULL: ((v / 255) - 0.5) / 0.5 of the uint8 value, division and subtraction kept apart
 *            (torchvision's ToTensor and Normalize(0.5, 0.5))
 *   a        8 doubles in HOST memory, read before the call returns (vtoonify_amd/align.py quad_coefficients)
 * VT_ERR_ARG for a null pointer, sizes < 1, S > 4096, a pitch < 3 w or a coefficient that is not finite.
 * --------------------------------------------------------------------------------- */
int vt_align_quad(uint8_t* out_u8, float* out_f32, const uint8_t* img, int h, int w, int pitch, const double* a, int S,
                  vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_ALIGN_H */
