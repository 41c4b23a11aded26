/* vtoonify_amd_rgbup.h -- entry point of libvtoonify_amd.so for the RGB skip path without its up-sampled planes
 * (model/stylegan/model.py:383-392: ToRGB.forward, `out + self.upsample(skip)`).  Included by vtoonify_amd.h:
 * same library, same return codes, vt_last_error and stream conventions.  Additive to ABI version 5: nothing declared in
 * vtoonify_amd.h changes and vt_conv_desc gets no field.  Bound by vtoonify_amd/_lib.py (_RGBUP_SIGS); tests/test_rgb_skip_fold.py
 * checks declaration, binding and export of the entry declared here. */
#ifndef VTOONIFY_AMD_RGBUP_H
#define VTOONIFY_AMD_RGBUP_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * A 3x3 conv with the fused ToRGB (conv->rgb_weight) whose epilogue adds Upsample(skip) -- upfirdn2d with up 2, pad (2, 1) and
 * the 4 x 4 `fir` (model.py:32-50) -- formed from the lo-res planes instead of read from planes that a launch of their own wrote:
 *   rgb_out[n][j][y][x] = ToRGB(conv(x))[n][j][y][x] + rgb_bias[j] + up(lo_planes)[n][j][y][x]
 * lo_planes: (n, 3, out_h / 2, out_w / 2) fp32; up(.) with the operations of the up-sampling launch in its order (flipped taps,
 * zeros outside the image, fp32 fmaf in (ky, kx) ascending order): the bits of the up-sampling launch into rgb_out followed by
 * the plain conv entry with rgb_resid = rgb_out, for any fir.  conv->rgb_resid is not read.  lo_planes must not alias rgb_out.
 * VT_ERR_UNSUPPORTED, nothing launched, unless the descriptor has rgb_weight (and no stats_part), out_h and out_w are even and
 * the plain conv entry would run it on the persistent 32 -> 32 kernel or on the weights-resident form of the patch kernel (KIND 3
 * of the tile query; KIND 1 with 64 -> 64 channels, a lean epilogue and at least two tiles per persistent workgroup).
 * --------------------------------------------------------------------------------- */
int vt_conv2d_rgbup(const vt_conv_desc* conv, const float* lo_planes, const float* fir, vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_RGBUP_H */
