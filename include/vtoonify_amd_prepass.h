/* vtoonify_amd_prepass.h -- entry points of libvtoonify_amd.so for the streaming flicker-reduction pre-pass
 * (smooth_parsing_map.py; vtoonify_amd/smooth.py ParsingSmoother).  Included by vtoonify_amd.h: same library, same return
 * codes, vt_last_error and stream conventions.  Additive to ABI version 5: nothing declared in vtoonify_amd.h changes.
 * Bound by vtoonify_amd/_lib.py (_PREPASS_SIGS); tests/test_smooth_stream.py checks declaration, binding, export and test
 * coverage of every entry declared here. */
#ifndef VTOONIFY_AMD_PREPASS_H
#define VTOONIFY_AMD_PREPASS_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * Frame ingest of the pre-pass: frames (n,h,w,3) uint8 -> its three inputs at twice the frame size, planar fp32
 * (n,3,2h,2w), in one read of the frame:
 *   is         = F.upsample(Normalize(ToTensor(frame)), scale_factor=2, mode='bilinear')
 *                (smooth_parsing_map.py:86-89,128; align_corners=False, aten's area_pixel_compute_source_index and
 *                lerp order h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d) in fp32)
 *   raft_in    = (is + 1) * 255.0 / 2   RAFT's network input (smooth_parsing_map.py:154); NULL to skip
 *   bisenet_in = 2 * is                 BiSeNet's network input (smooth_parsing_map.py:136); NULL to skip
 * swap_rb != 0: frames are BGR as cv2 delivers them (replaces cv2.cvtColor, smooth_parsing_map.py:122).
 * fp32 op order is the reference's: raft_in / bisenet_in are bit-exact images of `is` under the torch formulas.
 * h * w < 2^28.
 * --------------------------------------------------------------------------------- */
int vt_frame_ingest2x(float* is, float* raft_in, float* bisenet_in, const uint8_t* frames, int swap_rb, int n, int h,
                      int w, vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_PREPASS_H */
