/* vtoonify_amd_fusion.h -- entry points of libvtoonify_amd.so for the Fusion block without its packed operand
 * (model/vtoonify.py:122-128, 197-198, 262).  Included by vtoonify_amd.h: same library, same return codes,
 * vt_last_error and stream conventions.  Additive to ABI version 5: nothing declared in vtoonify_amd.h changes and
 * vt_conv_desc gets no field.  Bound by vtoonify_amd/_lib.py (_FUSION_SIGS); tests/test_fusion_gate_fem.py checks declaration,
 * binding and export of every entry declared here. */
#ifndef VTOONIFY_AMD_FUSION_H
#define VTOONIFY_AMD_FUSION_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * The gate's mask conv, m_E = relu(tanh(conv(AdaIN(cat[f_G, |f_G - f_E|])))) (vtoonify.py:125-126), that also writes the
 * fusion operand f_E * m_E (vtoonify.py:127).  Runs `mask_conv` exactly as the plain conv entry would -- the mask plane is
 * written to mask_conv->out -- and in the same launch
 *   fem[n][p][c] = round_T(float(src1[n][p][c]) * mask[n][p])     (n, h, w, c0) rows of ld_fem elements of the compute type
 * with the operations of vt_fusion_pack in its order: the same bits, without its pass over f_E.  fem must not alias src0 or
 * src1 (other workgroups still read their halos).  VT_ERR_UNSUPPORTED, nothing launched, when the descriptor is not the gate
 * form of the thin-output kernels: in_absdiff, 3x3, pad 1, cout 1, stride 1, NCHW fp32 output, c0 a multiple of the K step
 * (32 channels of a 16-bit type, 16 of fp32).
 * --------------------------------------------------------------------------------- */
int vt_conv2d_gate(const vt_conv_desc* mask_conv, void* fem, int32_t ld_fem, vt_stream stream);

/* ---------------------------------------------------------------------------------
 * fusion_skip (vtoonify.py:197-198, 262: a 3x3 conv of cat[skip, f_E * m_E]) with the skip planes as a second source: the K
 * range of `conv` is
 *   [ hdr_c fp32 NCHW planes (n, hdr_c, h, w), each value rounded to the compute type | zeros up to hdr_pad channels |
 *     the c0 channels of conv->src0 ]
 * and conv->weight holds c0 + hdr_pad input channels per tap in that order: the layout, the K order and the bits of the
 * plain conv entry on the tensor that vt_fusion_pack writes with a header of hdr_pad channels -- without that tensor.
 * VT_ERR_UNSUPPORTED, nothing launched, unless: 3x3, pad 1, stride 1, cout <= 3, a single source, NCHW fp32 output,
 * 0 <= hdr_c <= hdr_pad and hdr_pad a positive multiple of the K step (32 channels of a 16-bit type, 16 of fp32).
 * --------------------------------------------------------------------------------- */
int vt_conv2d_hdr(const vt_conv_desc* conv, const float* hdr_planes, int32_t hdr_c, int32_t hdr_pad, vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_FUSION_H */
