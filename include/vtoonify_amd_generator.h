/* vtoonify_amd_generator.h -- entry points of libvtoonify_amd.so for the parts of the StyleGAN2 / DualStyleGAN generator
 * forward (model/stylegan/model.py:395-590, model/dualstylegan.py:47-200) that the VToonify path never runs: real noise
 * injection and the latent row arithmetic.  Included by vtoonify_amd.h: same library, same return codes,
 * vt_last_error and stream conventions.  Additive to ABI version 5: nothing declared in vtoonify_amd.h changes.  Bound by
 * vtoonify_amd/_lib.py (_GENERATOR_SIGS); tests/test_generator_ops.py checks declaration, binding and export of every entry
 * declared here.  Every entry is asynchronous on the caller's stream, allocates nothing, and launches nothing when it returns
 * an error. */
#ifndef VTOONIFY_AMD_GENERATOR_H
#define VTOONIFY_AMD_GENERATOR_H
#include "vtoonify_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------
 * The counter-based generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
 * SC'11), the variant of Random123 and cuRAND.  One BLOCK is four 32-bit words x0..x3, a pure function of a 128-bit counter
 * (c0,c1,c2,c3) and a 64-bit key (k0,k1):
 *     ten rounds of   (c0,c1,c2,c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))
 *     with M0 = 0xD2511F53, M1 = 0xCD9E8D57 and hi/lo the halves of the 64-bit product; between two rounds (nine times)
 *     k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32).
 * The 64-bit arguments map to the words as
 *     c0 = low 32 bits of ctr_lo,  c1 = high 32 bits of ctr_lo,  c2 = low 32 bits of ctr_hi,  c3 = high 32 bits of ctr_hi,
 *     k0 = low 32 bits of key,     k1 = high 32 bits of key.
 *
 * vt_philox_u32: out (blocks,4) uint32 -- block i is the Philox block of counter (ctr_lo + i mod 2^64, ctr_hi) and `key`.
 *
 * vt_randn: out[e], 0 <= e < n, is element g = offset + e of the normal sequence of (key, stream_id).  Element g lives in
 * block j = g / 4 -- the Philox block of counter (ctr_lo = j, ctr_hi = stream_id) -- whose words make two Box-Muller pairs:
 *     pair A = (x0, x1) -> elements 4j and 4j+1,     pair B = (x2, x3) -> elements 4j+2 and 4j+3
 *     of a pair (x, y):   u = ((x >> 8) + 1) 2^-24  in (0,1],    v = (y >> 8) 2^-24  in [0,1)      (both exact in float32)
 *                         r = sqrtf(-2 logf(u)),    a = 6.2831855f v   (the float32 nearest to 2 pi, one rounded product)
 *                         first element = r cosf(a),   second element = r sinf(a)
 * in float32 with the accurate library logf, sqrtf and sincosf, no contraction; |value| <= sqrt(48 ln 2) = 5.77.  A lane
 * computes one block and, where out + e is 16-byte aligned and the four elements lie inside [0, n), writes them with one
 * 16-byte store; offset, n and the alignment of out are otherwise free.  The sequence depends on (key, stream_id, g) only:
 * drawing [offset, offset + n) in one call or in pieces gives the same bits.  The values are N(0,1) draws of THIS generator,
 * not the bits of any other library's normal sampler.
 * VT_ERR_ARG for a null pointer, blocks or n < 0 or offset < 0; zero blocks / n launches nothing and returns VT_OK.
 * --------------------------------------------------------------------------------- */
int vt_philox_u32(uint32_t* out, int64_t blocks, uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key, vt_stream stream);
int vt_randn(float* out, int64_t n, int64_t offset, uint64_t key, uint64_t stream_id, vt_stream stream);

/* ---------------------------------------------------------------------------------
 * The tail of StyledConv.forward (model/stylegan/model.py:364-370: NoiseInjection, then FusedLeakyReLU) in one pass over an
 * NHWC tensor:
 *     out[b,p,c] = lrelu(x[b,p,c] + w noise[nb == 1 ? 0 : b, p] + bias[c], 0.2) sqrt(2)
 * float32 arithmetic in this order: t = w noise (rounded), s = x + t, s = s + bias, s < 0 ? 0.2f s : s, times 1.41421356f;
 * one rounding to the tensor's type.
 *   out, x   (B, HW, C) of `dtype` (VT_F32, VT_BF16, VT_F16) with row strides ld_out, ld_x >= C in elements; 16-byte aligned
 *            pointers and row strides.  out == x with ld_out == ld_x (in place) is allowed; any other overlap is not.
 *   noise    (nb, HW) float32, nb = 1 (shared by the batch) or B
 *   w        one float32 in memory the GPU reads (NoiseInjection.weight is a parameter: no host read, graph-capturable)
 *   bias     (C) float32, or NULL for none
 * VT_ERR_UNSUPPORTED when C % 8 != 0 or for another dtype; VT_ERR_ARG for null pointers, sizes < 1, nb other than 1 or B, a
 * row stride below C, or a pointer / row stride that is not 16-byte aligned.
 * --------------------------------------------------------------------------------- */
int vt_noise_bias_act(void* out, int ld_out, const void* x, int ld_x, const float* noise, int nb, const float* w,
                      const float* bias, int B, int HW, int C, int dtype, vt_stream stream);

/* ---------------------------------------------------------------------------------
 * Latent row arithmetic (model/stylegan/model.py:533-538 truncation; model/dualstylegan.py:166-181 path mix), float32:
 *     out[r,i] = f_r b[r,i] + (1 - f_r) a[r,i]        f_r = f[r * f_stride],  f_stride = 0 (one factor) or 1 (one per row)
 * evaluated as written (two products, one difference, one sum: no contraction), so f = 0 returns a and f = 1 returns b
 * exactly for finite inputs.  Truncation is a = truncation_latent, b = style, f = psi; the path mix is a = w, b = T(e),
 * f = interp_weight.  A row stride of 0 for a or b broadcasts one row (the truncation latent) to every row.
 *   out (rows, dim) with row stride ld_out >= dim; a, b with row strides ld_a, ld_b that are 0 or >= dim; f in memory the GPU
 *   reads.  out may be a or b exactly (same stride); any other overlap is not allowed.
 * VT_ERR_ARG for null pointers, rows or dim < 1, a bad stride, or f_stride other than 0 or 1.
 * --------------------------------------------------------------------------------- */
int vt_lerp_rows(float* out, int ld_out, const float* a, int ld_a, const float* b, int ld_b, const float* f, int f_stride,
                 int rows, int dim, vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VTOONIFY_AMD_GENERATOR_H */
