// Kernels of the StyleGAN2 / DualStyleGAN generator forward that the VToonify path never needed (include/vtoonify_amd_generator.h,
// DESIGN.md 4.10): a counter-based normal generator (Philox4x32-10 + Box-Muller) for NoiseInjection's per-call noise, the tail
// of StyledConv.forward (noise, bias, leaky ReLU) in one pass over an NHWC tensor, and the latent row blend of truncation and
// of DualStyleGAN's path mix.
//
// All three are HBM streaming or tiny: no LDS, no inter-lane traffic.
//   * randn: one lane = one Philox block = four normals = one 16-byte store; 40 integer multiplies and two log / sqrt / sincos
//     per 16 bytes written, far below the store rate of a 1024 x 1024 map (4 MB).
//   * noise_bias_act: a workgroup is (rows per pass) x (16-byte channel vectors of a row); a lane keeps ONE channel vector for
//     all its rows, so the bias vector is read once per workgroup into registers and the row loop does one 16-byte load, one
//     4-byte noise load (the lanes of a row read the same address: one request) and one 16-byte store.
#include <math.h>

#include "vt_common.hpp"
#include "../../include/vtoonify_amd_generator.h"

namespace {

struct PhiloxBlock {
    uint32_t x[4];
};

__device__ __forceinline__ PhiloxBlock philox4x32_10(uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
    uint32_t c0 = (uint32_t)ctr_lo, c1 = (uint32_t)(ctr_lo >> 32), c2 = (uint32_t)ctr_hi, c3 = (uint32_t)(ctr_hi >> 32);
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;   // the bump after the tenth round is never read
        k1 += 0xBB67AE85u;
    }
    PhiloxBlock b;
    b.x[0] = c0, b.x[1] = c1, b.x[2] = c2, b.x[3] = c3;
    return b;
}

// one Box-Muller pair of the header's definition
__device__ __forceinline__ void box_muller(uint32_t x, uint32_t y, float& z0, float& z1) {
    const float u = (float)((x >> 8) + 1u) * 5.9604644775390625e-8f;   // 2^-24: (0,1], exact
    const float v = (float)(y >> 8) * 5.9604644775390625e-8f;          // [0,1), exact
    const float r = sqrtf(-2.0f * logf(u));
    const float a = 6.2831855f * v;
    float s, c;
    sincosf(a, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

__global__ void __launch_bounds__(256)
philox_u32_kernel(uint32_t* __restrict__ out, int64_t blocks, uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= blocks) return;
    const PhiloxBlock b = philox4x32_10(ctr_lo + (uint64_t)i, ctr_hi, key);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * i + j] = b.x[j];   // out is only 4-byte aligned by contract
}

// lane i computes block j0 + i; `vec` (wave-uniform) says that out + (4 j - offset) is 16-byte aligned for every block
__global__ void __launch_bounds__(256)
randn_kernel(float* __restrict__ out, int64_t n, int64_t offset, int64_t j0, int64_t nblocks, uint64_t key, uint64_t stream_id,
             int vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nblocks) return;
    const int64_t j = j0 + i;
    const PhiloxBlock b = philox4x32_10((uint64_t)j, stream_id, key);
    float z[4];
    box_muller(b.x[0], b.x[1], z[0], z[1]);
    box_muller(b.x[2], b.x[3], z[2], z[3]);
    const int64_t e = 4 * j - offset;   // index in out of the block's first element: may be -3 .. -1 for the first block
    if (vec && e >= 0 && e + 4 <= n) {
        st128(out + e, pack16<float>(z));
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (e + t >= 0 && e + t < n) out[e + t] = z[t];
    }
}

// Lane layout: lanes_c = min(C / VEC, 256) channel vectors side by side, rpp = 256 / lanes_c rows per pass; a workgroup owns
// `rows_per_wg` consecutive pixel rows (of the B * HW rows of the tensor).  x and out may be the same memory: no __restrict__.
template <typename T>
__global__ void __launch_bounds__(256)
noise_bias_act_kernel(T* out, int ld_out, const T* x, int ld_x, const float* __restrict__ noise, int noise_per_sample,
                      const float* __restrict__ w, const float* __restrict__ bias, int64_t rows, int HW, int C, int lanes_c,
                      int rows_per_wg) {
    constexpr int VEC = 16 / sizeof(T);
    const int rpp = 256 / lanes_c;
    const int lr = threadIdx.x / lanes_c;
    const int lc = threadIdx.x - lr * lanes_c;
    if (lr >= rpp) return;   // 256 % lanes_c lanes have no row
    const float wv = w[0];
    const int cvec = C / VEC;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
    int64_t row1 = row0 + rows_per_wg;
    if (row1 > rows) row1 = rows;
    for (int cv = lc; cv < cvec; cv += lanes_c) {   // one trip unless a row has more than 256 vectors
        float bv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) bv[j] = bias ? bias[cv * VEC + j] : 0.0f;
        for (int64_t r = row0 + lr; r < row1; r += rpp) {
            const int64_t nidx = noise_per_sample ? r : r % HW;
            const float t = wv * noise[nidx];
            float f[VEC];
            unpack16<T>(ld128(x + r * ld_x + cv * VEC), f);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float s = f[j] + t;
                s = s + bv[j];
                s = s < 0.0f ? 0.2f * s : s;
                f[j] = s * 1.41421356f;
            }
            st128(out + r * ld_out + cv * VEC, pack16<T>(f));
        }
    }
}

template <typename T>
int launch_nba(void* out, int ld_out, const void* x, int ld_x, const float* noise, int nb, const float* w, const float* bias,
               int B, int HW, int C, vt_stream stream) {
    constexpr int VEC = 16 / sizeof(T);
    VT_REQUIRE(ld_out % VEC == 0 && ld_x % VEC == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x % 16 == 0,
               "vt_noise_bias_act: pointers and row strides must be 16-byte aligned (ld_out %d, ld_x %d)", ld_out, ld_x);
    const int cvec = C / VEC;
    const int lanes_c = cvec < 256 ? cvec : 256;
    const int rpp = 256 / lanes_c;
    const int64_t rows = (int64_t)B * HW;
    const int rows_per_wg = rpp * 4;
    const int64_t grid = (rows + rows_per_wg - 1) / rows_per_wg;
    VT_REQUIRE(grid < ((int64_t)1 << 31), "vt_noise_bias_act: %lld rows are too many", (long long)rows);
    auto k = noise_bias_act_kernel<T>;
    VT_LAUNCH(k, dim3((unsigned)grid), dim3(256), stream, (T*)out, ld_out, (const T*)x, ld_x, noise, nb == 1 ? 0 : 1, w, bias,
              rows, HW, C, lanes_c, rows_per_wg);
    return vt_check_launch("vt_noise_bias_act");
}

__global__ void __launch_bounds__(256)
lerp_rows_kernel(float* out, int ld_out, const float* a, int ld_a, const float* b, int ld_b, const float* __restrict__ f,
                 int f_stride, int rows, int dim) {
    const int64_t total = (int64_t)rows * dim;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / dim);
        const int c = (int)(i - (int64_t)r * dim);
        const float fr = f[(int64_t)r * f_stride];
        const float pb = fr * b[(int64_t)r * ld_b + c];
        const float pa = (1.0f - fr) * a[(int64_t)r * ld_a + c];
        out[(int64_t)r * ld_out + c] = pb + pa;
    }
}

}  // namespace

extern "C" int vt_philox_u32(uint32_t* out, int64_t blocks, uint64_t ctr_lo, uint64_t ctr_hi, uint64_t key, vt_stream stream) {
    VT_REQUIRE(blocks >= 0, "vt_philox_u32: negative block count");
    if (blocks == 0) return VT_OK;
    VT_REQUIRE(out, "vt_philox_u32: null output");
    const int64_t grid = (blocks + 255) / 256;
    VT_REQUIRE(grid < ((int64_t)1 << 31), "vt_philox_u32: %lld blocks are too many", (long long)blocks);
    VT_LAUNCH(philox_u32_kernel, dim3((unsigned)grid), dim3(256), stream, out, blocks, ctr_lo, ctr_hi, key);
    return vt_check_launch("vt_philox_u32");
}

extern "C" int vt_randn(float* out, int64_t n, int64_t offset, uint64_t key, uint64_t stream_id, vt_stream stream) {
    VT_REQUIRE(n >= 0 && offset >= 0, "vt_randn: negative n or offset");
    if (n == 0) return VT_OK;
    VT_REQUIRE(out, "vt_randn: null output");
    VT_REQUIRE(offset <= INT64_MAX - n, "vt_randn: offset + n overflows");
    const int64_t j0 = offset >> 2;
    const int64_t nblocks = ((offset + n - 1) >> 2) - j0 + 1;
    const int64_t grid = (nblocks + 255) / 256;
    VT_REQUIRE(grid < ((int64_t)1 << 31), "vt_randn: %lld elements are too many", (long long)n);
    // block j starts at out + 4 j - offset: with offset % 4 == 0 that is out + a multiple of 16 bytes
    const int vec = (offset % 4 == 0) && ((uintptr_t)out % 16 == 0);
    VT_LAUNCH(randn_kernel, dim3((unsigned)grid), dim3(256), stream, out, n, offset, j0, nblocks, key, stream_id, vec);
    return vt_check_launch("vt_randn");
}

extern "C" int vt_noise_bias_act(void* out, int ld_out, const void* x, int ld_x, const float* noise, int nb, const float* w,
                                 const float* bias, int B, int HW, int C, int dtype, vt_stream stream) {
    VT_REQUIRE(out && x && noise && w, "vt_noise_bias_act: null pointer");
    VT_REQUIRE(B >= 1 && HW >= 1 && C >= 1, "vt_noise_bias_act: sizes must be >= 1 (B %d, HW %d, C %d)", B, HW, C);
    VT_REQUIRE(nb == 1 || nb == B, "vt_noise_bias_act: noise batch %d is neither 1 nor B = %d", nb, B);
    VT_REQUIRE(ld_out >= C && ld_x >= C, "vt_noise_bias_act: row stride below C (ld_out %d, ld_x %d, C %d)", ld_out, ld_x, C);
    if (C % 8 != 0) {
        vt_set_error("vt_noise_bias_act: C = %d is not a multiple of 8", C);
        return VT_ERR_UNSUPPORTED;
    }
    switch (dtype) {
        case VT_F32:
            return launch_nba<float>(out, ld_out, x, ld_x, noise, nb, w, bias, B, HW, C, stream);
        case VT_BF16:
            return launch_nba<bf16_t>(out, ld_out, x, ld_x, noise, nb, w, bias, B, HW, C, stream);
        case VT_F16:
            return launch_nba<f16_t>(out, ld_out, x, ld_x, noise, nb, w, bias, B, HW, C, stream);
    }
    vt_set_error("vt_noise_bias_act: unsupported dtype %d", dtype);
    return VT_ERR_UNSUPPORTED;
}

extern "C" int vt_lerp_rows(float* out, int ld_out, const float* a, int ld_a, const float* b, int ld_b, const float* f,
                            int f_stride, int rows, int dim, vt_stream stream) {
    VT_REQUIRE(out && a && b && f, "vt_lerp_rows: null pointer");
    VT_REQUIRE(rows >= 1 && dim >= 1, "vt_lerp_rows: sizes must be >= 1 (rows %d, dim %d)", rows, dim);
    VT_REQUIRE(ld_out >= dim && (ld_a == 0 || ld_a >= dim) && (ld_b == 0 || ld_b >= dim),
               "vt_lerp_rows: bad row stride (ld_out %d, ld_a %d, ld_b %d, dim %d)", ld_out, ld_a, ld_b, dim);
    VT_REQUIRE(f_stride == 0 || f_stride == 1, "vt_lerp_rows: f_stride %d is neither 0 nor 1", f_stride);
    int64_t grid = ((int64_t)rows * dim + 255) / 256;
    if (grid > 4096) grid = 4096;
    VT_LAUNCH(lerp_rows_kernel, dim3((unsigned)grid), dim3(256), stream, out, ld_out, a, ld_a, b, ld_b, f, f_stride, rows, dim);
    return vt_check_launch("vt_lerp_rows");
}
