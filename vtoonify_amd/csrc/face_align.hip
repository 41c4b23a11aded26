// Face alignment for the style encoder from given landmarks (gfx950): what model/encoder/align_all_parallel.py:108-145 does on
// the host with Pillow, numpy and scipy.ndimage, as three entries; the plan (quad, shrink, crop box, pads) is host work
// (vtoonify_amd/align.py).  Arithmetic: DESIGN.md 4.9.
//
//   vt_align_resample_u8   Pillow's 8-bit LANCZOS resize of a region: both passes in ONE launch, integer arithmetic
//   vt_align_pad_blend     reflect pad + float64-accumulated Gaussian + mask blend + exact per-channel median + blend + rint
//   vt_align_quad          Pillow's QUAD transform with BILINEAR sampling in float64, plus the normalised float32 planes
//
// Resample: one workgroup = one output tile.  It stages the tile's bounds in LDS, derives the source footprint from them, loads
// the footprint with byte-consecutive lanes, runs the horizontal pass LDS -> LDS (uint8 between the passes, as Pillow keeps it)
// and the vertical pass LDS -> global.  Pad blend: six small launches over an image of at most ~1100 x 1100 pixels -- the
// column blur reads the byte rows of the view directly (lanes walk a row), the row blur stages a row segment with its halo in
// LDS; the median is a radix select over the order-preserving integer image of the float bits, one histogram launch per byte,
// each launch deriving the prefixes so far from the histograms before it.  Quad: one wave per strip of 64 pixels of an output
// row.  The library is built with -ffp-contract=off: no product here is fused into an addition.
#include <math.h>

#include <vector>

#include "vt_common.hpp"
#include "../../include/vtoonify_amd_align.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ resample
constexpr int AR_THREADS = 256;
constexpr int AR_LDS_A = 40960;   // bytes of the source footprint (row pitch 3 * width)
constexpr int AR_LDS_T = 8192;    // bytes of the horizontally filtered footprint (3 * tile width per row)
constexpr int AR_TW_MAX = 32, AR_TH_MAX = 16;
constexpr int AR_BITS = 22;       // Pillow's PRECISION_BITS for 8-bit images

__device__ __forceinline__ unsigned char al_clip8(int acc) {
    const int v = acc >> AR_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ void __launch_bounds__(AR_THREADS)
align_resample_kernel(unsigned char* __restrict__ out, const unsigned char* __restrict__ src, int row0, int Ws,
                      const int* __restrict__ xb, const int* __restrict__ xk, int kx, const int* __restrict__ yb,
                      const int* __restrict__ yk, int ky, int H, int W, int th_, int tw_) {
    __shared__ uint32_t sAw[AR_LDS_A / 4];
    __shared__ unsigned char sT[AR_LDS_T];
    __shared__ int sXB[AR_TW_MAX * 2], sYB[AR_TH_MAX * 2];
    unsigned char* const sA = reinterpret_cast<unsigned char*>(sAw);
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * tw_, oy0 = blockIdx.y * th_;
    const int tw = W - ox0 < tw_ ? W - ox0 : tw_, th = H - oy0 < th_ ? H - oy0 : th_;

    if (tid < tw * 2) sXB[tid] = xb[ox0 * 2 + tid];
    if (tid >= 128 && tid - 128 < th * 2) sYB[tid - 128] = yb[oy0 * 2 + tid - 128];
    __syncthreads();

    int fx0 = sXB[0], fx1 = sXB[0] + sXB[1], fy0 = sYB[0], fy1 = sYB[0] + sYB[1];
    for (int i = 1; i < tw; ++i) {
        const int a = sXB[2 * i], b = a + sXB[2 * i + 1];
        fx0 = a < fx0 ? a : fx0, fx1 = b > fx1 ? b : fx1;
    }
    for (int i = 1; i < th; ++i) {
        const int a = sYB[2 * i], b = a + sYB[2 * i + 1];
        fy0 = a < fy0 ? a : fy0, fy1 = b > fy1 ? b : fy1;
    }
    const int fh = fy1 - fy0, rowbytes = 3 * (fx1 - fx0), orow = 3 * tw;

    // ---- footprint -> LDS: consecutive lanes fetch consecutive bytes of a source row
    {
        const unsigned char* const foot = src + ((int64_t)(fy0 - row0) * Ws + fx0) * 3;
        const int items = fh * rowbytes;
        for (int i = tid; i < items; i += AR_THREADS) {
            const int r = i / rowbytes, b = i - r * rowbytes;
            sA[i] = foot[(int64_t)r * Ws * 3 + b];
        }
    }
    __syncthreads();
    // ---- horizontal pass, every footprint row: LDS -> LDS, uint8
    {
        const int items = fh * orow;
        for (int i = tid; i < items; i += AR_THREADS) {
            const int r = i / orow, e = i - r * orow;
            const int col = e / 3, c = e - 3 * col;
            const int first = sXB[2 * col], cnt = sXB[2 * col + 1];
            const int* k = xk + (int64_t)(ox0 + col) * kx;
            const unsigned char* p = sA + r * rowbytes + 3 * (first - fx0) + c;
            int acc = 1 << (AR_BITS - 1);
            for (int j = 0; j < cnt; ++j) acc += k[j] * (int)p[3 * j];
            sT[i] = al_clip8(acc);
        }
    }
    __syncthreads();
    // ---- vertical pass: LDS -> global, consecutive lanes write consecutive bytes of an output row
    {
        const int items = th * orow;
        for (int i = tid; i < items; i += AR_THREADS) {
            const int r = i / orow, e = i - r * orow;
            const int first = sYB[2 * r], cnt = sYB[2 * r + 1];
            const int* k = yk + (int64_t)(oy0 + r) * ky;
            const unsigned char* p = sT + (first - fy0) * orow + e;
            int acc = 1 << (AR_BITS - 1);
            for (int j = 0; j < cnt; ++j) acc += k[j] * (int)p[j * orow];
            out[((int64_t)(oy0 + r) * W + ox0) * 3 + e] = al_clip8(acc);
        }
    }
}

int al_fetch(std::vector<int>& host, const int32_t* tab, size_t count) {
    host.resize(count);
#ifdef VT_EMU
    memcpy(host.data(), tab, count * sizeof(int));
    return 0;
#else
    return hipMemcpy(host.data(), tab, count * sizeof(int), hipMemcpyDefault) == hipSuccess ? 0 : 1;
#endif
}

// widest source extent of any tile of `tile` outputs along one axis
int al_max_extent(const std::vector<int>& bound, int count, int tile) {
    int best = 0;
    for (int t0 = 0; t0 < count; t0 += tile) {
        int lo = bound[2 * t0], hi = lo + bound[2 * t0 + 1];
        for (int i = t0; i < count && i < t0 + tile; ++i) {
            const int a = bound[2 * i], b = a + bound[2 * i + 1];
            lo = a < lo ? a : lo, hi = b > hi ? b : hi;
        }
        best = hi - lo > best ? hi - lo : best;
    }
    return best;
}

// ----------------------------------------------------------------------------------------------------------- pad blend
constexpr int AP_THREADS = 256;
constexpr int AP_SEG = 256;                                   // pixels of a row that one workgroup of the row blur filters
constexpr int AP_HIST = 4 * 3 * 2 * 256;                      // ints: [byte pass][channel][lower / upper middle][bin]
constexpr int AP_MAX_BLOCKS = 2048;

struct ApGeom {
    int h0, w0, pitch, pl, pt, pr, pb, h, w, r;
};

// numpy's 'reflect' (the edge sample is not repeated) of a view of n samples extended by less than n
__device__ __forceinline__ int ap_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// scipy.ndimage's 'reflect' (the edge sample repeats) for a reach below n
__device__ __forceinline__ int ap_symm(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

__device__ __forceinline__ float ap_div(float a, float b) {
#ifdef VT_EMU
    return a / b;
#else
    return __fdiv_rn(a, b);
#endif
}

__device__ __forceinline__ float ap_pixel(const unsigned char* __restrict__ src, const ApGeom& g, int y, int x, int c) {
    return (float)src[(int64_t)ap_reflect(y - g.pt, g.h0) * g.pitch + 3 * ap_reflect(x - g.pl, g.w0) + c];
}

__device__ __forceinline__ float ap_mask(const ApGeom& g, int y, int x) {
    const float mx = fminf(ap_div((float)x, (float)g.pl), ap_div((float)(g.w - 1 - x), (float)g.pr));
    const float my = fminf(ap_div((float)y, (float)g.pt), ap_div((float)(g.h - 1 - y), (float)g.pb));
    return fmaxf(1.0f - mx, 1.0f - my);
}

__device__ __forceinline__ float ap_clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// order-preserving integer image of a float
__device__ __forceinline__ uint32_t ap_key(float f) {
    const uint32_t u = vt_f2u(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ap_unkey(uint32_t k) { return vt_u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Radix select, the part between two histogram launches.  Selection s = 2 c + which (channel c, lower / upper middle value)
// has a rank among the n keys of its channel; the histograms of byte passes 0 .. p-1 fix the top p bytes of its key.  Called
// by every thread of the workgroup: per pass the 6 x 256 bins come into LDS with one coalesced load, six lanes walk them.
__device__ void ap_select(uint32_t* sPrefix, int* sRank, int* sBins, const int* __restrict__ hist, int n, int p) {
    const int tid = threadIdx.x;
    if (tid < 6) {
        sRank[tid] = (tid & 1) ? n / 2 : (n - 1) / 2;
        sPrefix[tid] = 0u;
    }
    for (int q = 0; q < p; ++q) {
        for (int i = tid; i < 6 * 256; i += AP_THREADS) {
            const int sel = i >> 8;                                                    // (pass 0 has no prefix: one histogram)
            sBins[i] = hist[((q * 3 + (sel >> 1)) * 2 + (q == 0 ? 0 : (sel & 1))) * 256 + (i & 255)];
        }
        __syncthreads();
        if (tid < 6) {
            const int* bins = sBins + tid * 256;
            const int rank = sRank[tid];
            int cum = 0, bin = 255;
            for (int k = 0; k < 256; ++k) {
                const int cnt = bins[k];
                if (rank < cum + cnt) {
                    bin = k;
                    break;
                }
                cum += cnt;
            }
            sRank[tid] = rank - cum;
            sPrefix[tid] = (sPrefix[tid] << 8) | (uint32_t)bin;
        }
        __syncthreads();
    }
}

// columns: B0[y,x,c] = float(sum over rows in float64); block 0 also clears the histograms
__global__ void __launch_bounds__(AP_THREADS)
align_blur_cols_kernel(float* __restrict__ b0, int* __restrict__ hist, const unsigned char* __restrict__ src, ApGeom g,
                       const double* __restrict__ taps) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < AP_HIST; i += AP_THREADS) hist[i] = 0;
    const int row = 3 * g.w, total = g.h * row;
    for (int e = blockIdx.x * AP_THREADS + threadIdx.x; e < total; e += gridDim.x * AP_THREADS) {
        const int y = e / row, rem = e - y * row;
        const int x = rem / 3, c = rem - 3 * x;
        double acc = (double)ap_pixel(src, g, y, x, c) * taps[0];
        for (int j = g.r; j > 0; --j)
            acc += ((double)ap_pixel(src, g, ap_symm(y - j, g.h), x, c) + (double)ap_pixel(src, g, ap_symm(y + j, g.h), x, c)) * taps[j];
        b0[e] = (float)acc;
    }
}

// rows: blur of B0 along x from a row segment staged in LDS with its halo, then the first blend; histogram of the top byte
__global__ void __launch_bounds__(AP_THREADS)
align_blur_rows_blend_kernel(float* __restrict__ img, int* __restrict__ hist, const float* __restrict__ b0,
                             const unsigned char* __restrict__ src, ApGeom g, const double* __restrict__ taps) {
    __shared__ float sRow[(AP_SEG + 2 * VT_ALIGN_MAX_RADIUS) * 3];
    __shared__ int sHist[3 * 256];
    const int tid = threadIdx.x;
    const int y = blockIdx.y, x0 = blockIdx.x * AP_SEG;
    const int seg = g.w - x0 < AP_SEG ? g.w - x0 : AP_SEG;
    for (int i = tid; i < 3 * 256; i += AP_THREADS) sHist[i] = 0;
    const float* const line = b0 + (int64_t)y * g.w * 3;
    for (int i = tid; i < (seg + 2 * g.r) * 3; i += AP_THREADS) {
        const int px = i / 3, c = i - 3 * px;
        sRow[i] = line[3 * ap_symm(x0 - g.r + px, g.w) + c];
    }
    __syncthreads();
    for (int i = tid; i < seg * 3; i += AP_THREADS) {
        const int xl = i / 3, c = i - 3 * xl;
        const float* p = sRow + 3 * g.r + i;
        double acc = (double)p[0] * taps[0];
        for (int j = g.r; j > 0; --j) acc += ((double)p[-3 * j] + (double)p[3 * j]) * taps[j];
        const float blur = (float)acc;
        const int x = x0 + xl;
        const float v = ap_pixel(src, g, y, x, c);
        const float m = ap_mask(g, y, x);
        const float t = (blur - v) * ap_clip01(m * 3.0f + 1.0f);
        const float o = v + t;
        img[((int64_t)y * g.w + x0) * 3 + i] = o;
        atomicAdd(&sHist[c * 256 + (int)(ap_key(o) >> 24)], 1);
    }
    __syncthreads();
    for (int i = tid; i < 3 * 256; i += AP_THREADS)
        if (sHist[i]) atomicAdd(&hist[(i >> 8) * 512 + (i & 255)], sHist[i]);      // pass 0: [c][0][bin]
}

// byte pass p = 1..3 of the radix select: histogram of byte p of the keys whose top p bytes equal a selection's prefix
__global__ void __launch_bounds__(AP_THREADS)
align_median_hist_kernel(int* __restrict__ hist, const float* __restrict__ img, int n, int p) {
    __shared__ int sHist[6 * 256], sBins[6 * 256], sRank[6];
    __shared__ uint32_t sPrefix[6];
    const int tid = threadIdx.x;
    for (int i = tid; i < 6 * 256; i += AP_THREADS) sHist[i] = 0;
    ap_select(sPrefix, sRank, sBins, hist, n, p);          // (ends on a barrier)
    const int hi = 32 - 8 * p, lo = 24 - 8 * p;
    for (int e = blockIdx.x * AP_THREADS + tid; e < 3 * n; e += gridDim.x * AP_THREADS) {
        const int c = e % 3;
        const uint32_t k = ap_key(img[e]);
        const int bin = (int)((k >> lo) & 255u);
        if ((k >> hi) == sPrefix[2 * c]) atomicAdd(&sHist[(2 * c) * 256 + bin], 1);
        if ((k >> hi) == sPrefix[2 * c + 1]) atomicAdd(&sHist[(2 * c + 1) * 256 + bin], 1);
    }
    __syncthreads();
    int* const hp = hist + p * (3 * 2 * 256);
    for (int i = tid; i < 6 * 256; i += AP_THREADS)
        if (sHist[i]) atomicAdd(&hp[i], sHist[i]);
}

// the median from the four histograms, the second blend and the rounding to uint8
__global__ void __launch_bounds__(AP_THREADS)
align_median_blend_kernel(unsigned char* __restrict__ out, const int* __restrict__ hist, const float* __restrict__ img, ApGeom g) {
    __shared__ int sBins[6 * 256], sRank[6];
    __shared__ uint32_t sPrefix[6];
    const int tid = threadIdx.x, n = g.h * g.w;
    ap_select(sPrefix, sRank, sBins, hist, n, 4);          // (ends on a barrier)
    const int row = 3 * g.w;
    for (int e = blockIdx.x * AP_THREADS + tid; e < 3 * n; e += gridDim.x * AP_THREADS) {
        const int y = e / row, rem = e - y * row;
        const int x = rem / 3, c = rem - 3 * x;
        const float med = (ap_unkey(sPrefix[2 * c]) + ap_unkey(sPrefix[2 * c + 1])) / 2.0f;
        const float v = img[e];
        const float t = (med - v) * ap_clip01(ap_mask(g, y, x));
        const float o = rintf(v + t);
        out[e] = (unsigned char)(int)fminf(fmaxf(o, 0.0f), 255.0f);
    }
}

int64_t ap_ws_bytes(int h, int w) { return 2 * (int64_t)h * w * 3 * (int64_t)sizeof(float) + (int64_t)AP_HIST * (int64_t)sizeof(int); }

// ---------------------------------------------------------------------------------------------------------------- quad
struct AqCoef {
    double a[8];
};

__global__ void __launch_bounds__(64)
align_quad_kernel(unsigned char* __restrict__ out_u8, float* __restrict__ out_f32, const unsigned char* __restrict__ img, int h,
                  int w, int pitch, AqCoef q, int S) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    if (x >= S) return;
    const double xo = (double)x + 0.5, yo = (double)y + 0.5;
    double xin = q.a[0] + q.a[1] * xo + q.a[2] * yo + q.a[3] * xo * yo;
    double yin = q.a[4] + q.a[5] * xo + q.a[6] * yo + q.a[7] * xo * yo;
    unsigned char v[3] = {0, 0, 0};
    if (!(xin < 0.0 || xin >= (double)w || yin < 0.0 || yin >= (double)h) && xin == xin && yin == yin) {
        xin -= 0.5, yin -= 0.5;
        const double fx = floor(xin), fy = floor(yin);
        const double dx = xin - fx, dy = yin - fy;
        const int ix = (int)fx, iy = (int)fy;
        const int xa = ix < 0 ? 0 : ix, xb = ix + 1 > w - 1 ? w - 1 : ix + 1;
        const int ya = iy < 0 ? 0 : iy, yb = iy + 1 > h - 1 ? h - 1 : iy + 1;
        const unsigned char* ra = img + (int64_t)ya * pitch;
        const unsigned char* rb = img + (int64_t)yb * pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p00 = ra[3 * xa + c], p01 = ra[3 * xb + c], p10 = rb[3 * xa + c], p11 = rb[3 * xb + c];
            const double v1 = p00 + (p01 - p00) * dx;
            const double v2 = p10 + (p11 - p10) * dx;
            v[c] = (unsigned char)(int)(v1 + (v2 - v1) * dy);
        }
    }
    unsigned char* o = out_u8 + ((int64_t)y * S + x) * 3;
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
    if (out_f32) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = ap_div((float)v[c], 255.0f);
            out_f32[((int64_t)c * S + y) * S + x] = ap_div(f - 0.5f, 0.5f);
        }
    }
}

}  // namespace

extern "C" int vt_align_resample_u8(uint8_t* out, const uint8_t* src, int rows, int row0, int Hs, int Ws, const int32_t* xbound,
                                    const int32_t* xcoef, int kx, const int32_t* ybound, const int32_t* ycoef, int ky, int H,
                                    int W, vt_stream stream) {
    VT_REQUIRE(out && src && xbound && xcoef && ybound && ycoef, "vt_align_resample_u8: null tensor");
    VT_REQUIRE(Hs > 0 && Ws > 0 && H > 0 && W > 0 && H <= 65535 && W <= (1 << 20), "vt_align_resample_u8: bad sizes");
    VT_REQUIRE(kx > 0 && ky > 0 && kx <= 4096 && ky <= 4096, "vt_align_resample_u8: table widths kx = %d, ky = %d (1..4096)", kx, ky);
    VT_REQUIRE(rows > 0 && row0 >= 0 && row0 <= Hs - rows, "vt_align_resample_u8: slab rows [%d, %d) outside the image (%d rows)",
               row0, row0 + rows, Hs);
    VT_REQUIRE((int64_t)rows * Ws * 3 < ((int64_t)1 << 31), "vt_align_resample_u8: slab of %d x %d pixels too large", rows, Ws);
    std::vector<int> xb, yb;
    if (al_fetch(xb, xbound, (size_t)W * 2) || al_fetch(yb, ybound, (size_t)H * 2)) {
        vt_set_error("vt_align_resample_u8: cannot read the tables");
        return VT_ERR_LAUNCH;
    }
    for (int i = 0; i < W; ++i) {
        const int first = xb[2 * i], cnt = xb[2 * i + 1];
        VT_REQUIRE(cnt >= 1 && cnt <= kx, "vt_align_resample_u8: xbound[%d] counts %d taps, the table is %d wide", i, cnt, kx);
        VT_REQUIRE(first >= 0 && first <= Ws - cnt, "vt_align_resample_u8: xbound[%d] = columns [%d, %d) outside the image (Ws %d)",
                   i, first, first + cnt, Ws);
    }
    for (int i = 0; i < H; ++i) {
        const int first = yb[2 * i], cnt = yb[2 * i + 1];
        VT_REQUIRE(cnt >= 1 && cnt <= ky, "vt_align_resample_u8: ybound[%d] counts %d taps, the table is %d wide", i, cnt, ky);
        VT_REQUIRE(first >= 0 && first <= Hs - cnt, "vt_align_resample_u8: ybound[%d] = rows [%d, %d) outside the image (Hs %d)", i,
                   first, first + cnt, Hs);
        VT_REQUIRE(first >= row0 && first + cnt <= row0 + rows,
                   "vt_align_resample_u8: ybound[%d] reads rows [%d, %d), the slab holds [%d, %d)", i, first, first + cnt, row0,
                   row0 + rows);
    }
    int th = 0, tw = 0;
    const int tiles[3][2] = {{AR_TH_MAX, AR_TW_MAX}, {8, 16}, {4, 8}};
    for (const auto& t : tiles) {
        const int fh = al_max_extent(yb, H, t[0]), fw = al_max_extent(xb, W, t[1]);
        if ((int64_t)fh * 3 * fw <= AR_LDS_A && (int64_t)fh * 3 * t[1] <= AR_LDS_T) {
            th = t[0], tw = t[1];
            break;
        }
    }
    if (!th) {
        vt_set_error("vt_align_resample_u8: the source footprint of a 4 x 8 output tile does not fit %d bytes of LDS (shrink "
                     "factors up to 8 are supported)", AR_LDS_A + AR_LDS_T);
        return VT_ERR_UNSUPPORTED;
    }
    auto k = align_resample_kernel;
    VT_LAUNCH(k, dim3(vt_cdiv(W, tw), vt_cdiv(H, th)), dim3(AR_THREADS), stream, (unsigned char*)out, (const unsigned char*)src, row0,
              Ws, (const int*)xbound, (const int*)xcoef, kx, (const int*)ybound, (const int*)ycoef, ky, H, W, th, tw);
    return vt_check_launch("vt_align_resample_u8");
}

extern "C" int64_t vt_align_pad_blend_workspace(int h, int w, int r) {
    if (h < 1 || w < 1 || h > 16384 || w > 16384 || r < 0 || r > VT_ALIGN_MAX_RADIUS) {
        vt_set_error("vt_align_pad_blend_workspace: image %d x %d (1..16384), radius %d (0..%d)", h, w, r, VT_ALIGN_MAX_RADIUS);
        return 0;
    }
    return ap_ws_bytes(h, w);
}

extern "C" int vt_align_pad_blend(uint8_t* out, const uint8_t* src, int h0, int w0, int pitch, int pad_l, int pad_t, int pad_r,
                                  int pad_b, const double* taps, int r, void* ws, int64_t ws_bytes, vt_stream stream) {
    VT_REQUIRE(out && src && taps && ws, "vt_align_pad_blend: null tensor");
    VT_REQUIRE(h0 > 0 && w0 > 0 && h0 <= 16384 && w0 <= 16384 && pitch >= 3 * w0, "vt_align_pad_blend: view %d x %d, pitch %d", h0,
               w0, pitch);
    VT_REQUIRE(pad_l >= 1 && pad_t >= 1 && pad_r >= 1 && pad_b >= 1,
               "vt_align_pad_blend: pads (%d, %d, %d, %d): the mask divides by each of them, none may be 0", pad_l, pad_t, pad_r, pad_b);
    VT_REQUIRE(pad_l < w0 && pad_r < w0 && pad_t < h0 && pad_b < h0,
               "vt_align_pad_blend: pads (%d, %d, %d, %d) reach the side of the %d x %d view they reflect", pad_l, pad_t, pad_r, pad_b,
               w0, h0);
    const int h = h0 + pad_t + pad_b, w = w0 + pad_l + pad_r;
    VT_REQUIRE(h <= 16384 && w <= 16384 && (int64_t)h * w * 3 < ((int64_t)1 << 30), "vt_align_pad_blend: padded image %d x %d too large", h, w);
    VT_REQUIRE(r >= 0 && r < h && r < w, "vt_align_pad_blend: radius %d (0 .. below the padded sides %d, %d)", r, h, w);
    if (r > VT_ALIGN_MAX_RADIUS) {
        vt_set_error("vt_align_pad_blend: radius %d beyond the %d a row segment's halo holds in LDS", r, VT_ALIGN_MAX_RADIUS);
        return VT_ERR_UNSUPPORTED;
    }
    VT_REQUIRE(ws_bytes >= ap_ws_bytes(h, w) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)taps & 7) == 0,
               "vt_align_pad_blend: workspace of %lld bytes, %lld needed (8-byte aligned, as the taps)", (long long)ws_bytes,
               (long long)ap_ws_bytes(h, w));
    ApGeom g = {h0, w0, pitch, pad_l, pad_t, pad_r, pad_b, h, w, r};
    const int n = h * w;
    float* b0 = (float*)ws;
    float* img = b0 + (int64_t)n * 3;
    int* hist = (int*)(img + (int64_t)n * 3);
    int blocks = vt_cdiv((int64_t)n * 3, AP_THREADS);
    blocks = blocks > AP_MAX_BLOCKS ? AP_MAX_BLOCKS : blocks;
    auto kc = align_blur_cols_kernel;
    VT_LAUNCH(kc, dim3(blocks), dim3(AP_THREADS), stream, b0, hist, (const unsigned char*)src, g, taps);
    auto kr = align_blur_rows_blend_kernel;
    VT_LAUNCH(kr, dim3(vt_cdiv(w, AP_SEG), h), dim3(AP_THREADS), stream, img, hist, (const float*)b0, (const unsigned char*)src, g, taps);
    auto kh = align_median_hist_kernel;
    for (int p = 1; p < 4; ++p) VT_LAUNCH(kh, dim3(blocks), dim3(AP_THREADS), stream, hist, (const float*)img, n, p);
    auto kb = align_median_blend_kernel;
    VT_LAUNCH(kb, dim3(blocks), dim3(AP_THREADS), stream, (unsigned char*)out, (const int*)hist, (const float*)img, g);
    return vt_check_launch("vt_align_pad_blend");
}

extern "C" int vt_align_quad(uint8_t* out_u8, float* out_f32, const uint8_t* img, int h, int w, int pitch, const double* a, int S,
                             vt_stream stream) {
    VT_REQUIRE(out_u8 && img && a, "vt_align_quad: null pointer");
    VT_REQUIRE(h > 0 && w > 0 && h <= 65535 && w <= 65535 && pitch >= 3 * w, "vt_align_quad: view %d x %d, pitch %d", h, w, pitch);
    VT_REQUIRE(S > 0 && S <= 4096, "vt_align_quad: output size %d (1..4096)", S);
    AqCoef q;
    for (int i = 0; i < 8; ++i) {
        VT_REQUIRE(a[i] == a[i] && fabs(a[i]) <= 1e300, "vt_align_quad: coefficient a[%d] is not finite", i);
        q.a[i] = a[i];
    }
    auto k = align_quad_kernel;
    VT_LAUNCH(k, dim3(vt_cdiv(S, 64), S), dim3(64), stream, (unsigned char*)out_u8, out_f32, (const unsigned char*)img, h, w, pitch, q, S);
    return vt_check_launch("vt_align_quad");
}
