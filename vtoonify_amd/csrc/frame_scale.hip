// --scale_image on the GPU (gfx950): low-pass filter, bilinear resize and crop of source-size uint8 frames in ONE launch --
// what the reference does per frame on the host with cv2.sepFilter2D (once or twice over the whole frame), cv2.resize of the
// whole frame and a slice (style_transfer.py:113-127,150-155).
//
//   vt_frame_scale_crop   src (n,rows,Ws,3) uint8, source rows [row0, row0+rows) of Hs x Ws frames -> out (n,H,W,3) uint8
//
// Arithmetic (integer only, so a numpy restatement matches bit for bit):
//   blur pass    B[y,x] = (sum_i sum_j k_i k_j P[r(y+o_i), r(x+o_j)] + 32768) >> 16,  k = (32,96,96,32) at offsets (-2,-1,0,+1),
//                r = reflect-101 in FULL-FRAME coordinates; done separably: the row sums fit uint16 (<= 256*255), the column
//                sums int32, one rounding.  `passes` of them (0..2), each on the uint8 result of the one before.
//   resize       the host's tables give, per output column, x0 x1 a0 a1 and, per output row, y0 y1 b0 b1 (weights of 2048):
//                h_r = a0 Q[r,x0] + a1 Q[r,x1];  out = (((b0 (h_y0 >> 4)) >> 16) + ((b1 (h_y1 >> 4)) >> 16) + 2) >> 2
//
// One workgroup = one output tile (32x32, 16x16 or 8x8, picked by the launcher so that the footprint fits the LDS below).
// It stages its slice of the tables in LDS, derives the source footprint from them (first / last x0..x1, y0..y1, widened per
// pass by 2 left / up and 1 right / down and by what reflect-101 reaches at a frame border), loads the footprint once with
// aligned 4-byte loads (a row of 3-byte pixels starts at any byte: the LDS image keeps the row's byte phase), runs the passes
// LDS -> LDS (rows into a uint16 plane, columns back into the uint8 plane), interpolates from LDS and writes packed 32-bit
// words.  No intermediate image goes to global memory.
// Algorithmic bytes: n*rows*Ws*3 + n*H*W*3.
#include <vector>

#include "vt_common.hpp"
#include "../../include/vtoonify_amd_frames.h"

namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_TILE_MAX = 32;
constexpr int FS_LDS_A = 21504;   // bytes of the uint8 plane (row pitch: 3 * width + byte phase, rounded up to 4)
constexpr int FS_LDS_T = 20480;   // uint16 elements of the row-filtered plane (3 * width * height)

struct FsRange {
    int lo, hi;
};

__host__ __device__ inline int fs_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// what one blur pass over [lo, hi] reads of an axis of length n >= 3: [lo-2, hi+1], reflected into the frame
__host__ __device__ inline FsRange fs_expand(FsRange r, int n) {
    const int lo = r.lo - 2, hi = r.hi + 1;
    FsRange e;
    e.lo = lo < 0 ? 0 : lo;
    e.hi = hi > n - 1 ? n - 1 : hi;
    if (lo < 0 && -lo > e.hi) e.hi = -lo;
    if (hi > n - 1 && 2 * (n - 1) - hi < e.lo) e.lo = 2 * (n - 1) - hi;
    return e;
}

__host__ __device__ inline int fs_pitch(int fw) { return (3 * fw + 6) & ~3; }

// flat item index -> (row, column) for a stride of FS_THREADS items, without a division per item
struct FsWalk {
    int r, c, dr, dc, w;
    __device__ FsWalk(int first, int width) : r(first / width), c(first % width), dr(FS_THREADS / width), dc(FS_THREADS % width), w(width) {}
    __device__ void next() {
        r += dr;
        c += dc;
        if (c >= w) {
            c -= w;
            ++r;
        }
    }
};

__global__ void __launch_bounds__(FS_THREADS)
frame_scale_crop_kernel(unsigned char* __restrict__ out, const unsigned char* __restrict__ src, int64_t src_bytes, int rows,
                        int row0, int Hs, int Ws, int passes, const int* __restrict__ xtab, const int* __restrict__ ytab,
                        int H, int W, int tile) {
    __shared__ uint32_t sAw[FS_LDS_A / 4];
    __shared__ unsigned short sT[FS_LDS_T];
    __shared__ int sX[FS_TILE_MAX * 4], sY[FS_TILE_MAX * 4];
    unsigned char* const sA = reinterpret_cast<unsigned char*>(sAw);
    const int tid = threadIdx.x;
    const int img = blockIdx.z;
    const int ox0 = blockIdx.x * tile, oy0 = blockIdx.y * tile;
    const int tw = W - ox0 < tile ? W - ox0 : tile, th = H - oy0 < tile ? H - oy0 : tile;

    if (tid < tw * 4) sX[tid] = xtab[ox0 * 4 + tid];
    if (tid >= 128 && tid - 128 < th * 4) sY[tid - 128] = ytab[oy0 * 4 + tid - 128];
    __syncthreads();

    // levels of the tile, from the interpolation's reads outwards: q0 is read of the frame after `passes` passes
    FsRange x0r, y0r;
    x0r.lo = sX[0], x0r.hi = sX[1], y0r.lo = sY[0], y0r.hi = sY[1];
    for (int i = 0; i < tw; ++i) {
        const int a = sX[4 * i], b = sX[4 * i + 1];
        x0r.lo = a < x0r.lo ? a : x0r.lo, x0r.lo = b < x0r.lo ? b : x0r.lo;
        x0r.hi = a > x0r.hi ? a : x0r.hi, x0r.hi = b > x0r.hi ? b : x0r.hi;
    }
    for (int i = 0; i < th; ++i) {
        const int a = sY[4 * i], b = sY[4 * i + 1];
        y0r.lo = a < y0r.lo ? a : y0r.lo, y0r.lo = b < y0r.lo ? b : y0r.lo;
        y0r.hi = a > y0r.hi ? a : y0r.hi, y0r.hi = b > y0r.hi ? b : y0r.hi;
    }
    const FsRange x1r = passes >= 1 ? fs_expand(x0r, Ws) : x0r, y1r = passes >= 1 ? fs_expand(y0r, Hs) : y0r;
    const FsRange x2r = passes >= 2 ? fs_expand(x1r, Ws) : x1r, y2r = passes >= 2 ? fs_expand(y1r, Hs) : y1r;
    const int fx0 = x2r.lo, fy0 = y2r.lo, fw = x2r.hi - x2r.lo + 1, fh = y2r.hi - y2r.lo + 1;
    const int pitch = fs_pitch(fw);

    // ---- footprint -> LDS: rows fy0.. of the slab, bytes 3*fx0 .. 3*(fx0+fw) of each, fetched as the aligned 4-byte words
    // that cover them; a row's first pixel sits at byte `phase` of its LDS row
    const unsigned char* const img_src = src + (int64_t)img * rows * Ws * 3;
    const unsigned char* const src_end = src + src_bytes;
    const unsigned char* const foot = img_src + ((int64_t)(fy0 - row0) * Ws + fx0) * 3;
    const unsigned foot_lo = (unsigned)(uintptr_t)foot, row_step = (unsigned)Ws * 3u;
    {
        const int pw = pitch / 4;
        const int items = fh * pw;
        FsWalk it(tid, pw);
        for (int i = tid; i < items; i += FS_THREADS, it.next()) {
            const unsigned char* rowp = foot + (int64_t)it.r * Ws * 3;
            const int phase = (int)((uintptr_t)rowp & 3);
            if (4 * it.c >= phase + 3 * fw) continue;
            const unsigned char* p = rowp - phase + 4 * it.c;
            uint32_t v = 0;
            if (p >= src && p + 4 <= src_end) {
                v = *reinterpret_cast<const uint32_t*>(p);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (p + b >= src && p + b < src_end) v |= (uint32_t)p[b] << (8 * b);
            }
            sAw[it.r * pw + it.c] = v;
        }
    }
    __syncthreads();
#define FS_AOFF(yl) ((yl) * pitch + (int)((foot_lo + (unsigned)(yl) * row_step) & 3u))

    // ---- blur passes, LDS -> LDS
    for (int p = 0; p < passes; ++p) {
        const bool outer = passes - p == 2;
        const FsRange sy = outer ? y2r : y1r, dx = outer ? x1r : x0r, dy = outer ? y1r : y0r;
        const int dw = dx.hi - dx.lo + 1;
        {   // rows: every source row, destination columns
            const int items = (sy.hi - sy.lo + 1) * dw;
            FsWalk it(tid, dw);
            for (int i = tid; i < items; i += FS_THREADS, it.next()) {
                const int yl = sy.lo + it.r - fy0, x = dx.lo + it.c;
                const unsigned char* a = sA + FS_AOFF(yl);
                const int xa = 3 * (fs_reflect(x - 2, Ws) - fx0), xb = 3 * (fs_reflect(x - 1, Ws) - fx0), xc = 3 * (x - fx0),
                          xd = 3 * (fs_reflect(x + 1, Ws) - fx0);
                unsigned short* t = sT + (yl * fw + (x - fx0)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    t[c] = (unsigned short)(32 * (a[xa + c] + a[xd + c]) + 96 * (a[xb + c] + a[xc + c]));
            }
        }
        __syncthreads();
        {   // columns: destination rows and columns, back into the uint8 plane
            const int items = (dy.hi - dy.lo + 1) * dw;
            FsWalk it(tid, dw);
            for (int i = tid; i < items; i += FS_THREADS, it.next()) {
                const int y = dy.lo + it.r, xl = dx.lo + it.c - fx0;
                const unsigned short* ta = sT + ((fs_reflect(y - 2, Hs) - fy0) * fw + xl) * 3;
                const unsigned short* tb = sT + ((fs_reflect(y - 1, Hs) - fy0) * fw + xl) * 3;
                const unsigned short* tc = sT + ((y - fy0) * fw + xl) * 3;
                const unsigned short* td = sT + ((fs_reflect(y + 1, Hs) - fy0) * fw + xl) * 3;
                unsigned char* a = sA + FS_AOFF(y - fy0) + 3 * xl;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    a[c] = (unsigned char)((32 * ((int)ta[c] + (int)td[c]) + 96 * ((int)tb[c] + (int)tc[c]) + 32768) >> 16);
            }
        }
        __syncthreads();
    }

    // ---- interpolate: one item = 4 output bytes of a tile row
    {
        const int rowbytes = 3 * tw;
        const int dpr = (rowbytes + 3) / 4;
        const int items = th * dpr;
        FsWalk it(tid, dpr);
        for (int i = tid; i < items; i += FS_THREADS, it.next()) {
            const int* ye = sY + 4 * it.r;
            const int r0 = FS_AOFF(ye[0] - fy0) - 3 * fx0, r1 = FS_AOFF(ye[1] - fy0) - 3 * fx0;
            const int b0 = ye[2], b1 = ye[3];
            unsigned char* o = out + (((int64_t)img * H + oy0 + it.r) * W + ox0) * 3 + 4 * it.c;
            const int nb = rowbytes - 4 * it.c < 4 ? rowbytes - 4 * it.c : 4;
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < nb) {
                    const int b = 4 * it.c + k;
                    const int px = b / 3, c = b - 3 * px;
                    const int* xe = sX + 4 * px;
                    const int ia = 3 * xe[0] + c, ib = 3 * xe[1] + c;
                    const int h0 = xe[2] * sA[r0 + ia] + xe[3] * sA[r0 + ib], h1 = xe[2] * sA[r1 + ia] + xe[3] * sA[r1 + ib];
                    const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    word |= (uint32_t)(v & 255) << (8 * k);
                }
            }
            if (nb == 4 && ((uintptr_t)o & 3) == 0) {
                *reinterpret_cast<uint32_t*>(o) = word;
            } else {
                for (int k = 0; k < nb; ++k) o[k] = (unsigned char)(word >> (8 * k));
            }
        }
    }
#undef FS_AOFF
}

// widest footprint (along one axis) of any tile of `tile` outputs: entries (lo, hi) per output, `passes` expansions
int fs_max_extent(const std::vector<int>& tab, int count, int tile, int passes, int n) {
    int best = 0;
    for (int t0 = 0; t0 < count; t0 += tile) {
        FsRange r;
        r.lo = tab[4 * t0], r.hi = tab[4 * t0];
        for (int i = t0; i < count && i < t0 + tile; ++i)
            for (int j = 0; j < 2; ++j) {
                const int v = tab[4 * i + j];
                r.lo = v < r.lo ? v : r.lo, r.hi = v > r.hi ? v : r.hi;
            }
        for (int p = 0; p < passes; ++p) r = fs_expand(r, n);
        best = r.hi - r.lo + 1 > best ? r.hi - r.lo + 1 : best;
    }
    return best;
}

// the tables live where the kernel reads them; the launcher checks a host copy of them before anything is launched
int fs_fetch_table(std::vector<int>& host, const int32_t* tab, int count) {
    host.resize((size_t)count * 4);
#ifdef VT_EMU
    memcpy(host.data(), tab, host.size() * sizeof(int));
    return 0;
#else
    return hipMemcpy(host.data(), tab, host.size() * sizeof(int), hipMemcpyDefault) == hipSuccess ? 0 : 1;
#endif
}

}  // namespace

extern "C" int vt_frame_scale_crop(uint8_t* out, const uint8_t* src, int n, int rows, int row0, int Hs, int Ws, int passes,
                                   const int32_t* xtab, const int32_t* ytab, int H, int W, vt_stream stream) {
    VT_REQUIRE(out && src && xtab && ytab, "vt_frame_scale_crop: null tensor");
    VT_REQUIRE(n > 0 && n <= 65535, "vt_frame_scale_crop: n = %d frames (1..65535)", n);
    VT_REQUIRE(passes >= 0 && passes <= 2, "vt_frame_scale_crop: passes = %d (0, 1 or 2 blur passes)", passes);
    VT_REQUIRE(Hs > 0 && Ws > 0 && H > 0 && W > 0 && H <= (1 << 16) && W <= (1 << 16), "vt_frame_scale_crop: bad sizes");
    VT_REQUIRE(passes == 0 || (Hs >= 3 && Ws >= 3), "vt_frame_scale_crop: a blur pass needs a frame of at least 3 x 3");
    VT_REQUIRE(rows > 0 && row0 >= 0 && row0 <= Hs - rows, "vt_frame_scale_crop: slab rows [%d, %d) outside the frame (%d rows)",
               row0, row0 + rows, Hs);
    VT_REQUIRE((int64_t)rows * Ws * 3 < ((int64_t)1 << 31), "vt_frame_scale_crop: slab of %d x %d pixels too large", rows, Ws);
    std::vector<int> xt, yt;
    if (fs_fetch_table(xt, xtab, W) || fs_fetch_table(yt, ytab, H)) {
        vt_set_error("vt_frame_scale_crop: cannot read the tables");
        return VT_ERR_LAUNCH;
    }
    for (int i = 0; i < W; ++i) {
        const int* e = &xt[4 * i];
        VT_REQUIRE(e[0] >= 0 && e[0] < Ws && e[1] >= 0 && e[1] < Ws, "vt_frame_scale_crop: xtab[%d] = (%d, %d) outside the frame (Ws %d)",
                   i, e[0], e[1], Ws);
        VT_REQUIRE(e[2] >= 0 && e[2] <= 2048 && e[3] >= 0 && e[3] <= 2048, "vt_frame_scale_crop: xtab[%d] weights (%d, %d) outside 0..2048",
                   i, e[2], e[3]);
    }
    FsRange need;
    need.lo = yt[0], need.hi = yt[0];
    for (int i = 0; i < H; ++i) {
        const int* e = &yt[4 * i];
        VT_REQUIRE(e[0] >= 0 && e[0] < Hs && e[1] >= 0 && e[1] < Hs, "vt_frame_scale_crop: ytab[%d] = (%d, %d) outside the frame (Hs %d)",
                   i, e[0], e[1], Hs);
        VT_REQUIRE(e[2] >= 0 && e[2] <= 2048 && e[3] >= 0 && e[3] <= 2048, "vt_frame_scale_crop: ytab[%d] weights (%d, %d) outside 0..2048",
                   i, e[2], e[3]);
        for (int j = 0; j < 2; ++j) need.lo = e[j] < need.lo ? e[j] : need.lo, need.hi = e[j] > need.hi ? e[j] : need.hi;
    }
    for (int p = 0; p < passes; ++p) need = fs_expand(need, Hs);
    VT_REQUIRE(need.lo >= row0 && need.hi < row0 + rows,
               "vt_frame_scale_crop: the crop and its blur halo read source rows [%d, %d], the slab holds [%d, %d)", need.lo,
               need.hi + 1, row0, row0 + rows);
    int tile = 0;
    for (int t : {32, 16, 8}) {
        const int fw = fs_max_extent(xt, W, t, passes, Ws), fh = fs_max_extent(yt, H, t, passes, Hs);
        if (fh * fs_pitch(fw) <= FS_LDS_A && (passes == 0 || 3 * fw * fh <= FS_LDS_T)) {
            tile = t;
            break;
        }
    }
    if (!tile) {
        vt_set_error("vt_frame_scale_crop: the source footprint of an 8 x 8 output tile does not fit %d bytes of LDS (scales "
                     "down to 1/8 are supported)", FS_LDS_A + 2 * FS_LDS_T);
        return VT_ERR_UNSUPPORTED;
    }
    auto k = frame_scale_crop_kernel;
    VT_LAUNCH(k, dim3(vt_cdiv(W, tile), vt_cdiv(H, tile), n), dim3(FS_THREADS), stream, (unsigned char*)out,
              (const unsigned char*)src, (int64_t)n * rows * Ws * 3, rows, row0, Hs, Ws, passes, (const int*)xtab,
              (const int*)ytab, H, W, tile);
    return vt_check_launch("vt_frame_scale_crop");
}
