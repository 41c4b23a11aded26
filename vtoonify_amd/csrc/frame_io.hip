// Frame packing / unpacking either side of VToonify.forward (gfx950) -- the per-frame host work of
// the reference's video loop moved onto the GPU:
//
//   vt_frame_pack    uint8 HWC frame (+ optional fp32 parsing map) -> the fp32 NCHW network input
//                      x[c] = ((u8 / 255) - 0.5) / 0.5                (transforms.ToTensor + Normalize,
//                                                                      style_transfer.py:57-60,160)
//                      x[3+j] = parsing[j] * parsing_scale            (x_p / 16., style_transfer.py:174)
//                    with the BGR->RGB swap of cv2.cvtColor (style_transfer.py:114) folded in.
//   vt_frame_unpack  fp32 NCHW image -> uint8 HWC frame
//                      u8 = (uint8)((clamp(y, -1, 1) + 1.0) * 127.5)  (torch.clamp style_transfer.py:177,
//                                                                      tensor2cv2 util.py:190-192)
//                    with the RGB->BGR swap of tensor2cv2 folded in.
//
//   vt_frame_ingest2x  uint8 HWC frames -> the three tensors of the flicker-reduction pre-pass at twice the frame size, in
//                    one read of the frame (smooth_parsing_map.py:86-89,128,136,154):
//                      Is      = F.upsample(Normalize(ToTensor(frame)), scale_factor=2, mode='bilinear')
//                      raft    = (Is + 1) * 255.0 / 2          RAFT's network input in [0, 255]
//                      bisenet = 2 * Is                        BiSeNet's network input
//                    all planar fp32 (n,3,2h,2w), the layout RaftEngine.encode / BiSeNetEngine.forward take.
//
// The first two are pure streaming kernels: 4 pixels per lane (12 payload bytes <-> three 16-byte plane
// vectors), every plane access a coalesced 16-byte vector.  The fp32 arithmetic is the reference's op
// sequence (div, sub, div / add, mul, truncate), unfused, so results are BIT-exact against the
// numpy / torch formulas (tests/test_video.py).
// vt_frame_ingest2x: one lane per output pixel; the four source pixels are 12 cached bytes, the nine stores of a wave are
// coalesced 256-byte rows.  Source index and lerp follow aten (area_pixel_compute_source_index with scale 0.5,
// align_corners=False; h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)), the two affine images are the reference's op
// sequences, unfused.
// Algorithmic bytes: pack  n*h*w*(3 + 4*(3+pc) + 4*pc);  unpack  n*H*W*(12 + 3);  ingest2x  n*h*w*(3 + 4*3*4*3).
#include "vt_common.hpp"

namespace {

__device__ __forceinline__ float norm_u8(unsigned v) { return ((float)v / 255.0f - 0.5f) / 0.5f; }

__device__ __forceinline__ unsigned quant_u8(float y) {
    y = fminf(fmaxf(y, -1.0f), 1.0f);
    return (unsigned)(int)((y + 1.0f) * 127.5f);   // truncation, as ndarray.astype(np.uint8)
}

// one thread = 4 consecutive pixels of one image (hw % 4 == 0) or 1 pixel (G = 1)
template <int G>
__global__ void __launch_bounds__(256)
frame_pack_kernel(float* __restrict__ x, const unsigned char* __restrict__ frames,
                  const float* __restrict__ parsing, int n, int hw, int pc, float pscale, int swap_rb) {
    const int groups = hw / G;
    const int64_t total = (int64_t)n * groups;
    const int ct = 3 + pc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int img = (int)(i / groups);
        const int p0 = (int)(i - (int64_t)img * groups) * G;
        const unsigned char* src = frames + ((int64_t)img * hw + p0) * 3;
        float* dst = x + (int64_t)img * ct * hw + p0;
        unsigned char b[3 * G];
        if (G == 4) {
            const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);   // 12-byte aligned group
            const uint32_t w0 = s32[0], w1 = s32[1], w2 = s32[2];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b[k] = (w0 >> (8 * k)) & 255;
                b[4 + k] = (w1 >> (8 * k)) & 255;
                b[8 + k] = (w2 >> (8 * k)) & 255;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * G; ++k) b[k] = src[k];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sc = swap_rb ? 2 - ch : ch;
            float v[G];
#pragma unroll
            for (int k = 0; k < G; ++k) v[k] = norm_u8(b[3 * k + sc]);
            if (G == 4) {
                st128(dst + (int64_t)ch * hw, pack16<float>(v));
            } else {
                dst[(int64_t)ch * hw] = v[0];
            }
        }
        for (int j = 0; j < pc; ++j) {
            const float* ps = parsing + ((int64_t)img * pc + j) * hw + p0;
            float* pd = dst + (int64_t)(3 + j) * hw;
            if (G == 4) {
                float q[4];
                unpack16<float>(ld128(ps), q);
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] *= pscale;
                st128(pd, pack16<float>(q));
            } else {
                pd[0] = ps[0] * pscale;
            }
        }
    }
}

template <int G>
__global__ void __launch_bounds__(256)
frame_unpack_kernel(unsigned char* __restrict__ frames, const float* __restrict__ image, int n, int hw,
                    int swap_rb) {
    const int groups = hw / G;
    const int64_t total = (int64_t)n * groups;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int img = (int)(i / groups);
        const int p0 = (int)(i - (int64_t)img * groups) * G;
        const float* src = image + (int64_t)img * 3 * hw + p0;
        unsigned char* dst = frames + ((int64_t)img * hw + p0) * 3;
        unsigned b[3 * G];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int dc = swap_rb ? 2 - ch : ch;
            float v[G];
            if (G == 4) {
                unpack16<float>(ld128(src + (int64_t)ch * hw), v);
            } else {
                v[0] = src[(int64_t)ch * hw];
            }
#pragma unroll
            for (int k = 0; k < G; ++k) b[3 * k + dc] = quant_u8(v[k]);
        }
        if (G == 4) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
            d32[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            d32[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            d32[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 3 * G; ++k) dst[k] = (unsigned char)b[k];
        }
    }
}

// aten area_pixel_compute_source_index(scale = 0.5, align_corners = false) + guard_index_and_lambda
__device__ __forceinline__ void up2_tap(int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = 0.5f * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.0f) src = 0.0f;
    i0 = (int)src;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// one thread = one output pixel (Y, X) of one image, its three channels and three destinations
__global__ void __launch_bounds__(256)
frame_ingest2x_kernel(float* __restrict__ is, float* __restrict__ raft, float* __restrict__ bise,
                      const unsigned char* __restrict__ frames, int n, int h, int w, int swap_rb) {
    const int oh = 2 * h, ow = 2 * w;
    const int64_t ohw = (int64_t)oh * ow;
    const int64_t total = (int64_t)n * ohw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int img = (int)(i / ohw);
        const int64_t rem = i - (int64_t)img * ohw;
        const int Y = (int)(rem / ow), X = (int)(rem - (int64_t)Y * ow);
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        up2_tap(Y, h, y0, y1, ly0, ly1);
        up2_tap(X, w, x0, x1, lx0, lx1);
        const unsigned char* f = frames + (int64_t)img * h * w * 3;
        const unsigned char* p00 = f + ((int64_t)y0 * w + x0) * 3;
        const unsigned char* p01 = f + ((int64_t)y0 * w + x1) * 3;
        const unsigned char* p10 = f + ((int64_t)y1 * w + x0) * 3;
        const unsigned char* p11 = f + ((int64_t)y1 * w + x1) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sc = swap_rb ? 2 - ch : ch;
            const float v = ly0 * (lx0 * norm_u8(p00[sc]) + lx1 * norm_u8(p01[sc])) +
                            ly1 * (lx0 * norm_u8(p10[sc]) + lx1 * norm_u8(p11[sc]));
            const int64_t o = ((int64_t)img * 3 + ch) * ohw + rem;
            is[o] = v;
            if (raft) raft[o] = (v + 1.0f) * 255.0f / 2.0f;
            if (bise) bise[o] = 2.0f * v;
        }
    }
}

inline unsigned grid_for(int64_t total) {
    int64_t b = (total + 255) / 256;
    if (b > 65536) b = 65536;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" int vt_frame_pack(float* x, const uint8_t* frames, int swap_rb, const float* parsing, int parsing_channels,
                             float parsing_scale, int n, int h, int w, vt_stream stream) {
    VT_REQUIRE(x && frames, "vt_frame_pack: null tensor");
    VT_REQUIRE(n > 0 && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31), "vt_frame_pack: bad sizes");
    VT_REQUIRE(parsing_channels >= 0 && (parsing_channels == 0 || parsing), "vt_frame_pack: parsing map missing");
    const int hw = h * w;
    const bool vec = hw % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)frames % 4 == 0 &&
                     (parsing_channels == 0 || (uintptr_t)parsing % 16 == 0);
    if (vec) {
        auto k = frame_pack_kernel<4>;
        VT_LAUNCH(k, dim3(grid_for((int64_t)n * hw / 4)), dim3(256), stream, x, (const unsigned char*)frames, parsing,
                  n, hw, parsing_channels, parsing_scale, swap_rb);
    } else {
        auto k = frame_pack_kernel<1>;
        VT_LAUNCH(k, dim3(grid_for((int64_t)n * hw)), dim3(256), stream, x, (const unsigned char*)frames, parsing, n,
                  hw, parsing_channels, parsing_scale, swap_rb);
    }
    return vt_check_launch("vt_frame_pack");
}

extern "C" int vt_frame_unpack(uint8_t* frames, const float* image, int swap_rb, int n, int h, int w,
                               vt_stream stream) {
    VT_REQUIRE(frames && image, "vt_frame_unpack: null tensor");
    VT_REQUIRE(n > 0 && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31), "vt_frame_unpack: bad sizes");
    const int hw = h * w;
    const bool vec = hw % 4 == 0 && (uintptr_t)image % 16 == 0 && (uintptr_t)frames % 4 == 0;
    if (vec) {
        auto k = frame_unpack_kernel<4>;
        VT_LAUNCH(k, dim3(grid_for((int64_t)n * hw / 4)), dim3(256), stream, (unsigned char*)frames, image, n, hw, swap_rb);
    } else {
        auto k = frame_unpack_kernel<1>;
        VT_LAUNCH(k, dim3(grid_for((int64_t)n * hw)), dim3(256), stream, (unsigned char*)frames, image, n, hw, swap_rb);
    }
    return vt_check_launch("vt_frame_unpack");
}

extern "C" int vt_frame_ingest2x(float* is, float* raft_in, float* bisenet_in, const uint8_t* frames, int swap_rb, int n,
                                 int h, int w, vt_stream stream) {
    VT_REQUIRE(is && frames, "vt_frame_ingest2x: null tensor");
    VT_REQUIRE(n > 0 && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 28), "vt_frame_ingest2x: bad sizes");
    auto k = frame_ingest2x_kernel;
    VT_LAUNCH(k, dim3(grid_for((int64_t)n * h * w * 4)), dim3(256), stream, is, raft_in, bisenet_in,
              (const unsigned char*)frames, n, h, w, swap_rb);
    return vt_check_launch("vt_frame_ingest2x");
}
