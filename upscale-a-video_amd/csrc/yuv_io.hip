// K13 — frame I/O conversions of the CLI on gfx950, HBM-bound elementwise: the uint8 / fp32 frame <-> clip
// normalisations of the reference program, and planar Y'CbCr <-> the clip / frame tensors for the Y4M front end.
//
//   frames_to_clip_kernel / clip_to_u8_kernel          uav_frames_to_clip_f32, uav_clip_to_frames_u8
//   yuv_to_clip_kernel<MODE,C444>                      uav_yuv420_to_clip_f32, uav_yuv444_to_clip_f32
//   yuv_sited_to_clip_kernel<MODE>                     uav_yuv420_sited_to_clip_f32
//   clip_to_yuv_kernel<MODE,C444,D10,SITED>            uav_clip_to_yuv420_u8, uav_clip_window_to_yuv420_u8, uav_clip_window_to_yuv,
//                                                      uav_clip_to_yuv420_sited
#include <type_traits>
#include "uav_common.h"
#include "yuv_common.h"
#include "yuv_mode.h"

namespace {
// (T,C,H,W) frames in 0..255 (uint8, or the fp32 tensor `read_frame_from_videos` returns) -> (C,T,H,W) fp32 in [-1,1]:
// `(vframes / 255. - 0.5) * 2` then 'b t c h w -> b c t h w' (inference_upscale_a_video.py:180,186-187), same op order.
template <typename T>
__global__ __launch_bounds__(256) void frames_to_clip_kernel(const T* __restrict__ src, float* __restrict__ dst, int t_len, int c,
                                                             long long hw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int tc = blockIdx.y, t = tc / c, ch = tc - t * c;
    const float v = (float)src[(long long)tc * hw + i];
    dst[((long long)ch * t_len + t) * hw + i] = (v / 255.0f - 0.5f) * 2.0f;
}
// (T,C,H,W) fp32 in [-1,1] -> (T,H,W,C) uint8: `(output / 2 + 0.5).clamp(0, 1) * 255`, 't c h w -> t h w c', numpy
// `.astype(np.uint8)` = truncation (inference_upscale_a_video.py:357-359).  One thread per pixel, C <= 4 channels.
__global__ __launch_bounds__(256) void clip_to_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, int c,
                                                         long long hw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const int t = blockIdx.y;
    for (int ch = 0; ch < c; ++ch) {
        float v = src[((long long)t * c + ch) * hw + i] / 2.0f + 0.5f;
        v = fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f;
        dst[((long long)t * hw + i) * c + ch] = (unsigned char)(int)v;
    }
}
}  // namespace

extern "C" int uav_frames_to_clip_f32(const void* frames_tchw, int32_t src_is_u8, float* clip_cthw, int32_t t_len, int32_t c,
                                      int64_t hw, void* stream) {
    if (!frames_tchw || !clip_cthw) return UAV_EINVAL;
    if (t_len <= 0 || c <= 0 || hw <= 0 || (int64_t)t_len * c > 65535) return UAV_ESHAPE;
    const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)(t_len * c));
    if (src_is_u8)
        hipLaunchKernelGGL(frames_to_clip_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames_tchw,
                           clip_cthw, t_len, c, (long long)hw);
    else
        hipLaunchKernelGGL(frames_to_clip_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)frames_tchw, clip_cthw,
                           t_len, c, (long long)hw);
    return uav_launch_status();
}

extern "C" int uav_clip_to_frames_u8(const float* frames_tchw, void* frames_thwc_u8, int32_t t_len, int32_t c, int64_t hw,
                                     void* stream) {
    if (!frames_tchw || !frames_thwc_u8) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || c <= 0 || c > 4 || hw <= 0) return UAV_ESHAPE;
    hipLaunchKernelGGL(clip_to_u8_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)t_len), dim3(256), 0, (hipStream_t)stream,
                       frames_tchw, (unsigned char*)frames_thwc_u8, c, (long long)hw);
    return uav_launch_status();
}

// ---- planar Y'CbCr 4:2:0 / 4:4:4, 8- / 10-bit <-> the clip / frame tensors ------------------------------------------------------
// Colour conversion in 16.16 fixed point on int32 (the host derives the coefficients from (Kr, Kb, range); every result is
// defined bit for bit), fused with the normalisation of the two kernels above.  HBM-bound: a thread owns YUV_RUN pixels of
// two adjacent rows, i.e. whole chroma samples, moves fp32 as 16-byte vectors and the planes as words, and falls back to scalar
// accesses for the tail of a row.  MODE 2: W % 8 == 0 (no tail), a run's samples of a row are one word; MODE 1: W % 4 == 0 (fp32
// rows stay 16-byte aligned), the same as two words of half the width, a 4-pixel tail is scalar; MODE 0: any W, scalar throughout.
// The launchers pick the mode from W and the alignment of every address a thread forms (yuv_mode.h).  No LDS, no scratch.
namespace {
constexpr int YUV_RUN = 8;
struct YuvInv { int yo, iy, rcr, gcb, gcr, bcb; };                             // YuvFwd: yuv_common.h

// What a thread owns: pixels [x0, x0 + n) of the rows [y0, y0 + rows) of frame t; ry = y0 / 2 is its chroma row in 4:2:0.
struct YuvOwn { int t, ry, x0, y0, rows, n; };
UAV_DEVINL bool yuv_own(int h, int w, YuvOwn& o) {
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = (h + 1) / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return false;
    o.t = blockIdx.y; o.ry = (int)(i / nrx); o.x0 = (int)(i - (long long)o.ry * nrx) * YUV_RUN; o.y0 = o.ry * 2;
    o.rows = min(2, h - o.y0); o.n = min(YUV_RUN, w - o.x0);
    return true;
}

UAV_DEVINL int yuv_clamp255(int v) { return min(max(v, 0), 255); }
// uint8 value -> [-1,1], the expression of frames_to_clip_kernel
UAV_DEVINL float yuv_u8_to_clip(int v) { return ((float)v / 255.0f - 0.5f) * 2.0f; }
// ([-1,1] -> uint8 value, the expression of clip_to_u8_kernel: yuv_clip_to_u8 in yuv_common.h)
UAV_DEVINL void yuv_to_rgb(const YuvInv& k, int yy, int u, int v, float& r, float& g, float& b) {
    const int y = (yy - k.yo) * k.iy;
    u -= 128; v -= 128;
    r = yuv_u8_to_clip(yuv_clamp255((y + k.rcr * v + 32768) >> 16));
    g = yuv_u8_to_clip(yuv_clamp255((y + k.gcb * u + k.gcr * v + 32768) >> 16));
    b = yuv_u8_to_clip(yuv_clamp255((y + k.bcb * u + 32768) >> 16));
}
UAV_DEVINL uint32_t yuv_byte(uint32_t w, int j) { return (w >> (8 * j)) & 255u; }

// ---- what the two decoders share: the loads of a whole run and the store of 4 converted pixels ---------------------------------
// 8 bytes of a row as two words: one 8-byte load (MODE 2) or two 4-byte loads
template <int MODE> UAV_DEVINL void yuv_load8(const unsigned char* p, uint32_t (&w)[2]) {
    if (MODE == 2) {
        const uint2_t v = *reinterpret_cast<const uint2_t*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
        w[1] = *reinterpret_cast<const uint32_t*>(p + 4);
    }
}
// the 4 chroma bytes of a 4:2:0 run as one word: one 4-byte load (MODE 2) or two 2-byte loads
template <int MODE> UAV_DEVINL uint32_t yuv_load4(const unsigned char* p) {
    if (MODE == 2) return *reinterpret_cast<const uint32_t*>(p);
    const unsigned short* a = reinterpret_cast<const unsigned short*>(p);
    return (uint32_t)a[0] | ((uint32_t)a[1] << 16);
}
// 4 pixels = one 16-byte store per channel, the channels `cs` elements apart
UAV_DEVINL void yuv_store_rgb4(float* o, long long cs, const float4_t& R, const float4_t& G, const float4_t& B) {
    *reinterpret_cast<float4_t*>(o) = R;
    *reinterpret_cast<float4_t*>(o + cs) = G;
    *reinterpret_cast<float4_t*>(o + 2 * cs) = B;
}

// planes Y (T,H,W), Cb / Cr (T,ch,cw) [ch = ceil(H/2), cw = ceil(W/2); C444: (T,H,W)] -> clip (3,T,H,W) fp32
template <int MODE, bool C444>
__global__ __launch_bounds__(256) void yuv_to_clip_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ cbp,
                                                          const unsigned char* __restrict__ crp, float* __restrict__ dst, int t_len,
                                                          int h, int w, YuvInv k) {
    YuvOwn own;
    if (!yuv_own(h, w, own)) return;
    const int ch = C444 ? h : (h + 1) / 2, cw = C444 ? w : (w + 1) / 2;
    const long long hw = (long long)h * w;
    const unsigned char* ysrc = yp + ((long long)own.t * h + own.y0) * w + own.x0;
    float* out = dst + ((long long)own.t * h + own.y0) * w + own.x0;           // channel stride: t_len * hw
    const long long cs = (long long)t_len * hw;
    if (MODE > 0 && own.n == YUV_RUN) {
        uint32_t cbw[2], crw[2];                                                // 4:2:0: word 0 only (4 samples, shared by both rows)
        if (!C444) {
            const long long co = ((long long)own.t * ch + own.ry) * cw + (own.x0 >> 1);
            cbw[0] = yuv_load4<MODE>(cbp + co);
            crw[0] = yuv_load4<MODE>(crp + co);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= own.rows) break;
            uint32_t yw[2];
            yuv_load8<MODE>(ysrc + (long long)r * w, yw);
            if (C444) {                                                         // the chroma bases are 4-byte aligned in both modes
                const long long co = ((long long)own.t * h + own.y0 + r) * w + own.x0;
                yuv_load8<1>(cbp + co, cbw);
                yuv_load8<1>(crp + co, crw);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float4_t R, G, B;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = q * 4 + j;
                    const int u = (int)(C444 ? yuv_byte(cbw[q], j) : yuv_byte(cbw[0], px >> 1));
                    const int v = (int)(C444 ? yuv_byte(crw[q], j) : yuv_byte(crw[0], px >> 1));
                    float fr, fg, fb;
                    yuv_to_rgb(k, (int)yuv_byte(yw[q], j), u, v, fr, fg, fb);
                    R[j] = fr; G[j] = fg; B[j] = fb;
                }
                yuv_store_rgb4(out + (long long)r * w + q * 4, cs, R, G, B);
            }
        }
        return;
    }
    for (int r = 0; r < own.rows; ++r)
        for (int j = 0; j < own.n; ++j) {
            const long long co = C444 ? ((long long)own.t * h + own.y0 + r) * w + own.x0 + j : ((long long)own.t * ch + own.ry) * cw + ((own.x0 + j) >> 1);
            float fr, fg, fb;
            yuv_to_rgb(k, ysrc[(long long)r * w + j], cbp[co], crp[co], fr, fg, fb);
            float* o = out + (long long)r * w + j;
            o[0] = fr; o[cs] = fg; o[2 * cs] = fb;
        }
}

// ---- siting-aware 4:2:0 decode (uav_yuv420_sited_to_clip_f32): `--chroma sited` of the front end ------------------------------
// Bilinear chroma up-sampling at the siting of the input's tag instead of replication.  Per axis a luma sample takes two
// chroma taps with weights in quarters — centre: (1,3) on c[i-1], c[i] for an even index, (3,1) on c[i], c[i+1] for an odd one;
// co-sited: (0,4) and (2,2) — indices clamped to the plane; the axes multiply (sixteenths) and the colour conversion rounds once.
struct YuvSiting { int he0, he1, ho0, ho1, ve0, ve1, vo0, vo1; };              // horizontal / vertical, even / odd index, tap 0 / 1

UAV_DEVINL void yuv_to_rgb16(const YuvInv& k, int yy, int u16, int v16, float& r, float& g, float& b) {
    const int y = (yy - k.yo) * k.iy * 16;
    r = yuv_u8_to_clip(yuv_clamp255((y + k.rcr * v16 + (1 << 19)) >> 20));
    g = yuv_u8_to_clip(yuv_clamp255((y + k.gcb * u16 + k.gcr * v16 + (1 << 19)) >> 20));
    b = yuv_u8_to_clip(yuv_clamp255((y + k.bcb * u16 + (1 << 19)) >> 20));
}

// planes Y (T,H,W), Cb / Cr (T,ch,cw) [ch = ceil(H/2), cw = ceil(W/2)] -> clip (3,T,H,W) fp32.  Ownership and MODEs of
// yuv_to_clip_kernel; a thread reads, beside its chroma word, the sample on either side of it in the rows ry-1, ry, ry+1
// (6 samples x 3 rows per plane, clamped at the borders): re-reads of what its neighbours own.
template <int MODE>
__global__ __launch_bounds__(256) void yuv_sited_to_clip_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ cbp,
                                                                const unsigned char* __restrict__ crp, float* __restrict__ dst, int t_len,
                                                                int h, int w, YuvInv k, YuvSiting s) {
    YuvOwn own;
    if (!yuv_own(h, w, own)) return;
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const long long hw = (long long)h * w;
    const unsigned char* ysrc = yp + ((long long)own.t * h + own.y0) * w + own.x0;
    float* out = dst + ((long long)own.t * h + own.y0) * w + own.x0;           // channel stride: t_len * hw
    const long long cs = (long long)t_len * hw;
    const long long crow[3] = {((long long)own.t * ch + max(own.ry - 1, 0)) * cw, ((long long)own.t * ch + own.ry) * cw,
                               ((long long)own.t * ch + min(own.ry + 1, ch - 1)) * cw};
    if (MODE > 0 && own.n == YUV_RUN) {
        const int i0 = own.x0 >> 1, il = max(i0 - 1, 0), ir = min(i0 + 4, cw - 1);  // i0 + 3 <= cw - 1: the run is whole
        int cbs[3][6], crs[3][6];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned char* pb = cbp + crow[a];
            const unsigned char* pr = crp + crow[a];
            const uint32_t bw = yuv_load4<MODE>(pb + i0), rw = yuv_load4<MODE>(pr + i0);
            cbs[a][0] = pb[il]; crs[a][0] = pr[il];
#pragma unroll
            for (int j = 0; j < 4; ++j) { cbs[a][1 + j] = (int)yuv_byte(bw, j); crs[a][1 + j] = (int)yuv_byte(rw, j); }
            cbs[a][5] = pb[ir]; crs[a][5] = pr[ir];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= own.rows) break;
            uint32_t yw[2];
            yuv_load8<MODE>(ysrc + (long long)r * w, yw);
            const int wa = r ? s.vo0 : s.ve0, wb = r ? s.vo1 : s.ve1;           // rows (ry-1, ry) for the even row, (ry, ry+1) for the odd one
            int ub[6], vb[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) { ub[c] = wa * cbs[r][c] + wb * cbs[r + 1][c]; vb[c] = wa * crs[r][c] + wb * crs[r + 1][c]; }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float4_t R, G, B;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = q * 4 + j, c = (px >> 1) + 1;                // samples (c-1, c) for an even pixel, (c, c+1) for an odd one
                    const int u16 = ((px & 1) ? s.ho0 * ub[c] + s.ho1 * ub[c + 1] : s.he0 * ub[c - 1] + s.he1 * ub[c]) - 2048;
                    const int v16 = ((px & 1) ? s.ho0 * vb[c] + s.ho1 * vb[c + 1] : s.he0 * vb[c - 1] + s.he1 * vb[c]) - 2048;
                    float fr, fg, fb;
                    yuv_to_rgb16(k, (int)yuv_byte(yw[q], j), u16, v16, fr, fg, fb);
                    R[j] = fr; G[j] = fg; B[j] = fb;
                }
                yuv_store_rgb4(out + (long long)r * w + q * 4, cs, R, G, B);
            }
        }
        return;
    }
    for (int r = 0; r < own.rows; ++r) {
        const long long ra = r ? crow[1] : crow[0], rb = r ? crow[2] : crow[1];
        const int wa = r ? s.vo0 : s.ve0, wb = r ? s.vo1 : s.ve1;
        for (int j = 0; j < own.n; ++j) {
            const int x = own.x0 + j, ci = x >> 1;
            const int ia = (x & 1) ? ci : max(ci - 1, 0), ib = (x & 1) ? min(ci + 1, cw - 1) : ci;
            const int w0 = (x & 1) ? s.ho0 : s.he0, w1 = (x & 1) ? s.ho1 : s.he1;
            const int u16 = wa * (w0 * cbp[ra + ia] + w1 * cbp[ra + ib]) + wb * (w0 * cbp[rb + ia] + w1 * cbp[rb + ib]) - 2048;
            const int v16 = wa * (w0 * crp[ra + ia] + w1 * crp[ra + ib]) + wb * (w0 * crp[rb + ia] + w1 * crp[rb + ib]) - 2048;
            float fr, fg, fb;
            yuv_to_rgb16(k, ysrc[(long long)r * w + j], u16, v16, fr, fg, fb);
            float* o = out + (long long)r * w + j;
            o[0] = fr; o[cs] = fg; o[2 * cs] = fb;
        }
    }
}

// ---- encode: every output format and both chroma sitings in one kernel -----------------------------------------------------------
// D10: 16-bit samples 0..1023 made from 12-bit RGB with no 8-bit intermediate, chroma centre 512; else uint8 samples from the
// uint8 RGB value of clip_to_u8_kernel, chroma centre 128.  C444: a chroma sample per pixel (one rounding each) instead of one
// per 2x2 block (the four products summed before the one rounding).  SITED (4:2:0 only): horizontally co-sited and vertically
// centred chroma, the siting of `C420mpeg2` and `C420p10` — a sample is made from the (1,2,1) filter around its EVEN luma
// column in both rows of its block, weights totalling 8, one rounding; a thread reads one more column, x0 - 1 (clamped to the
// window), per row and channel.  YuvDepth, yuv_clampd and yuv_luma_d are shared with the scene statistics: yuv_common.h.

// [-1,1] -> 12-bit value: the clamp of clip_to_u8_kernel, rounded to 0..4095
UAV_DEVINL int yuv_clip_to_q12(float x) {
#pragma clang fp contract(off)          // the product is rounded before the sum: a fused multiply-add would move some values by one
    float v = x / 2.0f + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (int)(v * 4095.0f + 0.5f);
}
template <bool D10> UAV_DEVINL int yuv_quant(float x) { return D10 ? yuv_clip_to_q12(x) : yuv_clip_to_u8(x); }
// a chroma sample from R, G, B weights totalling 2^(SHIFT - 16): of one pixel (yuv_chroma1), of the sums of a 2x2 block
// (yuv_chroma4), of the sited filter's sums (yuv_chroma8)
template <bool D10, int SHIFT> UAV_DEVINL int yuv_chroma_n(const int* f, int r, int g, int b) {
    return yuv_clampd<D10>(((f[0] * r + f[1] * g + f[2] * b + (1 << (SHIFT - 1))) >> SHIFT) + YuvDepth<D10>::centre);
}
template <bool D10> UAV_DEVINL int yuv_chroma1(const int* f, int r, int g, int b) { return yuv_chroma_n<D10, 16>(f, r, g, b); }
template <bool D10> UAV_DEVINL int yuv_chroma4(const int* f, int r, int g, int b) { return yuv_chroma_n<D10, 18>(f, r, g, b); }
template <bool D10> UAV_DEVINL int yuv_chroma8(const int* f, int r, int g, int b) { return yuv_chroma_n<D10, 19>(f, r, g, b); }
// sample j of a run, packed little-endian into 32-bit words
template <int BYTES> UAV_DEVINL void yuv_pack(uint32_t* words, int j, int v) {
    if (BYTES == 1) words[j >> 2] |= (uint32_t)v << (8 * (j & 3));
    else words[j >> 1] |= (uint32_t)v << (16 * (j & 1));
}
template <int BYTES> UAV_DEVINL void yuv_store(void* p, const uint32_t* w) {
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "one 4-, 8- or 16-byte store");
    if constexpr (BYTES == 16) { uint4_t v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3]; *reinterpret_cast<uint4_t*>(p) = v; }
    else if constexpr (BYTES == 8) { uint2_t v; v.x = w[0]; v.y = w[1]; *reinterpret_cast<uint2_t*>(p) = v; }
    else *reinterpret_cast<uint32_t*>(p) = w[0];
}
// BYTES of packed samples as one store (MODE 2) or as two halves (MODE 1); the halves of 4 bytes are the halves of one word
template <int MODE, int BYTES> UAV_DEVINL void yuv_store_run(void* p, const uint32_t* w) {
    if constexpr (MODE == 2) yuv_store<BYTES>(p, w);
    else if constexpr (BYTES == 4) {
        unsigned short* a = reinterpret_cast<unsigned short*>(p);
        a[0] = (unsigned short)w[0]; a[1] = (unsigned short)(w[0] >> 16);
    } else {
        yuv_store<BYTES / 2>(p, w);
        yuv_store<BYTES / 2>(reinterpret_cast<unsigned char*>(p) + BYTES / 2, w + BYTES / 8);
    }
}

// A window of h x w pixels of t_len frames inside larger tensors: the source is addressed by element strides of channel / frame /
// row (pixel stride 1: a crop of the decoder's (C,T,H,W) output, or of (T,C,H,W) frames), every plane by its row pitch and frame
// stride in SAMPLES, all pointers at the window's first sample.  Contiguous frames and planes are the window that is the whole.
struct YuvWindow { long long sc, st, sr, yp, yf, cp, cf; };

// 4:2:0 takes even h and w; 4:4:4 any h, w >= 1: a thread's run may have one row and an odd length.  A run's samples of a row
// are one store in MODE 2 (8 x 8-bit: 8 B, 8 x 16-bit: 16 B, 4 chroma x 8-bit: 4 B, x 16-bit: 8 B), two of half the width in MODE 1.
template <int MODE, bool C444, bool D10, bool SITED>
__global__ __launch_bounds__(256) void clip_to_yuv_kernel(const float* __restrict__ src, void* __restrict__ yv, void* __restrict__ cbv,
                                                          void* __restrict__ crv, int h, int w, YuvWindow g, YuvFwd k) {
    static_assert(!(SITED && C444), "siting is a property of sub-sampled chroma");
    typedef typename YuvDepth<D10>::sample S;
    constexpr int SB = (int)sizeof(S);
    YuvOwn own;
    if (!yuv_own(h, w, own)) return;
    const int x0 = own.x0, n = own.n, rows = C444 ? own.rows : 2;               // 4:2:0: two rows and n even
    const float* in = src + own.t * g.st + own.y0 * g.sr + x0;
    S* yd = reinterpret_cast<S*>(yv) + own.t * g.yf + own.y0 * g.yp + x0;
    const long long co = C444 ? own.t * g.cf + own.y0 * g.cp + x0 : own.t * g.cf + own.ry * g.cp + (x0 >> 1);
    S* cbd = reinterpret_cast<S*>(cbv) + co;
    S* crd = reinterpret_cast<S*>(crv) + co;
    if (MODE > 0 && n == YUV_RUN) {
        constexpr int NW = YUV_RUN * SB / 4;                                    // 32-bit words of a run's samples of one row
        int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) break;
            uint32_t yw[NW], bw[NW], rw[NW];
#pragma unroll
            for (int q = 0; q < NW; ++q) yw[q] = bw[q] = rw[q] = 0;
            const float* p0 = in + r * g.sr;
            int pr = 0, pg = 0, pb = 0;                                         // SITED: the pixel to the left
            if (SITED) {
                const int back = x0 > 0 ? 1 : 0;
                pr = yuv_quant<D10>(p0[-back]); pg = yuv_quant<D10>(p0[g.sc - back]); pb = yuv_quant<D10>(p0[2 * g.sc - back]);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* p = p0 + q * 4;
                const float4_t R = *reinterpret_cast<const float4_t*>(p);
                const float4_t G = *reinterpret_cast<const float4_t*>(p + g.sc);
                const float4_t B = *reinterpret_cast<const float4_t*>(p + 2 * g.sc);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = q * 4 + j;
                    const int ir = yuv_quant<D10>(R[j]), ig = yuv_quant<D10>(G[j]), ib = yuv_quant<D10>(B[j]);
                    yuv_pack<SB>(yw, px, yuv_luma_d<D10>(k, ir, ig, ib));
                    if (C444) {
                        yuv_pack<SB>(bw, px, yuv_chroma1<D10>(k.fcb, ir, ig, ib));
                        yuv_pack<SB>(rw, px, yuv_chroma1<D10>(k.fcr, ir, ig, ib));
                    } else if (SITED && !(px & 1)) {
                        sr[px >> 1] += pr + 2 * ir; sg[px >> 1] += pg + 2 * ig; sb[px >> 1] += pb + 2 * ib;
                    } else {
                        sr[px >> 1] += ir; sg[px >> 1] += ig; sb[px >> 1] += ib;
                    }
                    if (SITED) { pr = ir; pg = ig; pb = ib; }
                }
            }
            yuv_store_run<MODE, YUV_RUN * SB>(yd + r * g.yp, yw);
            if (C444) {
                yuv_store_run<MODE, YUV_RUN * SB>(cbd + r * g.cp, bw);
                yuv_store_run<MODE, YUV_RUN * SB>(crd + r * g.cp, rw);
            }
        }
        if constexpr (!C444) {
            uint32_t bw[2] = {0, 0}, rw[2] = {0, 0};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                yuv_pack<SB>(bw, c, SITED ? yuv_chroma8<D10>(k.fcb, sr[c], sg[c], sb[c]) : yuv_chroma4<D10>(k.fcb, sr[c], sg[c], sb[c]));
                yuv_pack<SB>(rw, c, SITED ? yuv_chroma8<D10>(k.fcr, sr[c], sg[c], sb[c]) : yuv_chroma4<D10>(k.fcr, sr[c], sg[c], sb[c]));
            }
            yuv_store_run<MODE, 4 * SB>(cbd, bw);
            yuv_store_run<MODE, 4 * SB>(crd, rw);
        }
        return;
    }
    if (C444) {
        for (int r = 0; r < rows; ++r)
            for (int j = 0; j < n; ++j) {
                const float* p = in + r * g.sr + j;
                const int ir = yuv_quant<D10>(p[0]), ig = yuv_quant<D10>(p[g.sc]), ib = yuv_quant<D10>(p[2 * g.sc]);
                yd[r * g.yp + j] = (S)yuv_luma_d<D10>(k, ir, ig, ib);
                cbd[r * g.cp + j] = (S)yuv_chroma1<D10>(k.fcb, ir, ig, ib);
                crd[r * g.cp + j] = (S)yuv_chroma1<D10>(k.fcr, ir, ig, ib);
            }
    } else {
        for (int c = 0; c < n / 2; ++c) {                                       // one chroma sample and its 2x2 luma block at a time
            const int back = x0 + c * 2 > 0 ? 1 : 0;
            int s_r = 0, s_g = 0, s_b = 0;
            for (int r = 0; r < 2; ++r) {
                const float* p = in + r * g.sr + c * 2;
                if (SITED) {
                    s_r += yuv_quant<D10>(p[-back]); s_g += yuv_quant<D10>(p[g.sc - back]); s_b += yuv_quant<D10>(p[2 * g.sc - back]);
                }
                for (int j = 0; j < 2; ++j) {
                    const int ir = yuv_quant<D10>(p[j]), ig = yuv_quant<D10>(p[g.sc + j]), ib = yuv_quant<D10>(p[2 * g.sc + j]);
                    yd[r * g.yp + c * 2 + j] = (S)yuv_luma_d<D10>(k, ir, ig, ib);
                    const int wt = SITED && j == 0 ? 2 : 1;
                    s_r += wt * ir; s_g += wt * ig; s_b += wt * ib;
                }
            }
            cbd[c] = (S)(SITED ? yuv_chroma8<D10>(k.fcb, s_r, s_g, s_b) : yuv_chroma4<D10>(k.fcb, s_r, s_g, s_b));
            crd[c] = (S)(SITED ? yuv_chroma8<D10>(k.fcr, s_r, s_g, s_b) : yuv_chroma4<D10>(k.fcr, s_r, s_g, s_b));
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline YuvInv yuv_inv(const int32_t* c) { return {c[0], c[1], c[2], c[3], c[4], c[5]}; }
inline uintptr_t yuv_addr(const void* p) { return (uintptr_t)p; }

// one thread per YUV_RUN x 2 pixels of a frame, the frames along y; false: more blocks than a grid dimension holds
inline bool yuv_grid(int t_len, int h, int w, dim3& grid) {
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * ((h + 1) / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return false;
    grid = dim3((unsigned)blocks, (unsigned)t_len);
    return true;
}
// f(std::integral_constant<int, mode>): the runtime mode as a template argument
template <typename F> void yuv_with_mode(int mode, F&& f) {
    switch (mode) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    default: f(std::integral_constant<int, 0>());
    }
}

template <bool C444>
int yuv_to_clip_launch(const void* y, const void* cb, const void* cr, float* clip, int32_t t_len, int32_t h, int32_t w,
                       const int32_t* coefs, void* stream) {
    if (!y || !cb || !cr || !clip || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0) return UAV_ESHAPE;
    dim3 grid;
    if (!yuv_grid(t_len, h, w, grid)) return UAV_ESHAPE;
    const YuvInv k = yuv_inv(coefs);
    const unsigned char *yp = (const unsigned char*)y, *cbp = (const unsigned char*)cb, *crp = (const unsigned char*)cr;
    yuv_with_mode(yuv_decode_mode(w, yuv_addr(clip), yuv_addr(y), yuv_addr(cb), yuv_addr(cr), C444), [&](auto m) {
        hipLaunchKernelGGL((yuv_to_clip_kernel<decltype(m)::value, C444>), grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip,
                           t_len, h, w, k);
    });
    return uav_launch_status();
}

// The instance of the encode kernel for a format: 4 unsited and 2 sited ones per mode, and no others are built.
typedef void (*YuvEncodeKernel)(const float*, void*, void*, void*, int, int, YuvWindow, YuvFwd);
template <int MODE, bool SITED> YuvEncodeKernel clip_to_yuv_instance(bool c444, bool d10) {
    if constexpr (SITED) return d10 ? clip_to_yuv_kernel<MODE, false, true, true> : clip_to_yuv_kernel<MODE, false, false, true>;
    else if (c444) return d10 ? clip_to_yuv_kernel<MODE, true, true, false> : clip_to_yuv_kernel<MODE, true, false, false>;
    else return d10 ? clip_to_yuv_kernel<MODE, false, true, false> : clip_to_yuv_kernel<MODE, false, false, false>;
}
// Every encoder's launch, after its entry point has checked the arguments: h x w pixels of t_len frames in the geometry `g`.
template <bool SITED>
int clip_to_yuv_launch(const float* src, void* y, void* cb, void* cr, int t_len, int h, int w, const YuvWindow& g, bool c444, int depth,
                       const int32_t* coefs, void* stream) {
    dim3 grid;
    if (!yuv_grid(t_len, h, w, grid)) return UAV_ESHAPE;
    const YuvFwd k = yuv_fwd(coefs);
    const bool d10 = depth == 10;
    const int mode = yuv_encode_mode(w, yuv_addr(src), yuv_addr(y), yuv_addr(cb), yuv_addr(cr), g.sc, g.st, g.sr, g.yp, g.yf, g.cp, g.cf,
                                     d10 ? 2 : 1, c444);
    yuv_with_mode(mode, [&](auto m) {
        const YuvEncodeKernel kernel = clip_to_yuv_instance<decltype(m)::value, SITED>(c444, d10);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, src, y, cb, cr, h, w, g, k);
    });
    return uav_launch_status();
}
// contiguous (T,3,H,W) frames and 4:2:0 planes Y (T,H,W), Cb / Cr (T,H/2,W/2) as a window
inline YuvWindow yuv_contiguous420(int h, int w) {
    const long long hw = (long long)h * w;
    return {hw, 3 * hw, w, w, hw, w / 2, hw / 4};
}
}  // namespace

extern "C" int uav_yuv420_to_clip_f32(const void* y, const void* cb, const void* cr, float* clip_cthw, int32_t t_len, int32_t h,
                                      int32_t w, const int32_t* coefs, void* stream) {
    return yuv_to_clip_launch<false>(y, cb, cr, clip_cthw, t_len, h, w, coefs, stream);
}

extern "C" int uav_yuv444_to_clip_f32(const void* y, const void* cb, const void* cr, float* clip_cthw, int32_t t_len, int32_t h,
                                      int32_t w, const int32_t* coefs, void* stream) {
    return yuv_to_clip_launch<true>(y, cb, cr, clip_cthw, t_len, h, w, coefs, stream);
}

extern "C" int uav_yuv420_sited_to_clip_f32(const void* y, const void* cb, const void* cr, float* clip_cthw, int32_t t_len, int32_t h,
                                            int32_t w, int32_t centre_h, int32_t centre_v, const int32_t* coefs, void* stream) {
    if (!y || !cb || !cr || !clip_cthw || !coefs) return UAV_EINVAL;
    if ((centre_h != 0 && centre_h != 1) || (centre_v != 0 && centre_v != 1)) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0) return UAV_ESHAPE;
    dim3 grid;
    if (!yuv_grid(t_len, h, w, grid)) return UAV_ESHAPE;
    const YuvInv k = yuv_inv(coefs);
    YuvSiting s;
    s.he0 = centre_h ? 1 : 0; s.he1 = centre_h ? 3 : 4; s.ho0 = centre_h ? 3 : 2; s.ho1 = centre_h ? 1 : 2;
    s.ve0 = centre_v ? 1 : 0; s.ve1 = centre_v ? 3 : 4; s.vo0 = centre_v ? 3 : 2; s.vo1 = centre_v ? 1 : 2;
    const unsigned char *yp = (const unsigned char*)y, *cbp = (const unsigned char*)cb, *crp = (const unsigned char*)cr;
    yuv_with_mode(yuv_decode_mode(w, yuv_addr(clip_cthw), yuv_addr(y), yuv_addr(cb), yuv_addr(cr), false), [&](auto m) {
        hipLaunchKernelGGL(yuv_sited_to_clip_kernel<decltype(m)::value>, grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip_cthw,
                           t_len, h, w, k, s);
    });
    return uav_launch_status();
}

extern "C" int uav_clip_to_yuv420_u8(const float* frames_tchw, void* y, void* cb, void* cr, int32_t t_len, int32_t h, int32_t w,
                                     const int32_t* coefs, void* stream) {
    if (!frames_tchw || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return UAV_ESHAPE;
    return clip_to_yuv_launch<false>(frames_tchw, y, cb, cr, t_len, h, w, yuv_contiguous420(h, w), false, 8, coefs, stream);
}

extern "C" int uav_clip_to_yuv420_sited(const float* frames_tchw, void* y, void* cb, void* cr, int32_t t_len, int32_t h, int32_t w,
                                        int32_t depth, const int32_t* coefs, void* stream) {
    if (!frames_tchw || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if (depth != 8 && depth != 10) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return UAV_ESHAPE;
    const uintptr_t sb = depth == 10 ? 2 : 1;                                   // bytes per sample
    if (!yuv_aligned(yuv_addr(y), sb) || !yuv_aligned(yuv_addr(cb), sb) || !yuv_aligned(yuv_addr(cr), sb)) return UAV_EALIGN;
    return clip_to_yuv_launch<true>(frames_tchw, y, cb, cr, t_len, h, w, yuv_contiguous420(h, w), false, depth, coefs, stream);
}

extern "C" int uav_clip_window_to_yuv(const float* src, int64_t src_c_stride, int64_t src_t_stride, int64_t src_row_stride, void* y,
                                      int64_t y_pitch, int64_t y_frame, void* cb, void* cr, int64_t c_pitch, int64_t c_frame,
                                      int32_t t_len, int32_t h, int32_t w, int32_t chroma444, int32_t depth, const int32_t* coefs,
                                      void* stream) {
    if (!src || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if ((depth != 8 && depth != 10) || (chroma444 != 0 && chroma444 != 1)) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (!chroma444 && ((h & 1) || (w & 1)))) return UAV_ESHAPE;
    const int ch = chroma444 ? h : h / 2, cw = chroma444 ? w : w / 2;
    // no negative strides, and the rows / frames of a plane must not overlap (two threads would own one sample)
    if (src_c_stride < 0 || src_t_stride < 0 || src_row_stride < 0 || y_pitch < w || c_pitch < cw) return UAV_ESHAPE;
    if (t_len > 1 && (y_frame < (int64_t)(h - 1) * y_pitch + w || c_frame < (int64_t)(ch - 1) * c_pitch + cw)) return UAV_ESHAPE;
    const uintptr_t sb = depth == 10 ? 2 : 1;                                   // bytes per sample
    if (!yuv_aligned(yuv_addr(y), sb) || !yuv_aligned(yuv_addr(cb), sb) || !yuv_aligned(yuv_addr(cr), sb)) return UAV_EALIGN;
    const YuvWindow g = {src_c_stride, src_t_stride, src_row_stride, y_pitch, y_frame, c_pitch, c_frame};
    return clip_to_yuv_launch<false>(src, y, cb, cr, t_len, h, w, g, chroma444 != 0, depth, coefs, stream);
}

extern "C" int uav_clip_window_to_yuv420_u8(const float* src, int64_t src_c_stride, int64_t src_t_stride, int64_t src_row_stride,
                                            void* y, int64_t y_pitch, int64_t y_frame, void* cb, void* cr, int64_t c_pitch,
                                            int64_t c_frame, int32_t t_len, int32_t h, int32_t w, const int32_t* coefs, void* stream) {
    return uav_clip_window_to_yuv(src, src_c_stride, src_t_stride, src_row_stride, y, y_pitch, y_frame, cb, cr, c_pitch, c_frame, t_len,
                                  h, w, 0, 8, coefs, stream);
}
