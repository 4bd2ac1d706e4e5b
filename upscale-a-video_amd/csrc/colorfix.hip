// K12 — colour-correction post-process of the CLI on the decoded frames (gfx950), fp32 planes (T*C, H, W).
//
// Replaces (reference models_video/color_correction.py, inference_upscale_a_video.py:322-333):
//   F.interpolate(vframes, scale_factor=4, mode='bicubic')          uav_resize_bicubic_f32
//   adaptive_instance_normalization (:59-71, calc_mean_std :43-57)   uav_plane_stats_f32 + uav_adain_apply_f32
//   wavelet_blur / wavelet_decomposition / _reconstruction (:73-118) uav_atrous_blur_f32 (+ uav_axpby_f32)
//
// All of it is HBM-bound elementwise / small-stencil work on 1280x1280 frames (20 MB per frame and channel triple):
// coalesced 4-B accesses along W, the stencil's 9 taps (dilation up to 16) come from L2.  Bounds: 8 B/pixel for the
// blur (read + write; +8 with the fused high-frequency accumulation), 4 B/pixel for the statistics pass, 8 B/pixel for
// the AdaIN apply, 4.25 B/pixel for the 4x bicubic resize.  Statistics are deterministic (two-stage, fp64 combine).
#include "uav_common.h"

namespace {

constexpr int CF_CHUNKS = 64;

__global__ __launch_bounds__(256) void plane_partial_kernel(const float* __restrict__ x, long long hw, double* __restrict__ ws) {
    __shared__ double rs[256], rq[256];
    const int plane = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long long per = (hw + CF_CHUNKS - 1) / CF_CHUNKS;
    const long long i0 = (long long)chunk * per;
    long long i1 = i0 + per; if (i1 > hw) i1 = hw;
    const float* p = x + (long long)plane * hw;
    double s = 0.0, q = 0.0;
    // fp64 sums of the values and of their squares (the square of an fp32 number is exact in fp64): the variance is
    // q - n m^2, which cancels all but var / mean^2 of q, so a square rounded to fp32 would cost a near-constant plane
    // most of its variance.  8 independent loads are in flight per thread.
    for (long long i = i0 + tid; i < i1; i += 256 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long j = i + (long long)u * 256;
            v[u] = j < i1 ? p[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const double d = (double)v[u]; s += d; q += d * d; }
    }
    rs[tid] = s; rq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { ws[((long long)plane * CF_CHUNKS + chunk) * 2] = rs[0]; ws[((long long)plane * CF_CHUNKS + chunk) * 2 + 1] = rq[0]; }
}

// mean and UNBIASED variance per plane (torch.var default, color_correction.py:54)
__global__ void plane_finalize_kernel(const double* __restrict__ ws, int planes, long long hw, float* __restrict__ mean,
                                      float* __restrict__ var) {
    const int plane = blockIdx.x * blockDim.x + threadIdx.x;
    if (plane >= planes) return;
    double s = 0.0, q = 0.0;
    for (int c = 0; c < CF_CHUNKS; ++c) { s += ws[((long long)plane * CF_CHUNKS + c) * 2]; q += ws[((long long)plane * CF_CHUNKS + c) * 2 + 1]; }
    const double n = (double)hw, m = s / n;
    double v = hw > 1 ? (q - n * m * m) / (n - 1.0) : 0.0;
    if (v < 0.0) v = 0.0;
    mean[plane] = (float)m; var[plane] = (float)v;
}

// out = (x - cm) / sqrt(cv + eps) * sqrt(sv + eps) + sm   (color_correction.py:69-71), 4 elements per thread
__global__ __launch_bounds__(256) void adain_apply_kernel(const float* __restrict__ x, float* __restrict__ out, long long hw,
                                                          const float* __restrict__ cm, const float* __restrict__ cv,
                                                          const float* __restrict__ sm, const float* __restrict__ sv, float eps) {
    const int plane = blockIdx.y;
    const float m = cm[plane], cs = sqrtf(cv[plane] + eps), ss = sqrtf(sv[plane] + eps), smn = sm[plane];
    const long long base = (long long)plane * hw;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 4 <= hw && !(base & 3)) {
        float4_t v = *(const float4_t*)(x + base + i), o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[j] - m) / cs * ss + smn;
        *(float4_t*)(out + base + i) = o;
    } else {
        for (long long j = i; j < hw && j < i + 4; ++j) out[base + j] = (x[base + j] - m) / cs * ss + smn;
    }
}

// 3x3 a-trous blur [1 2 1]^T [1 2 1] / 16 with dilation `r` on a replicate-padded image (wavelet_blur :73-91) and,
// optionally, the decomposition's running high-frequency sum high += image - low (:101-103).
__global__ __launch_bounds__(256) void atrous_blur_kernel(const float* __restrict__ src, float* __restrict__ low,
                                                          float* __restrict__ high, int h, int w, int r) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const long long base = (long long)blockIdx.z * h * w;
    const int xm = x - r < 0 ? 0 : x - r, xp = x + r > w - 1 ? w - 1 : x + r;
    const int ym = y - r < 0 ? 0 : y - r, yp = y + r > h - 1 ? h - 1 : y + r;
    const float* p = src + base;
    const float* r0 = p + (long long)ym * w; const float* r1 = p + (long long)y * w; const float* r2 = p + (long long)yp * w;
    const float c = r1[x];
    // same tap order as a 3x3 cross-correlation (row-major), weights exact in binary
    float a = 0.0625f * r0[xm];
    a += 0.125f * r0[x]; a += 0.0625f * r0[xp];
    a += 0.125f * r1[xm]; a += 0.25f * c; a += 0.125f * r1[xp];
    a += 0.0625f * r2[xm]; a += 0.125f * r2[x]; a += 0.0625f * r2[xp];
    const long long o = base + (long long)y * w + x;
    low[o] = a;
    if (high) high[o] += c - a;
}

// F.interpolate(mode='bicubic', align_corners=False) with an integer or fractional scale: ATen upsample_bicubic2d
// (cubic convolution, A = -0.75, source index scale*(dst+0.5)-0.5, clamped taps).
UAV_DEVINL float cc1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
UAV_DEVINL float cc2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
UAV_DEVINL void cubic_coeffs(float t, float (&c)[4]) {
    const float A = -0.75f;
    c[0] = cc2(t + 1.f, A); c[1] = cc1(t, A); c[2] = cc1(1.f - t, A); c[3] = cc2(2.f - t, A);
}

__global__ __launch_bounds__(256) void resize_bicubic_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi,
                                                             int ho, int wo, float sy, float sx) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= wo) return;
    const float* p = src + (long long)blockIdx.z * hi * wi;
    const float ry = sy * (y + 0.5f) - 0.5f, rx = sx * (x + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    float cy[4], cx[4];
    cubic_coeffs(ry - fy, cy); cubic_coeffs(rx - fx, cx);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int yy = iy - 1 + i; yy = yy < 0 ? 0 : (yy > hi - 1 ? hi - 1 : yy);
        const float* row = p + (long long)yy * wi;
        float rsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int xx = ix - 1 + j; xx = xx < 0 ? 0 : (xx > wi - 1 ? wi - 1 : xx);
            rsum += row[xx] * cx[j];
        }
        acc += rsum * cy[i];
    }
    dst[((long long)blockIdx.z * ho + y) * wo + x] = acc;
}

// F.interpolate(mode='area') = adaptive average pooling: window [floor(o*in/out), ceil((o+1)*in/out)) per axis; `mul`
// folds the flow rescale of Propagation.forward (propagation_module.py:206-209: flows * w / w_f).
__global__ __launch_bounds__(256) void resize_area_kernel(const float* __restrict__ src, float* __restrict__ dst, int hi, int wi,
                                                          int ho, int wo, float mul) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= wo) return;
    const float* p = src + (long long)blockIdx.z * hi * wi;
    const int y0 = (int)(((long long)y * hi) / ho), y1 = (int)((((long long)(y + 1)) * hi + ho - 1) / ho);
    const int x0 = (int)(((long long)x * wi) / wo), x1 = (int)((((long long)(x + 1)) * wi + wo - 1) / wo);
    float acc = 0.f;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) acc += p[(long long)yy * wi + xx];
    dst[((long long)blockIdx.z * ho + y) * wo + x] = acc / (float)((y1 - y0) * (x1 - x0)) * mul;
}

}  // namespace

extern "C" int uav_resize_area_f32(const float* src, float* dst, int32_t planes, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                                   float mul, void* stream) {
    if (!src || !dst) return UAV_EINVAL;
    if (planes <= 0 || planes > 65535 || hi <= 0 || wi <= 0 || ho <= 0 || ho > 65535 || wo <= 0) return UAV_ESHAPE;
    hipLaunchKernelGGL(resize_area_kernel, dim3((wo + 255) / 256, ho, planes), dim3(256), 0, (hipStream_t)stream, src, dst, hi, wi,
                       ho, wo, mul);
    return uav_launch_status();
}

// ---- K13: frame I/O conversions of the CLI, HBM-bound elementwise -----------------------------------
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

// ---- K13 (continued): planar Y'CbCr 4:2:0 / 4:4:4 uint8 <-> the clip / frame tensors, for the Y4M front end ---------------
// Colour conversion in 16.16 fixed point on int32 (the host derives the coefficients from (Kr, Kb, range); every result is
// defined bit for bit), fused with the normalisation of the two kernels above.  HBM-bound: a thread owns YUV_RUN pixels of
// two adjacent rows, i.e. whole chroma samples, moves fp32 as 16-byte vectors and the planes as 4- / 8-byte words, and
// falls back to scalar accesses for the tail of a row.  MODE 2: W % 8 == 0 (no tail); MODE 1: W % 4 == 0 (fp32 rows stay
// 16-byte aligned, planes are moved as 4-byte luma and 2-byte chroma words, a 4-pixel tail is scalar); MODE 0: any W,
// scalar throughout.  The launchers pick the mode from W and the pointers' alignment.  No LDS, no scratch.
namespace {
constexpr int YUV_RUN = 8;
struct YuvInv { int yo, iy, rcr, gcb, gcr, bcb; };
struct YuvFwd { int fy[3], fcb[3], fcr[3], yo; };

UAV_DEVINL int yuv_clamp255(int v) { return min(max(v, 0), 255); }
// uint8 value -> [-1,1], the expression of frames_to_clip_kernel
UAV_DEVINL float yuv_u8_to_clip(int v) { return ((float)v / 255.0f - 0.5f) * 2.0f; }
// [-1,1] -> uint8 value, the expression of clip_to_u8_kernel
UAV_DEVINL int yuv_clip_to_u8(float x) {
    float v = x / 2.0f + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f;
    return (int)v;
}
UAV_DEVINL void yuv_to_rgb(const YuvInv& k, int yy, int u, int v, float& r, float& g, float& b) {
    const int y = (yy - k.yo) * k.iy;
    u -= 128; v -= 128;
    r = yuv_u8_to_clip(yuv_clamp255((y + k.rcr * v + 32768) >> 16));
    g = yuv_u8_to_clip(yuv_clamp255((y + k.gcb * u + k.gcr * v + 32768) >> 16));
    b = yuv_u8_to_clip(yuv_clamp255((y + k.bcb * u + 32768) >> 16));
}
UAV_DEVINL int yuv_luma(const YuvFwd& k, int r, int g, int b) {
    return yuv_clamp255(((k.fy[0] * r + k.fy[1] * g + k.fy[2] * b + 32768) >> 16) + k.yo);
}
// one chroma sample from the R, G, B sums of its 2x2 block (the four products summed before the one rounding)
UAV_DEVINL int yuv_chroma(const int* f, int r, int g, int b) {
    return yuv_clamp255(((f[0] * r + f[1] * g + f[2] * b + (1 << 17)) >> 18) + 128);
}
UAV_DEVINL uint32_t yuv_byte(uint32_t w, int j) { return (w >> (8 * j)) & 255u; }

// planes Y (T,H,W), Cb / Cr (T,ch,cw) [ch = ceil(H/2), cw = ceil(W/2); C444: (T,H,W)] -> clip (3,T,H,W) fp32
template <int MODE, bool C444>
__global__ __launch_bounds__(256) void yuv_to_clip_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ cbp,
                                                          const unsigned char* __restrict__ crp, float* __restrict__ dst, int t_len,
                                                          int h, int w, YuvInv k) {
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = (h + 1) / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int rows = min(2, h - y0), n = min(YUV_RUN, w - x0);
    const int ch = C444 ? h : (h + 1) / 2, cw = C444 ? w : (w + 1) / 2;
    const long long hw = (long long)h * w;
    const unsigned char* ysrc = yp + ((long long)t * h + y0) * w + x0;
    float* out = dst + ((long long)t * h + y0) * w + x0;                       // channel stride: t_len * hw
    const long long cs = (long long)t_len * hw;
    if (MODE > 0 && n == YUV_RUN) {
        uint32_t cbw[2], crw[2];                                                // 4:2:0: word 0 only (4 samples, shared by both rows)
        if (!C444) {
            const long long co = ((long long)t * ch + ry) * cw + (x0 >> 1);
            if (MODE == 2) {
                cbw[0] = *reinterpret_cast<const uint32_t*>(cbp + co);
                crw[0] = *reinterpret_cast<const uint32_t*>(crp + co);
            } else {
                const unsigned short* a = reinterpret_cast<const unsigned short*>(cbp + co);
                const unsigned short* b = reinterpret_cast<const unsigned short*>(crp + co);
                cbw[0] = (uint32_t)a[0] | ((uint32_t)a[1] << 16);
                crw[0] = (uint32_t)b[0] | ((uint32_t)b[1] << 16);
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) break;
            uint32_t yw[2];
            if (MODE == 2) {
                const uint2_t v = *reinterpret_cast<const uint2_t*>(ysrc + (long long)r * w);
                yw[0] = v.x; yw[1] = v.y;
            } else {
                yw[0] = *reinterpret_cast<const uint32_t*>(ysrc + (long long)r * w);
                yw[1] = *reinterpret_cast<const uint32_t*>(ysrc + (long long)r * w + 4);
            }
            if (C444) {
                const long long co = ((long long)t * h + y0 + r) * w + x0;
                cbw[0] = *reinterpret_cast<const uint32_t*>(cbp + co); cbw[1] = *reinterpret_cast<const uint32_t*>(cbp + co + 4);
                crw[0] = *reinterpret_cast<const uint32_t*>(crp + co); crw[1] = *reinterpret_cast<const uint32_t*>(crp + co + 4);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {                                       // 4 pixels = one 16-byte store per channel
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
                float* o = out + (long long)r * w + q * 4;
                *reinterpret_cast<float4_t*>(o) = R;
                *reinterpret_cast<float4_t*>(o + cs) = G;
                *reinterpret_cast<float4_t*>(o + 2 * cs) = B;
            }
        }
        return;
    }
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < n; ++j) {
            const long long co = C444 ? ((long long)t * h + y0 + r) * w + x0 + j : ((long long)t * ch + ry) * cw + ((x0 + j) >> 1);
            float fr, fg, fb;
            yuv_to_rgb(k, ysrc[(long long)r * w + j], cbp[co], crp[co], fr, fg, fb);
            float* o = out + (long long)r * w + j;
            o[0] = fr; o[cs] = fg; o[2 * cs] = fb;
        }
}

// The work of one thread of the two kernels below: `n` (even, <= YUV_RUN) pixels of two adjacent rows of one frame -> their luma
// bytes and n/2 chroma samples.  `in`: the R value of the first pixel, G and B `cs` elements further each, the second row `rs`
// elements further; `yd`: the first luma byte, the second row `yp` bytes further; `cbd` / `crd`: the first chroma sample.
template <int MODE>
UAV_DEVINL void clip_to_yuv420_run(const float* __restrict__ in, long long cs, long long rs, unsigned char* __restrict__ yd, long long yp,
                                   unsigned char* __restrict__ cbd, unsigned char* __restrict__ crd, int n, const YuvFwd& k) {
    if (MODE > 0 && n == YUV_RUN) {
        int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t yw[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* p = in + r * rs + q * 4;
                const float4_t R = *reinterpret_cast<const float4_t*>(p);
                const float4_t G = *reinterpret_cast<const float4_t*>(p + cs);
                const float4_t B = *reinterpret_cast<const float4_t*>(p + 2 * cs);
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ir = yuv_clip_to_u8(R[j]), ig = yuv_clip_to_u8(G[j]), ib = yuv_clip_to_u8(B[j]);
                    word |= (uint32_t)yuv_luma(k, ir, ig, ib) << (8 * j);
                    sr[q * 2 + (j >> 1)] += ir; sg[q * 2 + (j >> 1)] += ig; sb[q * 2 + (j >> 1)] += ib;
                }
                yw[q] = word;
            }
            if (MODE == 2) {
                uint2_t v; v.x = yw[0]; v.y = yw[1];
                *reinterpret_cast<uint2_t*>(yd + r * yp) = v;
            } else {
                *reinterpret_cast<uint32_t*>(yd + r * yp) = yw[0];
                *reinterpret_cast<uint32_t*>(yd + r * yp + 4) = yw[1];
            }
        }
        uint32_t cbw = 0, crw = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            cbw |= (uint32_t)yuv_chroma(k.fcb, sr[c], sg[c], sb[c]) << (8 * c);
            crw |= (uint32_t)yuv_chroma(k.fcr, sr[c], sg[c], sb[c]) << (8 * c);
        }
        if (MODE == 2) {
            *reinterpret_cast<uint32_t*>(cbd) = cbw;
            *reinterpret_cast<uint32_t*>(crd) = crw;
        } else {
            unsigned short* a = reinterpret_cast<unsigned short*>(cbd);
            unsigned short* b = reinterpret_cast<unsigned short*>(crd);
            a[0] = (unsigned short)cbw; a[1] = (unsigned short)(cbw >> 16);
            b[0] = (unsigned short)crw; b[1] = (unsigned short)(crw >> 16);
        }
        return;
    }
    for (int c = 0; c < n / 2; ++c) {                                           // one 2x2 block at a time
        int r4 = 0, g4 = 0, b4 = 0;
        for (int r = 0; r < 2; ++r)
            for (int j = 0; j < 2; ++j) {
                const float* p = in + r * rs + c * 2 + j;
                const int ir = yuv_clip_to_u8(p[0]), ig = yuv_clip_to_u8(p[cs]), ib = yuv_clip_to_u8(p[2 * cs]);
                yd[r * yp + c * 2 + j] = (unsigned char)yuv_luma(k, ir, ig, ib);
                r4 += ir; g4 += ig; b4 += ib;
            }
        cbd[c] = (unsigned char)yuv_chroma(k.fcb, r4, g4, b4);
        crd[c] = (unsigned char)yuv_chroma(k.fcr, r4, g4, b4);
    }
}

// frames (T,3,H,W) fp32 in [-1,1], H and W even -> planes Y (T,H,W), Cb / Cr (T,H/2,W/2)
template <int MODE>
__global__ __launch_bounds__(256) void clip_to_yuv420_kernel(const float* __restrict__ src, unsigned char* __restrict__ yp,
                                                             unsigned char* __restrict__ cbp, unsigned char* __restrict__ crp, int h,
                                                             int w, YuvFwd k) {
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = h / 2, cw = w / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int n = min(YUV_RUN, w - x0);                                         // even
    const long long hw = (long long)h * w;
    const float* in = src + (long long)t * 3 * hw + (long long)y0 * w + x0;    // channel stride: hw
    unsigned char* yd = yp + (long long)t * hw + (long long)y0 * w + x0;
    const long long co = ((long long)t * nry + ry) * cw + (x0 >> 1);
    clip_to_yuv420_run<MODE>(in, hw, w, yd, w, cbp + co, crp + co, n, k);
}

// The same for a WINDOW of h x w pixels (both even) of t_len frames inside larger tensors: the source is addressed by element
// strides of channel / frame / row (pixel stride 1: a crop of the decoder's (C,T,H,W) output, or of (T,C,H,W) frames), every
// plane by its row pitch and frame stride in bytes, all pointers at the window's first sample.
struct YuvWindow { long long sc, st, sr, yp, yf, cp, cf; };
template <int MODE>
__global__ __launch_bounds__(256) void clip_window_to_yuv420_kernel(const float* __restrict__ src, unsigned char* __restrict__ yp,
                                                                    unsigned char* __restrict__ cbp, unsigned char* __restrict__ crp,
                                                                    int h, int w, YuvWindow g, YuvFwd k) {
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = h / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int n = min(YUV_RUN, w - x0);                                         // even
    const float* in = src + t * g.st + y0 * g.sr + x0;
    unsigned char* yd = yp + t * g.yf + y0 * g.yp + x0;
    const long long co = t * g.cf + ry * g.cp + (x0 >> 1);
    clip_to_yuv420_run<MODE>(in, g.sc, g.sr, yd, g.yp, cbp + co, crp + co, n, k);
}

// ---- the output formats beside 8-bit 4:2:0: 8-bit 4:4:4 and 10-bit 4:2:0 / 4:4:4 (uav_clip_window_to_yuv) -------------------
// D10: 16-bit samples 0..1023 made from 12-bit RGB with no 8-bit intermediate, chroma centre 512; else the uint8 RGB value and
// the luma of the kernels above, chroma centre 128.  C444: a chroma sample per pixel (one rounding each) instead of per 2x2 block.
template <bool D10> struct YuvDepth { typedef unsigned char sample; static constexpr int centre = 128, vmax = 255; };
template <> struct YuvDepth<true> { typedef unsigned short sample; static constexpr int centre = 512, vmax = 1023; };

// [-1,1] -> 12-bit value: the clamp of clip_to_u8_kernel, rounded to 0..4095
UAV_DEVINL int yuv_clip_to_q12(float x) {
#pragma clang fp contract(off)          // the product is rounded before the sum: a fused multiply-add would move some values by one
    float v = x / 2.0f + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (int)(v * 4095.0f + 0.5f);
}
template <bool D10> UAV_DEVINL int yuv_quant(float x) { return D10 ? yuv_clip_to_q12(x) : yuv_clip_to_u8(x); }
template <bool D10> UAV_DEVINL int yuv_clampd(int v) { return min(max(v, 0), YuvDepth<D10>::vmax); }
template <bool D10> UAV_DEVINL int yuv_luma_d(const YuvFwd& k, int r, int g, int b) {
    return yuv_clampd<D10>(((k.fy[0] * r + k.fy[1] * g + k.fy[2] * b + 32768) >> 16) + k.yo);
}
// a chroma sample of one pixel / of the R, G, B sums of a 2x2 block
template <bool D10> UAV_DEVINL int yuv_chroma1(const int* f, int r, int g, int b) {
    return yuv_clampd<D10>(((f[0] * r + f[1] * g + f[2] * b + 32768) >> 16) + YuvDepth<D10>::centre);
}
template <bool D10> UAV_DEVINL int yuv_chroma4(const int* f, int r, int g, int b) {
    return yuv_clampd<D10>(((f[0] * r + f[1] * g + f[2] * b + (1 << 17)) >> 18) + YuvDepth<D10>::centre);
}
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
// BYTES of packed samples as one store (MODE 2) or as two halves (MODE 1)
template <int MODE, int BYTES> UAV_DEVINL void yuv_store_run(void* p, const uint32_t* w) {
    if constexpr (MODE == 2) yuv_store<BYTES>(p, w);
    else {
        yuv_store<BYTES / 2>(p, w);
        yuv_store<BYTES / 2>(reinterpret_cast<unsigned char*>(p) + BYTES / 2, w + BYTES / 8);
    }
}

// A window of h x w pixels of t_len frames, as clip_window_to_yuv420_kernel, for the three formats above; YuvWindow's plane
// pitches and frame strides are in SAMPLES here.  4:4:4 takes any h, w >= 1: a thread's run may have one row and an odd length.
// MODE 2: w % 8 == 0, a run's samples of a row are one store (8 x 8-bit: 8 B, 8 x 16-bit: 16 B, 4 chroma x 16-bit: 8 B);
// MODE 1: w % 4 == 0, the same as two stores of half the width, a 4-pixel tail is scalar; MODE 0: scalar throughout.
template <int MODE, bool C444, bool D10>
__global__ __launch_bounds__(256) void clip_window_to_yuv_kernel(const float* __restrict__ src, void* __restrict__ yv, void* __restrict__ cbv,
                                                                 void* __restrict__ crv, int h, int w, YuvWindow g, YuvFwd k) {
    static_assert(C444 || D10, "8-bit 4:2:0 is clip_window_to_yuv420_kernel's");
    typedef typename YuvDepth<D10>::sample S;
    constexpr int SB = (int)sizeof(S);
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = (h + 1) / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int rows = min(2, h - y0), n = min(YUV_RUN, w - x0);                  // 4:2:0: rows == 2 and n even
    const float* in = src + t * g.st + y0 * g.sr + x0;
    S* yd = reinterpret_cast<S*>(yv) + t * g.yf + y0 * g.yp + x0;
    const long long co = C444 ? t * g.cf + y0 * g.cp + x0 : t * g.cf + ry * g.cp + (x0 >> 1);
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
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* p = in + r * g.sr + q * 4;
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
                    } else {
                        sr[px >> 1] += ir; sg[px >> 1] += ig; sb[px >> 1] += ib;
                    }
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
                yuv_pack<SB>(bw, c, yuv_chroma4<D10>(k.fcb, sr[c], sg[c], sb[c]));
                yuv_pack<SB>(rw, c, yuv_chroma4<D10>(k.fcr, sr[c], sg[c], sb[c]));
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
        for (int c = 0; c < n / 2; ++c) {                                       // one 2x2 block at a time
            int r4 = 0, g4 = 0, b4 = 0;
            for (int r = 0; r < 2; ++r)
                for (int j = 0; j < 2; ++j) {
                    const float* p = in + r * g.sr + c * 2 + j;
                    const int ir = yuv_quant<D10>(p[0]), ig = yuv_quant<D10>(p[g.sc]), ib = yuv_quant<D10>(p[2 * g.sc]);
                    yd[r * g.yp + c * 2 + j] = (S)yuv_luma_d<D10>(k, ir, ig, ib);
                    r4 += ir; g4 += ig; b4 += ib;
                }
            cbd[c] = (S)yuv_chroma4<D10>(k.fcb, r4, g4, b4);
            crd[c] = (S)yuv_chroma4<D10>(k.fcr, r4, g4, b4);
        }
    }
}

// ---- siting-aware 4:2:0 (uav_yuv420_sited_to_clip_f32 / uav_clip_to_yuv420_sited): `--chroma sited` of the front end ----------
// Decode: bilinear chroma up-sampling at the siting of the input's tag instead of replication.  Per axis a luma sample takes two
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
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = (h + 1) / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int rows = min(2, h - y0), n = min(YUV_RUN, w - x0);
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const long long hw = (long long)h * w;
    const unsigned char* ysrc = yp + ((long long)t * h + y0) * w + x0;
    float* out = dst + ((long long)t * h + y0) * w + x0;                       // channel stride: t_len * hw
    const long long cs = (long long)t_len * hw;
    const long long crow[3] = {((long long)t * ch + max(ry - 1, 0)) * cw, ((long long)t * ch + ry) * cw,
                               ((long long)t * ch + min(ry + 1, ch - 1)) * cw};
    if (MODE > 0 && n == YUV_RUN) {
        const int i0 = x0 >> 1, il = max(i0 - 1, 0), ir = min(i0 + 4, cw - 1);  // i0 + 3 <= cw - 1: the run is whole
        int cbs[3][6], crs[3][6];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned char* pb = cbp + crow[a];
            const unsigned char* pr = crp + crow[a];
            uint32_t bw, rw;
            if (MODE == 2) {
                bw = *reinterpret_cast<const uint32_t*>(pb + i0);
                rw = *reinterpret_cast<const uint32_t*>(pr + i0);
            } else {
                const unsigned short* hb = reinterpret_cast<const unsigned short*>(pb + i0);
                const unsigned short* hr = reinterpret_cast<const unsigned short*>(pr + i0);
                bw = (uint32_t)hb[0] | ((uint32_t)hb[1] << 16);
                rw = (uint32_t)hr[0] | ((uint32_t)hr[1] << 16);
            }
            cbs[a][0] = pb[il]; crs[a][0] = pr[il];
#pragma unroll
            for (int j = 0; j < 4; ++j) { cbs[a][1 + j] = (int)yuv_byte(bw, j); crs[a][1 + j] = (int)yuv_byte(rw, j); }
            cbs[a][5] = pb[ir]; crs[a][5] = pr[ir];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) break;
            uint32_t yw[2];
            if (MODE == 2) {
                const uint2_t v = *reinterpret_cast<const uint2_t*>(ysrc + (long long)r * w);
                yw[0] = v.x; yw[1] = v.y;
            } else {
                yw[0] = *reinterpret_cast<const uint32_t*>(ysrc + (long long)r * w);
                yw[1] = *reinterpret_cast<const uint32_t*>(ysrc + (long long)r * w + 4);
            }
            const int wa = r ? s.vo0 : s.ve0, wb = r ? s.vo1 : s.ve1;           // rows (ry-1, ry) for the even row, (ry, ry+1) for the odd one
            int ub[6], vb[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) { ub[c] = wa * cbs[r][c] + wb * cbs[r + 1][c]; vb[c] = wa * crs[r][c] + wb * crs[r + 1][c]; }
#pragma unroll
            for (int q = 0; q < 2; ++q) {                                       // 4 pixels = one 16-byte store per channel
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
                float* o = out + (long long)r * w + q * 4;
                *reinterpret_cast<float4_t*>(o) = R;
                *reinterpret_cast<float4_t*>(o + cs) = G;
                *reinterpret_cast<float4_t*>(o + 2 * cs) = B;
            }
        }
        return;
    }
    for (int r = 0; r < rows; ++r) {
        const long long ra = r ? crow[1] : crow[0], rb = r ? crow[2] : crow[1];
        const int wa = r ? s.vo0 : s.ve0, wb = r ? s.vo1 : s.ve1;
        for (int j = 0; j < n; ++j) {
            const int x = x0 + j, ci = x >> 1;
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

// Encode, horizontally co-sited and vertically centred (the siting of `C420mpeg2` and `C420p10`): a chroma sample is made from
// the (1,2,1) filter around its EVEN luma column in both rows of its block, weights totalling 8, one rounding.
template <bool D10> UAV_DEVINL int yuv_chroma8(const int* f, int r, int g, int b) {
    return yuv_clampd<D10>(((f[0] * r + f[1] * g + f[2] * b + (1 << 18)) >> 19) + YuvDepth<D10>::centre);
}

// frames (T,3,H,W) fp32 in [-1,1], H and W even -> planes Y (T,H,W), Cb / Cr (T,H/2,W/2), contiguous.  Ownership and MODEs of
// clip_window_to_yuv_kernel; a thread reads one more column, x0 - 1 (clamped to the frame), per row and channel.
template <int MODE, bool D10>
__global__ __launch_bounds__(256) void clip_to_yuv420_sited_kernel(const float* __restrict__ src, void* __restrict__ yv, void* __restrict__ cbv,
                                                                   void* __restrict__ crv, int h, int w, YuvFwd k) {
    typedef typename YuvDepth<D10>::sample S;
    constexpr int SB = (int)sizeof(S);
    const int nrx = (w + YUV_RUN - 1) / YUV_RUN, nry = h / 2, cw = w / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nrx * nry) return;
    const int t = blockIdx.y, ry = (int)(i / nrx), x0 = (int)(i - (long long)ry * nrx) * YUV_RUN, y0 = ry * 2;
    const int n = min(YUV_RUN, w - x0);                                         // even
    const long long hw = (long long)h * w;
    const float* in = src + (long long)t * 3 * hw + (long long)y0 * w + x0;    // channel stride: hw
    S* yd = reinterpret_cast<S*>(yv) + (long long)t * hw + (long long)y0 * w + x0;
    const long long co = ((long long)t * nry + ry) * cw + (x0 >> 1);
    S* cbd = reinterpret_cast<S*>(cbv) + co;
    S* crd = reinterpret_cast<S*>(crv) + co;
    if (MODE > 0 && n == YUV_RUN) {
        constexpr int NW = YUV_RUN * SB / 4;                                    // 32-bit words of a run's luma samples of one row
        const int back = x0 > 0 ? 1 : 0;
        int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t yw[NW];
#pragma unroll
            for (int q = 0; q < NW; ++q) yw[q] = 0;
            const float* p0 = in + (long long)r * w;
            int pr = yuv_quant<D10>(p0[-back]), pg = yuv_quant<D10>(p0[hw - back]), pb = yuv_quant<D10>(p0[2 * hw - back]);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float* p = p0 + q * 4;
                const float4_t R = *reinterpret_cast<const float4_t*>(p);
                const float4_t G = *reinterpret_cast<const float4_t*>(p + hw);
                const float4_t B = *reinterpret_cast<const float4_t*>(p + 2 * hw);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int px = q * 4 + j;
                    const int ir = yuv_quant<D10>(R[j]), ig = yuv_quant<D10>(G[j]), ib = yuv_quant<D10>(B[j]);
                    yuv_pack<SB>(yw, px, yuv_luma_d<D10>(k, ir, ig, ib));
                    if (px & 1) { sr[px >> 1] += ir; sg[px >> 1] += ig; sb[px >> 1] += ib; }
                    else { sr[px >> 1] += pr + 2 * ir; sg[px >> 1] += pg + 2 * ig; sb[px >> 1] += pb + 2 * ib; }
                    pr = ir; pg = ig; pb = ib;
                }
            }
            yuv_store_run<MODE, YUV_RUN * SB>(yd + (long long)r * w, yw);
        }
        uint32_t bw[2] = {0, 0}, rw[2] = {0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            yuv_pack<SB>(bw, c, yuv_chroma8<D10>(k.fcb, sr[c], sg[c], sb[c]));
            yuv_pack<SB>(rw, c, yuv_chroma8<D10>(k.fcr, sr[c], sg[c], sb[c]));
        }
        if constexpr (SB == 2) {
            yuv_store_run<MODE, 8>(cbd, bw);
            yuv_store_run<MODE, 8>(crd, rw);
        } else if constexpr (MODE == 2) {
            yuv_store<4>(cbd, bw);
            yuv_store<4>(crd, rw);
        } else {
            unsigned short* a = reinterpret_cast<unsigned short*>(cbd);
            unsigned short* b = reinterpret_cast<unsigned short*>(crd);
            a[0] = (unsigned short)bw[0]; a[1] = (unsigned short)(bw[0] >> 16);
            b[0] = (unsigned short)rw[0]; b[1] = (unsigned short)(rw[0] >> 16);
        }
        return;
    }
    for (int c = 0; c < n / 2; ++c) {                                           // one chroma sample and its 2x2 luma block at a time
        const int back = x0 + c * 2 > 0 ? 1 : 0;
        int s_r = 0, s_g = 0, s_b = 0;
        for (int r = 0; r < 2; ++r) {
            const float* p = in + (long long)r * w + c * 2;
            const int r0 = yuv_quant<D10>(p[0]), g0 = yuv_quant<D10>(p[hw]), b0 = yuv_quant<D10>(p[2 * hw]);
            const int r1 = yuv_quant<D10>(p[1]), g1 = yuv_quant<D10>(p[hw + 1]), b1 = yuv_quant<D10>(p[2 * hw + 1]);
            yd[(long long)r * w + c * 2] = (S)yuv_luma_d<D10>(k, r0, g0, b0);
            yd[(long long)r * w + c * 2 + 1] = (S)yuv_luma_d<D10>(k, r1, g1, b1);
            s_r += yuv_quant<D10>(p[-back]) + 2 * r0 + r1;
            s_g += yuv_quant<D10>(p[hw - back]) + 2 * g0 + g1;
            s_b += yuv_quant<D10>(p[2 * hw - back]) + 2 * b0 + b1;
        }
        cbd[c] = (S)yuv_chroma8<D10>(k.fcb, s_r, s_g, s_b);
        crd[c] = (S)yuv_chroma8<D10>(k.fcr, s_r, s_g, s_b);
    }
}

inline bool yuv_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline int yuv_mode(int w, const void* f32, const void* y, const void* cb, const void* cr, bool c444) {
    if (!yuv_aligned(f32, 16)) return 0;
    if (w % 8 == 0 && yuv_aligned(y, 8) && yuv_aligned(cb, 4) && yuv_aligned(cr, 4)) return 2;
    if (w % 4 == 0 && yuv_aligned(y, 4) && yuv_aligned(cb, c444 ? 4 : 2) && yuv_aligned(cr, c444 ? 4 : 2)) return 1;
    return 0;
}

template <bool C444>
int yuv_to_clip_launch(const void* y, const void* cb, const void* cr, float* clip, int32_t t_len, int32_t h, int32_t w,
                       const int32_t* coefs, void* stream) {
    if (!y || !cb || !cr || !clip || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0) return UAV_ESHAPE;
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * ((h + 1) / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    const YuvInv k = {coefs[0], coefs[1], coefs[2], coefs[3], coefs[4], coefs[5]};
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    const unsigned char *yp = (const unsigned char*)y, *cbp = (const unsigned char*)cb, *crp = (const unsigned char*)cr;
    switch (yuv_mode(w, clip, y, cb, cr, C444)) {
    case 2: hipLaunchKernelGGL((yuv_to_clip_kernel<2, C444>), grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip, t_len, h, w, k); break;
    case 1: hipLaunchKernelGGL((yuv_to_clip_kernel<1, C444>), grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip, t_len, h, w, k); break;
    default: hipLaunchKernelGGL((yuv_to_clip_kernel<0, C444>), grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip, t_len, h, w, k);
    }
    return uav_launch_status();
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

extern "C" int uav_clip_to_yuv420_u8(const float* frames_tchw, void* y, void* cb, void* cr, int32_t t_len, int32_t h, int32_t w,
                                     const int32_t* coefs, void* stream) {
    if (!frames_tchw || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return UAV_ESHAPE;
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * (h / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    YuvFwd k;
    for (int i = 0; i < 3; ++i) { k.fy[i] = coefs[i]; k.fcb[i] = coefs[3 + i]; k.fcr[i] = coefs[6 + i]; }
    k.yo = coefs[9];
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    unsigned char *yp = (unsigned char*)y, *cbp = (unsigned char*)cb, *crp = (unsigned char*)cr;
    switch (yuv_mode(w, frames_tchw, y, cb, cr, false)) {
    case 2: hipLaunchKernelGGL(clip_to_yuv420_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, frames_tchw, yp, cbp, crp, h, w, k); break;
    case 1: hipLaunchKernelGGL(clip_to_yuv420_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, frames_tchw, yp, cbp, crp, h, w, k); break;
    default: hipLaunchKernelGGL(clip_to_yuv420_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, frames_tchw, yp, cbp, crp, h, w, k);
    }
    return uav_launch_status();
}

extern "C" int uav_clip_window_to_yuv420_u8(const float* src, int64_t src_c_stride, int64_t src_t_stride, int64_t src_row_stride,
                                            void* y, int64_t y_pitch, int64_t y_frame, void* cb, void* cr, int64_t c_pitch,
                                            int64_t c_frame, int32_t t_len, int32_t h, int32_t w, const int32_t* coefs, void* stream) {
    if (!src || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return UAV_ESHAPE;
    // no negative strides, and the rows / frames of a plane must not overlap (two threads would own one byte)
    if (src_c_stride < 0 || src_t_stride < 0 || src_row_stride < 0 || y_pitch < w || c_pitch < w / 2) return UAV_ESHAPE;
    if (t_len > 1 && (y_frame < (int64_t)(h - 1) * y_pitch + w || c_frame < (int64_t)(h / 2 - 1) * c_pitch + w / 2)) return UAV_ESHAPE;
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * (h / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    YuvFwd k;
    for (int i = 0; i < 3; ++i) { k.fy[i] = coefs[i]; k.fcb[i] = coefs[3 + i]; k.fcr[i] = coefs[6 + i]; }
    k.yo = coefs[9];
    const YuvWindow g = {src_c_stride, src_t_stride, src_row_stride, y_pitch, y_frame, c_pitch, c_frame};
    // the vector modes of yuv_mode() hold for every row of every frame only when the strides keep the alignment of the bases
    int mode = (src_c_stride | src_t_stride | src_row_stride) % 4 == 0 ? yuv_mode(w, src, y, cb, cr, false) : 0;
    if (mode == 2 && ((y_pitch | y_frame) % 8 != 0 || (c_pitch | c_frame) % 4 != 0)) mode = 1;      // what mode 2 asks implies mode 1
    if (mode == 1 && ((y_pitch | y_frame) % 4 != 0 || (c_pitch | c_frame) % 2 != 0)) mode = 0;
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    unsigned char *yp = (unsigned char*)y, *cbp = (unsigned char*)cb, *crp = (unsigned char*)cr;
    switch (mode) {
    case 2: hipLaunchKernelGGL(clip_window_to_yuv420_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, src, yp, cbp, crp, h, w, g, k); break;
    case 1: hipLaunchKernelGGL(clip_window_to_yuv420_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, yp, cbp, crp, h, w, g, k); break;
    default: hipLaunchKernelGGL(clip_window_to_yuv420_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, src, yp, cbp, crp, h, w, g, k);
    }
    return uav_launch_status();
}

namespace {
template <bool C444, bool D10>
void clip_window_to_yuv_launch(int mode, dim3 grid, hipStream_t s, const float* src, void* y, void* cb, void* cr, int h, int w,
                               const YuvWindow& g, const YuvFwd& k) {
    switch (mode) {
    case 2: hipLaunchKernelGGL((clip_window_to_yuv_kernel<2, C444, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, g, k); break;
    case 1: hipLaunchKernelGGL((clip_window_to_yuv_kernel<1, C444, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, g, k); break;
    default: hipLaunchKernelGGL((clip_window_to_yuv_kernel<0, C444, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, g, k);
    }
}
}  // namespace

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
    if (!yuv_aligned(y, sb) || !yuv_aligned(cb, sb) || !yuv_aligned(cr, sb)) return UAV_EALIGN;
    if (!chroma444 && depth == 8)                                               // the format of the entry point above: its kernels
        return uav_clip_window_to_yuv420_u8(src, src_c_stride, src_t_stride, src_row_stride, y, y_pitch, y_frame, cb, cr, c_pitch,
                                            c_frame, t_len, h, w, coefs, stream);
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * ((h + 1) / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    YuvFwd k;
    for (int i = 0; i < 3; ++i) { k.fy[i] = coefs[i]; k.fcb[i] = coefs[3 + i]; k.fcr[i] = coefs[6 + i]; }
    k.yo = coefs[9];
    const YuvWindow g = {src_c_stride, src_t_stride, src_row_stride, y_pitch, y_frame, c_pitch, c_frame};
    // a vector mode holds for every row of every frame only when pointers, strides and pitches keep the alignment: `a` luma
    // samples per store (8 in mode 2, 4 in mode 1), as many chroma samples in 4:4:4 and half as many in 4:2:0
    const auto planes_ok = [&](int64_t a) {
        const int64_t c = chroma444 ? a : a / 2;
        return w % a == 0 && yuv_aligned(y, a * sb) && (y_pitch | y_frame) % a == 0 && yuv_aligned(cb, c * sb) && yuv_aligned(cr, c * sb) &&
               (c_pitch | c_frame) % c == 0;
    };
    int mode = 0;
    if ((src_c_stride | src_t_stride | src_row_stride) % 4 == 0 && yuv_aligned(src, 16)) mode = planes_ok(8) ? 2 : planes_ok(4) ? 1 : 0;
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    hipStream_t s = (hipStream_t)stream;
    if (depth == 8) clip_window_to_yuv_launch<true, false>(mode, grid, s, src, y, cb, cr, h, w, g, k);
    else if (chroma444) clip_window_to_yuv_launch<true, true>(mode, grid, s, src, y, cb, cr, h, w, g, k);
    else clip_window_to_yuv_launch<false, true>(mode, grid, s, src, y, cb, cr, h, w, g, k);
    return uav_launch_status();
}

extern "C" int uav_yuv420_sited_to_clip_f32(const void* y, const void* cb, const void* cr, float* clip_cthw, int32_t t_len, int32_t h,
                                            int32_t w, int32_t centre_h, int32_t centre_v, const int32_t* coefs, void* stream) {
    if (!y || !cb || !cr || !clip_cthw || !coefs) return UAV_EINVAL;
    if ((centre_h != 0 && centre_h != 1) || (centre_v != 0 && centre_v != 1)) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0) return UAV_ESHAPE;
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * ((h + 1) / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    const YuvInv k = {coefs[0], coefs[1], coefs[2], coefs[3], coefs[4], coefs[5]};
    YuvSiting s;
    s.he0 = centre_h ? 1 : 0; s.he1 = centre_h ? 3 : 4; s.ho0 = centre_h ? 3 : 2; s.ho1 = centre_h ? 1 : 2;
    s.ve0 = centre_v ? 1 : 0; s.ve1 = centre_v ? 3 : 4; s.vo0 = centre_v ? 3 : 2; s.vo1 = centre_v ? 1 : 2;
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    const unsigned char *yp = (const unsigned char*)y, *cbp = (const unsigned char*)cb, *crp = (const unsigned char*)cr;
    switch (yuv_mode(w, clip_cthw, y, cb, cr, false)) {
    case 2: hipLaunchKernelGGL(yuv_sited_to_clip_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip_cthw, t_len, h, w, k, s); break;
    case 1: hipLaunchKernelGGL(yuv_sited_to_clip_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip_cthw, t_len, h, w, k, s); break;
    default: hipLaunchKernelGGL(yuv_sited_to_clip_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, yp, cbp, crp, clip_cthw, t_len, h, w, k, s);
    }
    return uav_launch_status();
}

namespace {
template <bool D10>
void clip_to_yuv420_sited_launch(int mode, dim3 grid, hipStream_t s, const float* src, void* y, void* cb, void* cr, int h, int w,
                                 const YuvFwd& k) {
    switch (mode) {
    case 2: hipLaunchKernelGGL((clip_to_yuv420_sited_kernel<2, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, k); break;
    case 1: hipLaunchKernelGGL((clip_to_yuv420_sited_kernel<1, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, k); break;
    default: hipLaunchKernelGGL((clip_to_yuv420_sited_kernel<0, D10>), grid, dim3(256), 0, s, src, y, cb, cr, h, w, k);
    }
}
}  // namespace

extern "C" int uav_clip_to_yuv420_sited(const float* frames_tchw, void* y, void* cb, void* cr, int32_t t_len, int32_t h, int32_t w,
                                        int32_t depth, const int32_t* coefs, void* stream) {
    if (!frames_tchw || !y || !cb || !cr || !coefs) return UAV_EINVAL;
    if (depth != 8 && depth != 10) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0 || (h & 1) || (w & 1)) return UAV_ESHAPE;
    const uintptr_t sb = depth == 10 ? 2 : 1;                                   // bytes per sample
    if (!yuv_aligned(y, sb) || !yuv_aligned(cb, sb) || !yuv_aligned(cr, sb)) return UAV_EALIGN;
    const long long threads = (long long)((w + YUV_RUN - 1) / YUV_RUN) * (h / 2), blocks = (threads + 255) / 256;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    YuvFwd k;
    for (int i = 0; i < 3; ++i) { k.fy[i] = coefs[i]; k.fcb[i] = coefs[3 + i]; k.fcr[i] = coefs[6 + i]; }
    k.yo = coefs[9];
    // contiguous planes: rows and frames keep the alignment of the bases when w allows the mode at all
    const auto planes_ok = [&](uintptr_t a) {
        return w % (int)a == 0 && yuv_aligned(y, a * sb) && yuv_aligned(cb, a / 2 * sb) && yuv_aligned(cr, a / 2 * sb);
    };
    const int mode = !yuv_aligned(frames_tchw, 16) ? 0 : planes_ok(8) ? 2 : planes_ok(4) ? 1 : 0;
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    if (depth == 10) clip_to_yuv420_sited_launch<true>(mode, grid, (hipStream_t)stream, frames_tchw, y, cb, cr, h, w, k);
    else clip_to_yuv420_sited_launch<false>(mode, grid, (hipStream_t)stream, frames_tchw, y, cb, cr, h, w, k);
    return uav_launch_status();
}

extern "C" int64_t uav_plane_stats_workspace_bytes(int32_t planes) { return (int64_t)planes * CF_CHUNKS * 2 * 8; }

extern "C" int uav_plane_stats_f32(const float* x, int32_t planes, int64_t hw, float* mean_out, float* var_out, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    if (!x || !mean_out || !var_out || !workspace) return UAV_EINVAL;
    if (planes <= 0 || planes > 65535 || hw <= 0) return UAV_ESHAPE;
    if (workspace_bytes < uav_plane_stats_workspace_bytes(planes)) return UAV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(plane_partial_kernel, dim3(CF_CHUNKS, planes), dim3(256), 0, s, x, (long long)hw, (double*)workspace);
    hipLaunchKernelGGL(plane_finalize_kernel, dim3((planes + 63) / 64), dim3(64), 0, s, (const double*)workspace, planes,
                       (long long)hw, mean_out, var_out);
    return uav_launch_status();
}

extern "C" int uav_adain_apply_f32(const float* x, float* out, int32_t planes, int64_t hw, const float* c_mean, const float* c_var,
                                   const float* s_mean, const float* s_var, float eps, void* stream) {
    if (!x || !out || !c_mean || !c_var || !s_mean || !s_var) return UAV_EINVAL;
    if (planes <= 0 || planes > 65535 || hw <= 0) return UAV_ESHAPE;
    const long long blocks = (hw + 1023) / 1024;
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    hipLaunchKernelGGL(adain_apply_kernel, dim3((unsigned)blocks, planes), dim3(256), 0, (hipStream_t)stream, x, out, (long long)hw,
                       c_mean, c_var, s_mean, s_var, eps);
    return uav_launch_status();
}

extern "C" int uav_atrous_blur_f32(const float* src, float* low_out, float* high_inout, int32_t planes, int32_t h, int32_t w,
                                   int32_t radius, void* stream) {
    if (!src || !low_out || src == low_out) return UAV_EINVAL;
    if (planes <= 0 || planes > 65535 || h <= 0 || h > 65535 || w <= 0 || radius <= 0) return UAV_ESHAPE;
    hipLaunchKernelGGL(atrous_blur_kernel, dim3((w + 255) / 256, h, planes), dim3(256), 0, (hipStream_t)stream, src, low_out,
                       high_inout, h, w, radius);
    return uav_launch_status();
}

extern "C" int uav_resize_bicubic_f32(const float* src, float* dst, int32_t planes, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                                      float scale_h, float scale_w, void* stream) {
    if (!src || !dst) return UAV_EINVAL;
    if (planes <= 0 || planes > 65535 || hi <= 0 || wi <= 0 || ho <= 0 || ho > 65535 || wo <= 0 || scale_h <= 0.f || scale_w <= 0.f)
        return UAV_ESHAPE;
    hipLaunchKernelGGL(resize_bicubic_kernel, dim3((wo + 255) / 256, ho, planes), dim3(256), 0, (hipStream_t)stream, src, dst, hi, wi,
                       ho, wo, scale_h, scale_w);
    return uav_launch_status();
}
