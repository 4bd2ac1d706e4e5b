// What the K13 Y'CbCr encoders (csrc/yuv_io.hip) and the scene statistics (csrc/scene_stats.hip) share: the uint8 RGB value of a
// clip sample and the integer luma of the forward table, so that both files form the same Y for the same fp32 input bit for bit.
#pragma once
#include "uav_common.h"

// forward table {fy[3], fcb[3], fcr[3], yo}: RGB -> Y'CbCr in 16.16 fixed point (uav.video_io.yuv_coefficients(...).forward)
struct YuvFwd { int fy[3], fcb[3], fcr[3], yo; };
inline YuvFwd yuv_fwd(const int32_t* c) { return {{c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}, c[9]}; }

// [-1,1] -> uint8 value, the expression of clip_to_u8_kernel
UAV_DEVINL int yuv_clip_to_u8(float x) {
    float v = x / 2.0f + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f;
    return (int)v;
}

// D10: 16-bit samples 0..1023, chroma centre 512; else uint8 samples, chroma centre 128
template <bool D10> struct YuvDepth { typedef unsigned char sample; static constexpr int centre = 128, vmax = 255; };
template <> struct YuvDepth<true> { typedef unsigned short sample; static constexpr int centre = 512, vmax = 1023; };

template <bool D10> UAV_DEVINL int yuv_clampd(int v) { return min(max(v, 0), YuvDepth<D10>::vmax); }
template <bool D10> UAV_DEVINL int yuv_luma_d(const YuvFwd& k, int r, int g, int b) {
    return yuv_clampd<D10>(((k.fy[0] * r + k.fy[1] * g + k.fy[2] * b + 32768) >> 16) + k.yo);
}
