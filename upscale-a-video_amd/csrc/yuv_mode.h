// The access mode of the K13 Y'CbCr kernels (csrc/yuv_io.hip), picked on the host from the row width and from the alignment
// of every address, stride and pitch a thread will form.  Plain C++ on integers, no HIP: a host program can include it.
//   mode 2: a thread's 8 pixels of a row move as whole vectors (fp32 as 16-byte loads / stores, a plane's samples as one word);
//   mode 1: the planes move as two half-width words, a 4-pixel tail of a row is scalar;
//   mode 0: scalar throughout, any width and alignment.
#pragma once
#include <stdint.h>

inline bool yuv_aligned(uintptr_t p, uintptr_t a) { return (p & (a - 1)) == 0; }

// Decode, contiguous tensors: 8-bit planes Y (T,H,W), Cb / Cr (4:2:0: (T,ceil(H/2),ceil(W/2)); c444: (T,H,W)) -> fp32 at `f32`.
inline int yuv_decode_mode(int w, uintptr_t f32, uintptr_t y, uintptr_t cb, uintptr_t cr, bool c444) {
    if (!yuv_aligned(f32, 16)) return 0;
    if (w % 8 == 0 && yuv_aligned(y, 8) && yuv_aligned(cb, 4) && yuv_aligned(cr, 4)) return 2;
    if (w % 4 == 0 && yuv_aligned(y, 4) && yuv_aligned(cb, c444 ? 4 : 2) && yuv_aligned(cr, c444 ? 4 : 2)) return 1;
    return 0;
}

// Encode: fp32 at `src` with element strides of channel / frame / row -> planes of `sb`-byte samples with row pitches and frame
// strides in samples.  A vector mode holds for every row of every frame only when bases, strides and pitches all keep the
// alignment: `a` luma samples per store (8 in mode 2, 4 in mode 1), as many chroma samples in 4:4:4 and half as many in 4:2:0.
inline int yuv_encode_mode(int w, uintptr_t src, uintptr_t y, uintptr_t cb, uintptr_t cr, int64_t sc, int64_t st, int64_t sr,
                           int64_t y_pitch, int64_t y_frame, int64_t c_pitch, int64_t c_frame, int sb, bool c444) {
    if ((sc | st | sr) % 4 != 0 || !yuv_aligned(src, 16)) return 0;
    for (int mode = 2; mode > 0; --mode) {
        const int a = 4 * mode, c = c444 ? a : a / 2;
        if (w % a == 0 && yuv_aligned(y, (uintptr_t)(a * sb)) && (y_pitch | y_frame) % a == 0 && yuv_aligned(cb, (uintptr_t)(c * sb)) &&
            yuv_aligned(cr, (uintptr_t)(c * sb)) && (c_pitch | c_frame) % c == 0)
            return mode;
    }
    return 0;
}
