// Host program of tests/test_yuv_mode_cpu.py: the mode pickers of csrc/yuv_mode.h over a grid.
// stdin: records of 15 little-endian int64 — kind (0 decode, 1 encode), w, fp32 address, y, cb, cr addresses, source strides of
// channel / frame / row, y_pitch, y_frame, c_pitch, c_frame, bytes per sample, c444 (a decode record uses w, the addresses and
// c444).  stdout: one character '0' + mode per record.
#include <cstdio>
#include <vector>
#include "../upscale-a-video_amd/csrc/yuv_mode.h"

int main() {
    int64_t r[15];
    std::vector<char> out;
    while (fread(r, sizeof r, 1, stdin) == 1) {
        const int w = (int)r[1];
        const uintptr_t f32 = (uintptr_t)r[2], y = (uintptr_t)r[3], cb = (uintptr_t)r[4], cr = (uintptr_t)r[5];
        const int mode = r[0] == 0 ? yuv_decode_mode(w, f32, y, cb, cr, r[14] != 0)
                                   : yuv_encode_mode(w, f32, y, cb, cr, r[6], r[7], r[8], r[9], r[10], r[11], r[12], (int)r[13], r[14] != 0);
        out.push_back((char)('0' + mode));
    }
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}
