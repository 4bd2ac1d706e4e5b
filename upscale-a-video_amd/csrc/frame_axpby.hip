// The cross-fade of `--scene-overlap` (uav/video_io.py, SceneChunks) on gfx950: a per-frame weighted sum of two fp32 frame
// stacks in one launch, every bit defined.
//
//   frame_axpby_kernel<VEC>                            uav_frame_axpby_f32
//
//   out[t][i] = wa[t] * a[t][i] + wb[t] * b[t][i]      both products rounded to fp32, then added: no fused multiply-add
//
// HBM-bound elementwise, 12 bytes per element: blockIdx.y is the frame, a block of 256 threads owns FA_BLOCK consecutive
// elements of it and a thread FA_STEPS pieces of them, 256 pieces apart — a piece is 4 elements moved as 16-byte vectors
// (VEC: every base 16-byte aligned and frame_elems % 4 == 0, so every frame starts aligned and has no tail) or one element.
// All loads of a thread are issued before its first store.  `out` may be exactly `a` or exactly `b`: a thread reads only what it
// writes, so the pointers carry no __restrict__.  No LDS, no scratch, no atomics.
#include <type_traits>
#include "uav_common.h"

namespace {
constexpr int FA_STEPS = 2;
constexpr int FA_BLOCK = 256 * 4 * FA_STEPS;           // elements of a frame per block, in both variants

template <typename V> UAV_DEVINL V fa_blend(float wa, V a, float wb, V b) {
#pragma clang fp contract(off)          // the products are rounded before the sum, as numpy's float32 expression rounds them
    const V pa = a * wa;
    const V pb = b * wb;
    return pa + pb;
}

template <bool VEC>
__global__ __launch_bounds__(256) void frame_axpby_kernel(const float* a, const float* b, float* out, const float* __restrict__ wa,
                                                          const float* __restrict__ wb, long long n) {
    typedef typename std::conditional<VEC, float4_t, float>::type V;
    constexpr int PIECE = VEC ? 4 : 1, STEPS = FA_BLOCK / (256 * PIECE);
    const float fa = wa[blockIdx.y], fb = wb[blockIdx.y];
    const long long frame = (long long)blockIdx.y * n;
    const long long i0 = (long long)blockIdx.x * FA_BLOCK + (long long)threadIdx.x * PIECE;
    V va[STEPS], vb[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const long long i = i0 + (long long)s * 256 * PIECE;
        if (i < n) {                                    // VEC: n % 4 == 0, so the whole piece lies inside the frame
            va[s] = *reinterpret_cast<const V*>(a + frame + i);
            vb[s] = *reinterpret_cast<const V*>(b + frame + i);
        }
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const long long i = i0 + (long long)s * 256 * PIECE;
        if (i < n) *reinterpret_cast<V*>(out + frame + i) = fa_blend<V>(fa, va[s], fb, vb[s]);
    }
}
}  // namespace

extern "C" int uav_frame_axpby_f32(const float* a, const float* b, float* out, const float* wa, const float* wb, int32_t t_len,
                                   int64_t frame_elems, void* stream) {
    if (!a || !b || !out || !wa || !wb) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || frame_elems <= 0) return UAV_ESHAPE;
    const int64_t blocks = (frame_elems - 1) / FA_BLOCK + 1;
    if (blocks * 256 > 0xffffffffll) return UAV_ESHAPE;                         // a grid dimension counts its threads in 32 bits
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)out;
    if (((bits | (uintptr_t)wa | (uintptr_t)wb) & 3) != 0) return UAV_EALIGN;
    const dim3 grid((unsigned)blocks, (unsigned)t_len);
    if ((bits & 15) == 0 && frame_elems % 4 == 0)
        hipLaunchKernelGGL(frame_axpby_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a, b, out, wa, wb, (long long)frame_elems);
    else
        hipLaunchKernelGGL(frame_axpby_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a, b, out, wa, wb, (long long)frame_elems);
    return uav_launch_status();
}
