// Scene statistics of a clip for the front end's `--scenes auto` (uav_clip_scene_stats): per frame the 64-bin histogram of the
// 8-bit luma and the sum of absolute luma differences to the frame before, all in integers, so every output is defined bit for
// bit and does not depend on the order in which partial sums arrive.  The luma is the one the encoders write: yuv_clip_to_u8 and
// yuv_luma_d<false> of yuv_common.h on the forward table the host passes.
//
// Design: ONE pass over the clip.  A thread owns SCENE_RUN = 4 consecutive pixels of the flattened frame (h*w) and walks the
// frames with the previous luma of its pixels in registers, so no luma plane is written and nothing is read twice but one
// frame per block: block b starts at frame t0 = b % T, after frame t0 - 1 once for its luma alone, and wraps around, so that at
// any moment the blocks add to T different rows of `hist` and `sad` instead of all to one row, where every block's atomics
// would queue behind each other.  Bytes: 12 per pixel and frame read, times (1 + 1/T).  The next frame's loads are
// issued before the current frame is reduced.  Per frame a wave counts into its own 64-bin histogram in LDS (LDS atomics) and
// reduces its SAD with shuffles; after one barrier 64 threads add the four copies into hist[t] — one wave instruction, 256
// contiguous bytes — and one thread adds the four wave sums into sad[t], with ordinary vector atomics: at most 64 + 1 global
// atomics per block and frame (empty bins are skipped), (64*4 + 8) bytes.  The LDS buffers alternate between frames so that
// one barrier per frame is enough.  A block covers 1024 pixels: 900 blocks at 720p, 100 at 320x320.  Unlike the encoders' flat
// grid, a block pays a serial chain per frame: load -> LDS -> barrier -> atomics (measured: profiles/scene_stats_kernel.txt).
//
// Loads are 16-byte when the clip's base is 16-byte aligned and h*w % 4 == 0 (every plane of every frame then starts aligned,
// whatever w is); otherwise every load is scalar and the last thread of a frame owns fewer than 4 pixels.  No scratch.
#include "uav_common.h"
#include "yuv_common.h"

namespace {
constexpr int SCENE_RUN = 4, SCENE_BINS = 64, SCENE_WAVES = 4;
constexpr int SCENE_DEPTH = 1;          // frames loaded ahead of the one being reduced

UAV_DEVINL int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the n <= 4 pixels at `p` of the three channels, `cs` elements apart
template <bool VEC> UAV_DEVINL void scene_load(const float* __restrict__ p, long long cs, int n, float (&v)[3][SCENE_RUN]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC) {
            if (n == SCENE_RUN) {
                const float4_t q = *reinterpret_cast<const float4_t*>(p + c * cs);
#pragma unroll
                for (int j = 0; j < SCENE_RUN; ++j) v[c][j] = q[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < SCENE_RUN; ++j)
                if (j < n) v[c][j] = p[c * cs + j];
        }
    }
}

// clip (3,T,h,w) fp32, hw = h*w -> hist [T][64] int32, sad [T] 64-bit; both zeroed by the launcher
template <bool VEC>
__global__ __launch_bounds__(256) void clip_scene_stats_kernel(const float* __restrict__ src, int* __restrict__ hist,
                                                               unsigned long long* __restrict__ sad, int t_len, long long hw, YuvFwd k) {
    __shared__ int s_hist[2][SCENE_WAVES][SCENE_BINS];
    __shared__ int s_sad[2][SCENE_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 2 * SCENE_WAVES * SCENE_BINS; i += 256) (&s_hist[0][0][0])[i] = 0;
    __syncthreads();
    const long long p = ((long long)blockIdx.x * 256 + tid) * SCENE_RUN;
    const int n = p >= hw ? 0 : (int)min(hw - p, (long long)SCENE_RUN);     // VEC: 0 or 4
    const long long cs = (long long)t_len * hw;
    // The block walks the frames t0, t0 + 1, ..., T - 1, 0, ..., t0 - 1, after frame t0 - 1 once for its luma alone (step -1).
    const int t0 = (int)(blockIdx.x % (unsigned)t_len);
    const int first = t0 > 0 ? -1 : 0;
    float v[SCENE_DEPTH + 1][3][SCENE_RUN];
#pragma unroll
    for (int a = 0; a <= SCENE_DEPTH; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < SCENE_RUN; ++j) v[a][c][j] = 0.0f;
#pragma unroll
    for (int a = 0; a < SCENE_DEPTH; ++a) {
        const int i = first + a;
        if (n > 0 && i < t_len) scene_load<VEC>(src + (long long)((t0 + i + t_len) % t_len) * hw + p, cs, n, v[a]);
    }
    int prev[SCENE_RUN] = {0, 0, 0, 0};
    for (int i = first; i < t_len; ++i) {
        const int t = (t0 + i + t_len) % t_len, buf = i & 1;
        if (n > 0 && i + SCENE_DEPTH < t_len)
            scene_load<VEC>(src + (long long)((t0 + i + SCENE_DEPTH + t_len) % t_len) * hw + p, cs, n, v[SCENE_DEPTH]);
        if (i >= 0) {
            int d = 0;
#pragma unroll
            for (int j = 0; j < SCENE_RUN; ++j)
                if (j < n) {
                    const int y = yuv_luma_d<false>(k, yuv_clip_to_u8(v[0][0][j]), yuv_clip_to_u8(v[0][1][j]), yuv_clip_to_u8(v[0][2][j]));
                    atomicAdd(&s_hist[buf][wave][y >> 2], 1);
                    d += abs(y - prev[j]);
                    prev[j] = y;
                }
            d = wave_sum_int(d);                                            // at most 256 * 255 per wave
            if (lane == 0) s_sad[buf][wave] = d;
            __syncthreads();
            // This step's buffers are next written two steps on, after the next barrier: one barrier per frame.
            if (tid < SCENE_BINS) {
                int s = 0;
#pragma unroll
                for (int q = 0; q < SCENE_WAVES; ++q) { s += s_hist[buf][q][tid]; s_hist[buf][q][tid] = 0; }
                if (s) atomicAdd(&hist[(long long)t * SCENE_BINS + tid], s);
            } else if (tid == SCENE_BINS && t > 0) {                        // sad[0] stays 0: there is no frame before the first
                int s = 0;
#pragma unroll
                for (int q = 0; q < SCENE_WAVES; ++q) s += s_sad[buf][q];
                if (s) atomicAdd(&sad[t], (unsigned long long)s);
            }
        } else {
#pragma unroll
            for (int j = 0; j < SCENE_RUN; ++j)
                if (j < n) prev[j] = yuv_luma_d<false>(k, yuv_clip_to_u8(v[0][0][j]), yuv_clip_to_u8(v[0][1][j]), yuv_clip_to_u8(v[0][2][j]));
        }
#pragma unroll
        for (int a = 0; a < SCENE_DEPTH; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < SCENE_RUN; ++j) v[a][c][j] = v[a + 1][c][j];
    }
}
}  // namespace

extern "C" int uav_clip_scene_stats(const float* clip_cthw, int32_t t_len, int32_t h, int32_t w, int32_t* hist, int64_t* sad,
                                    const int32_t* coefs, void* stream) {
    if (!clip_cthw || !hist || !sad || !coefs) return UAV_EINVAL;
    if (t_len <= 0 || t_len > 65535 || h <= 0 || w <= 0) return UAV_ESHAPE;
    const long long hw = (long long)h * w, blocks = (hw + 256 * SCENE_RUN - 1) / (256 * SCENE_RUN);
    if (blocks >= (1ll << 31)) return UAV_ESHAPE;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)t_len * SCENE_BINS * sizeof(int32_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(sad, 0, (size_t)t_len * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const YuvFwd k = yuv_fwd(coefs);
    const bool vec = ((uintptr_t)clip_cthw & 15) == 0 && hw % SCENE_RUN == 0;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "sad is accumulated as unsigned 64-bit");
    if (vec)
        hipLaunchKernelGGL(clip_scene_stats_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, clip_cthw, (int*)hist,
                           (unsigned long long*)sad, (int)t_len, hw, k);
    else
        hipLaunchKernelGGL(clip_scene_stats_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, clip_cthw, (int*)hist,
                           (unsigned long long*)sad, (int)t_len, hw, k);
    return uav_launch_status();
}
