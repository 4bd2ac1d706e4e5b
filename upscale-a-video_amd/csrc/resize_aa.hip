// K12b — antialiased separable cubic resize of fp32 planes (planes, hi, wi) -> (planes, ho, wo): the down-sampler between the
// decoder's 4x frames and the encoder (CLI --out-size / --out-scale).  Definition: include/uav_hip.h, uav_resize_aa_f32 — the
// filter of F.interpolate(mode='bicubic', antialias=True), with sample positions from integer arithmetic.
//
// Three launches on the caller's stream, no atomics:
//   set-up      one thread per result column and per result row: first tap, tap count and the normalised fp32 weights of that
//               sample, tabulated tap-major ([tap][n_out]) in the workspace.  Positions are exact: the argument of a tap is one
//               int64 quotient, divided in fp64 and rounded to fp32 once.
//   horizontal  (planes, hi, wi) -> (planes, hi, wo) in the workspace.  A block owns RA_SEG result columns of RA_ROWS rows and
//               stages the source span of its columns through LDS in chunks of RA_CHUNK samples (contiguous 16-byte loads when
//               wi % 4 == 0 and src is 16-byte aligned, 4-byte ones otherwise); a thread owns one column and walks its taps in
//               ascending order over the chunks.  Up to wi / wo = 4 - the program's range - the span is one chunk.
//   vertical    (planes, hi, wo) -> (planes, ho, wo).  A thread owns 4 adjacent columns (16 bytes per lane when wo % 4 == 0 and
//               both pointers are 16-byte aligned, else one column) of RA_VROWS adjacent result rows and walks the union of their
//               source rows once, ascending; taps and weights are uniform over the block (scalar loads).
// Every result sample is one fp32 accumulator fed by fmaf(weight, sample, acc) in ascending source index, in both access modes.
// HBM traffic: 4 * (hi*wi + 2*hi*wo + ho*wo) bytes per plane plus the tables; the vertical pass re-reads a source row for the
// (4s + RA_VROWS - 1) / RA_VROWS row groups that share it (s = hi / ho), which neighbouring blocks find in L2.
#include <type_traits>
#include "uav_common.h"

namespace {

constexpr int RA_SEG = 256;        // result columns per block of the horizontal pass = threads per block
constexpr int RA_ROWS = 4;         // rows per block of the horizontal pass
constexpr int RA_CHUNK = 1088;     // source samples per row staged at a time: 256 * 4 + 16 taps of margin + alignment, % 4 == 0
constexpr int RA_VROWS = 4;        // result rows per thread of the vertical pass
constexpr long long RA_MAX_RATIO = 64;

// Keys cubic, A = -0.5
UAV_DEVINL float ra_cubic(float x) {
    const float A = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return A * (((x - 5.0f) * x + 8.0f) * x - 4.0f);
    return 0.0f;
}

__host__ __device__ inline long long ra_floordiv(long long a, long long b) {      // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// most taps of one result sample of an axis: ceil(4 * n_in / n_out) when shrinking, 4 otherwise, never more than n_in
inline int ra_max_taps(long long n_in, long long n_out) {
    const long long k = n_in >= n_out ? (4 * n_in + n_out - 1) / n_out : 4;
    return (int)(k < n_in ? k : n_in);
}

struct RaAxis { int n_in, n_out, taps; float* w; int* lo; int* cnt; };

struct RaLayout { long long tmp, wx, wy, lox, cntx, loy, cnty, total; int kx, ky; };       // byte offsets into the workspace
inline long long ra_up16(long long v) { return (v + 15) & ~15ll; }
inline RaLayout ra_layout(long long planes, long long hi, long long wi, long long ho, long long wo) {
    RaLayout l;
    l.kx = ra_max_taps(wi, wo); l.ky = ra_max_taps(hi, ho);
    l.tmp = 0;
    l.wx = ra_up16(planes * hi * wo * 4);
    l.wy = l.wx + ra_up16((long long)l.kx * wo * 4);
    l.lox = l.wy + ra_up16((long long)l.ky * ho * 4);
    l.cntx = l.lox + ra_up16(wo * 4);
    l.loy = l.cntx + ra_up16(wo * 4);
    l.cnty = l.loy + ra_up16(ho * 4);
    l.total = l.cnty + ra_up16(ho * 4);
    return l;
}

__global__ __launch_bounds__(256) void resize_aa_setup_kernel(RaAxis ax, RaAxis ay) {
    int i = blockIdx.x * 256 + threadIdx.x;
    RaAxis a = ax;
    if (i >= ax.n_out) { i -= ax.n_out; a = ay; }
    if (i >= a.n_out) return;
    const long long n_in = a.n_in, n_out = a.n_out;
    const bool shrink = n_in >= n_out;
    const long long c2 = (2ll * i + 1) * n_in;                                  // centre c = c2 / (2 n_out)
    const long long sup = shrink ? 4 * n_in : 4 * n_out;                        // 2 * support * n_out
    long long lo = ra_floordiv(c2 - sup + n_out, 2 * n_out), hi = ra_floordiv(c2 + sup + n_out, 2 * n_out);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    int cnt = (int)(hi - lo);
    cnt = cnt > a.taps ? a.taps : cnt;                                          // (never: ra_max_taps is the bound)
    const double den = (double)(2 * (shrink ? n_in : n_out));
    float sum = 0.0f;
    for (int t = 0; t < cnt; ++t) sum += ra_cubic((float)((double)((2 * (lo + t) + 1) * n_out - c2) / den));
    for (int t = 0; t < a.taps; ++t) {
        const float k = t < cnt ? ra_cubic((float)((double)((2 * (lo + t) + 1) * n_out - c2) / den)) : 0.0f;
        a.w[(long long)t * n_out + i] = t < cnt ? k / sum : 0.0f;
    }
    a.lo[i] = (int)lo;
    a.cnt[i] = cnt;
}

template <bool VEC>
__global__ __launch_bounds__(256) void resize_aa_h_kernel(const float* __restrict__ src, float* __restrict__ tmp, int hi, int wi, int wo,
                                                          const float* __restrict__ wt, const int* __restrict__ lo,
                                                          const int* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) float tile[RA_ROWS][RA_CHUNK];
    const int tid = threadIdx.x, xb = blockIdx.y * RA_SEG, x = xb + tid;
    const int xl = min(xb + RA_SEG, wo) - 1;                                    // the block's last column
    const int y0 = blockIdx.x * RA_ROWS, rows = min(RA_ROWS, hi - y0);
    const bool live = x < wo;
    const int my_lo = live ? lo[x] : 0, my_hi = live ? my_lo + cnt[x] : 0;
    // first taps and ends grow with the column: the block's span is [first tap of its first column, end of its last one)
    const int span0 = VEC ? lo[xb] & ~3 : lo[xb], span1 = lo[xl] + cnt[xl];
    const float* p = src + ((long long)blockIdx.z * hi + y0) * wi;
    float acc[RA_ROWS];
#pragma unroll
    for (int r = 0; r < RA_ROWS; ++r) acc[r] = 0.0f;
    for (int c0 = span0; c0 < span1; c0 += RA_CHUNK) {
        const int c1 = min(c0 + RA_CHUNK, span1), len = c1 - c0;
        if (c0 != span0) __syncthreads();                                       // the chunk before is consumed
#pragma unroll
        for (int r = 0; r < RA_ROWS; ++r) {
            if (r >= rows) break;
            const float* row = p + (long long)r * wi + c0;
            if (VEC) {      // c0 % 4 == 0 and wi % 4 == 0: the last group of 4 ends at or before the row's end
                for (int k = tid * 4; k < len; k += 1024) *reinterpret_cast<float4_t*>(&tile[r][k]) = *reinterpret_cast<const float4_t*>(row + k);
            } else {
                for (int k = tid; k < len; k += 256) tile[r][k] = row[k];
            }
        }
        __syncthreads();
        const int j0 = max(my_lo, c0), j1 = min(my_hi, c1);
        for (int j = j0; j < j1; ++j) {
            const float w = wt[(long long)(j - my_lo) * wo + x];
#pragma unroll
            for (int r = 0; r < RA_ROWS; ++r) acc[r] = __builtin_fmaf(w, tile[r][j - c0], acc[r]);
        }
    }
    if (!live) return;
    float* o = tmp + ((long long)blockIdx.z * hi + y0) * wo + x;
#pragma unroll
    for (int r = 0; r < RA_ROWS; ++r)
        if (r < rows) o[(long long)r * wo] = acc[r];
}

// The horizontal pass for wi <= 4 wo, the program's range: at most RA_FTAPS taps per column and a span of at most RA_CHUNK samples
// per block, so a thread keeps its column's weights in registers (statically indexed: every tap of the unrolled loop is predicated,
// and the table is zero-padded to `taps` entries) and a block streams `groups` row groups of RA_ROWS rows through one LDS tile: the
// global loads of the next group are in flight, in registers, while the current one is computed.  Same taps, same order, same fmaf
// as resize_aa_h_kernel: the same bits.
constexpr int RA_FTAPS = 16;
template <bool VEC>
__global__ __launch_bounds__(256) void resize_aa_h4_kernel(const float* __restrict__ src, float* __restrict__ tmp, int hi, int wi, int wo,
                                                           int taps, int groups, const float* __restrict__ wt, const int* __restrict__ lo,
                                                           const int* __restrict__ cnt) {
    typedef typename std::conditional<VEC, float4_t, float>::type V;
    constexpr int N = VEC ? 4 : 1, NQ = (RA_CHUNK + 256 * N - 1) / (256 * N);   // loads of one thread per row: 2 of 16 bytes, or 5 of 4
    __shared__ __attribute__((aligned(16))) float tile[RA_ROWS][RA_CHUNK];
    const int tid = threadIdx.x, xb = blockIdx.y * RA_SEG, x = xb + tid;
    const int xl = min(xb + RA_SEG, wo) - 1;
    const bool live = x < wo;
    const int my_cnt = live ? cnt[x] : 0;
    const int span0 = VEC ? lo[xb] & ~3 : lo[xb], len = min(lo[xl] + cnt[xl] - span0, RA_CHUNK);      // (255 s + 1 + 16 + 3 <= 1040: never clipped)
    const int off = (live ? lo[x] : span0) - span0;
    float w[RA_FTAPS];
#pragma unroll
    for (int t = 0; t < RA_FTAPS; ++t) w[t] = (t < taps && live) ? wt[(long long)t * wo + x] : 0.0f;
    const int g0 = blockIdx.x * groups, g1 = min(g0 + groups, (hi + RA_ROWS - 1) / RA_ROWS);
    const float* plane = src + (long long)blockIdx.z * hi * wi + span0;
    V regs[RA_ROWS][NQ];
    const auto fetch = [&](int g) {
#pragma unroll
        for (int r = 0; r < RA_ROWS; ++r) {
            const int y = g * RA_ROWS + r;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = (q * 256 + tid) * N;      // VEC: span0 % 4 == 0 and wi % 4 == 0, a group of 4 ends at or before the row's end
                if (y < hi && k < len) regs[r][q] = *reinterpret_cast<const V*>(plane + (long long)y * wi + k);
                else regs[r][q] = V(0.0f);
            }
        }
    };
    fetch(g0);
    for (int g = g0; g < g1; ++g) {
#pragma unroll
        for (int r = 0; r < RA_ROWS; ++r) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int k = (q * 256 + tid) * N;
                if (k < len) *reinterpret_cast<V*>(&tile[r][k]) = regs[r][q];
            }
        }
        __syncthreads();
        if (g + 1 < g1) fetch(g + 1);
        float acc[RA_ROWS];
#pragma unroll
        for (int r = 0; r < RA_ROWS; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < RA_FTAPS; ++t) {
            if (t < taps && t < my_cnt) {
#pragma unroll
                for (int r = 0; r < RA_ROWS; ++r) acc[r] = __builtin_fmaf(w[t], tile[r][off + t], acc[r]);
            }
        }
        const int y0 = g * RA_ROWS;
        if (live) {
            float* o = tmp + ((long long)blockIdx.z * hi + y0) * wo + x;
#pragma unroll
            for (int r = 0; r < RA_ROWS; ++r)
                if (y0 + r < hi) o[(long long)r * wo] = acc[r];
        }
        __syncthreads();                                                        // the tile is consumed
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void resize_aa_v_kernel(const float* __restrict__ tmp, float* __restrict__ dst, int hi, int ho, int wo,
                                                          const float* __restrict__ wt, const int* __restrict__ lo,
                                                          const int* __restrict__ cnt) {
    constexpr int N = VEC ? 4 : 1;
    typedef typename std::conditional<VEC, float4_t, float>::type V;
    const long long x = ((long long)blockIdx.x * 256 + threadIdx.x) * N;
    if (x >= wo) return;
    const int y0 = blockIdx.y * RA_VROWS;
    int rlo[RA_VROWS], rhi[RA_VROWS];
    int j1 = 0;
#pragma unroll
    for (int r = 0; r < RA_VROWS; ++r) {
        const bool ok = y0 + r < ho;
        rlo[r] = ok ? lo[y0 + r] : 0;
        rhi[r] = ok ? rlo[r] + cnt[y0 + r] : 0;
        j1 = max(j1, rhi[r]);
    }
    const float* p = tmp + (long long)blockIdx.z * hi * wo + x;
    V acc[RA_VROWS];
#pragma unroll
    for (int r = 0; r < RA_VROWS; ++r) acc[r] = V(0.0f);
    for (int j = rlo[0]; j < j1; ++j) {                                          // first taps grow with the row: rlo[0] is the least
        const V v = *reinterpret_cast<const V*>(p + (long long)j * wo);
#pragma unroll
        for (int r = 0; r < RA_VROWS; ++r) {
            if (j >= rlo[r] && j < rhi[r]) {                                    // the same in every lane
                const float w = wt[(long long)(j - rlo[r]) * ho + y0 + r];
                if constexpr (VEC) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[r][q] = __builtin_fmaf(w, v[q], acc[r][q]);
                } else {
                    acc[r] = __builtin_fmaf(w, v, acc[r]);
                }
            }
        }
    }
    float* o = dst + ((long long)blockIdx.z * ho + y0) * wo + x;
#pragma unroll
    for (int r = 0; r < RA_VROWS; ++r)
        if (y0 + r < ho) *reinterpret_cast<V*>(o + (long long)r * wo) = acc[r];
}

inline bool ra_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// UAV_ESHAPE unless the kernels take the shape
inline int ra_shape_ok(int32_t planes, int32_t hi, int32_t wi, int32_t ho, int32_t wo) {
    if (planes < 1 || planes > 65535 || hi < 1 || wi < 1 || ho < 1 || wo < 1) return UAV_ESHAPE;
    if (hi > RA_MAX_RATIO * ho || wi > RA_MAX_RATIO * wo) return UAV_ESHAPE;
    // grid limits: row groups on y (65535), 2^31 - 1 blocks on x
    if ((wo + RA_SEG - 1) / RA_SEG > 65535 || (ho + RA_VROWS - 1) / RA_VROWS > 65535) return UAV_ESHAPE;
    if ((long long)wo + ho >= (1ll << 31)) return UAV_ESHAPE;
    return 0;
}

}  // namespace

extern "C" int64_t uav_resize_aa_workspace_bytes(int32_t planes, int32_t hi, int32_t wi, int32_t ho, int32_t wo) {
    if (ra_shape_ok(planes, hi, wi, ho, wo) != 0) return UAV_ESHAPE;
    return ra_layout(planes, hi, wi, ho, wo).total;
}

extern "C" int uav_resize_aa_f32(const float* src, float* dst, int32_t planes, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
    if (!src || !dst || !workspace) return UAV_EINVAL;
    if (!ra_aligned(src, 4) || !ra_aligned(dst, 4) || !ra_aligned(workspace, 4)) return UAV_EALIGN;
    if (ra_shape_ok(planes, hi, wi, ho, wo) != 0) return UAV_ESHAPE;
    const RaLayout l = ra_layout(planes, hi, wi, ho, wo);
    if (workspace_bytes < l.total) return UAV_ESHAPE;
    char* ws = (char*)workspace;
    float* tmp = (float*)(ws + l.tmp);
    const RaAxis ax = {wi, wo, l.kx, (float*)(ws + l.wx), (int*)(ws + l.lox), (int*)(ws + l.cntx)};
    const RaAxis ay = {hi, ho, l.ky, (float*)(ws + l.wy), (int*)(ws + l.loy), (int*)(ws + l.cnty)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(resize_aa_setup_kernel, dim3((unsigned)(((long long)wo + ho + 255) / 256)), dim3(256), 0, s, ax, ay);
    const bool hvec = wi % 4 == 0 && ra_aligned(src, 16);
    const unsigned segs = (unsigned)((wo + RA_SEG - 1) / RA_SEG), row_groups = (unsigned)((hi + RA_ROWS - 1) / RA_ROWS);
    if ((long long)wi <= 4ll * wo) {
        // row groups per block: 4, fewer while that leaves under 2048 blocks (8 per CU)
        unsigned groups = 4;
        while (groups > 1 && (unsigned long long)((row_groups + groups - 1) / groups) * segs * planes < 2048) groups /= 2;
        const dim3 gh((row_groups + groups - 1) / groups, segs, (unsigned)planes);
        if (hvec)
            hipLaunchKernelGGL(resize_aa_h4_kernel<true>, gh, dim3(256), 0, s, src, tmp, hi, wi, wo, l.kx, (int)groups, ax.w, ax.lo, ax.cnt);
        else
            hipLaunchKernelGGL(resize_aa_h4_kernel<false>, gh, dim3(256), 0, s, src, tmp, hi, wi, wo, l.kx, (int)groups, ax.w, ax.lo, ax.cnt);
    } else {
        const dim3 gh(row_groups, segs, (unsigned)planes);
        if (hvec)
            hipLaunchKernelGGL(resize_aa_h_kernel<true>, gh, dim3(256), 0, s, src, tmp, hi, wi, wo, ax.w, ax.lo, ax.cnt);
        else
            hipLaunchKernelGGL(resize_aa_h_kernel<false>, gh, dim3(256), 0, s, src, tmp, hi, wi, wo, ax.w, ax.lo, ax.cnt);
    }
    const unsigned rg = (unsigned)((ho + RA_VROWS - 1) / RA_VROWS);
    if (wo % 4 == 0 && ra_aligned(tmp, 16) && ra_aligned(dst, 16))
        hipLaunchKernelGGL(resize_aa_v_kernel<true>, dim3((unsigned)((wo / 4 + 255) / 256), rg, (unsigned)planes), dim3(256), 0, s, tmp, dst,
                           hi, ho, wo, ay.w, ay.lo, ay.cnt);
    else
        hipLaunchKernelGGL(resize_aa_v_kernel<false>, dim3((unsigned)((wo + 255) / 256), rg, (unsigned)planes), dim3(256), 0, s, tmp, dst,
                           hi, ho, wo, ay.w, ay.lo, ay.cnt);
    return uav_launch_status();
}
