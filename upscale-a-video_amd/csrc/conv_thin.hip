// Thin output-channel convolution: stride-1 (1,k,k) convs with n <= 16 output channels (UNet conv_out 256 -> 4, decoder conv_out
// 128 -> 3(4)).  The 128 x 128 tile kernel pads n to 128 columns and so multiplies 32x more than the result needs; here the GEMM N
// axis is ONE 16-wide MFMA tile (v_mfma_f32_16x16x32_f16: the real channels plus zero columns) and the launch is bound by reading its
// input rows, which is the floor of the layer.
//
// A 256-thread workgroup owns an 8 x 32 patch of output pixels of one image.  Per 64-channel chunk of the input it stages the haloed
// patch ((8 + k - 1) x (32 + k - 1) pixels x 128 B, every input row ONCE per workgroup — the taps then re-read LDS, not L2) and the
// weights of the chunk (k*k taps x 16 columns x 128 B; columns >= n are zeros).  62 KB for 3x3, so two workgroups share a CU and one
// computes while the other loads; inside a workgroup the next chunk travels global -> registers while the current one is multiplied.
// Pixels outside the image are staged as zeros, so border taps need no test in the loop.
//
// LDS rows are 128 B = 8 pieces of 16 B; piece s of row r holds channels 8 * (s ^ ((r >> 1) & 7)) .. + 7 of the chunk: the sixteen
// lanes of an MFMA operand read (consecutive rows, same logical piece) then fall into sixteen different 16-B columns of the 256-B bank
// line.  Writes are lane-linear.
//
// MFMA operands (swapped like the other conv kernels, so that a lane owns one pixel and four consecutive channels): A = weights
// (row = output channel = lane & 15, k = 8 * (lane >> 4) + j), B = pixels (column = pixel = lane & 15, same k), D: column = pixel,
// row = channel = 4 * (lane >> 4) + register.  A wave owns two patch rows = four 16-pixel groups and reuses each weight fragment for
// all four.  fp32 accumulation over the whole K; epilogue (acc + bias) * out_scale, 16-B (fp32) / 8-B (fp16) stores.
#include "conv_common.h"

namespace {
constexpr int TPH = 8, TPW = 32;          // output patch of a workgroup (4 waves x 2 rows x 32 pixels)

template <int KS, bool OF32>
__global__ __launch_bounds__(256, 2) void conv_thin_kernel(ConvArgs p, unsigned tiles_x, unsigned tiles_y) {
    constexpr int HH = TPH + KS - 1, HW = TPW + KS - 1, NPIX = HH * HW;
    constexpr int XPIECES = NPIX * 8, NX = (XPIECES + 255) / 256;       // 16-B pieces of the haloed patch, per thread
    constexpr int WROWS = KS * KS * 16;
    constexpr int WPIECES = WROWS * 8, NWL = (WPIECES + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sX = smem;
    char* sW = smem + NPIX * 128;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, r = lane & 15;

    const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);             // neighbouring patches (shared halo) on one XCD's L2
    const unsigned per_img = tiles_x * tiles_y;
    const unsigned img = bid / per_img, rem = bid - img * per_img;
    const unsigned ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = (int)ty * TPH, x0 = (int)tx * TPW;

    // ---- staging role of this thread: element offsets of its pieces inside the image / the weight matrix (-1: zeros) ----
    const half_t* xim = (const half_t*)p.a1 + (long long)img * p.hi * p.wi * p.c1;
    const half_t* wbase = (const half_t*)p.w;
    int xoff[NX], woff[NWL];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        const int idx = tid + i * 256;
        const int hp = idx >> 3, s = idx & 7;
        const int c = s ^ ((hp >> 1) & 7);
        const int hy = hp / HW, hx = hp - hy * HW;
        const int yy = y0 - p.pad_h + hy, xx = x0 - p.pad_w + hx;
        const bool ok = (idx < XPIECES) & ((unsigned)yy < (unsigned)p.hi) & ((unsigned)xx < (unsigned)p.wi);
        xoff[i] = ok ? (yy * p.wi + xx) * p.c1 + c * 8 : -1;
    }
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
        const int idx = tid + i * 256;
        const int rw = idx >> 3, s = idx & 7;
        const int c = s ^ ((rw >> 1) & 7);
        const int tap = rw >> 4, n = rw & 15;
        const bool ok = (idx < WPIECES) & (n < p.n);
        woff[i] = ok ? n * p.k_pad + tap * p.c1 + c * 8 : -1;
    }
    uint4_t px[NX], pw[NWL];
    const uint4_t zero4 = {0u, 0u, 0u, 0u};
#define THIN_FETCH(KC)                                                                                     \
    {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < NX; ++i)                                                     \
            px[i] = xoff[i] >= 0 ? *(const uint4_t*)(xim + xoff[i] + (KC)) : zero4;                        \
        _Pragma("unroll") for (int i = 0; i < NWL; ++i)                                                    \
            pw[i] = woff[i] >= 0 ? *(const uint4_t*)(wbase + woff[i] + (KC)) : zero4;                      \
    }

    float4_t acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = float4_t{0.f, 0.f, 0.f, 0.f};

    const int nchunk = p.c1 >> 6;
    THIN_FETCH(0)
    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch) __syncthreads();                     // every wave is done reading the previous chunk
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int idx = tid + i * 256;
            if (idx < XPIECES) *(uint4_t*)(sX + idx * 16) = px[i];
        }
#pragma unroll
        for (int i = 0; i < NWL; ++i) {
            const int idx = tid + i * 256;
            if (idx < WPIECES) *(uint4_t*)(sW + idx * 16) = pw[i];
        }
        __syncthreads();
        if (ch + 1 < nchunk) THIN_FETCH((ch + 1) * 64)     // in flight during the multiply below
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const int rw = (dy * KS + dx) * 16 + r;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int c = kk * 4 + q;
                    const half8_t wf = *(const half8_t*)(sW + rw * 128 + ((c ^ ((rw >> 1) & 7)) << 4));
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int hp = (wave * 2 + (g >> 1) + dy) * HW + (g & 1) * 16 + r + dx;
                        const half8_t xf = *(const half8_t*)(sX + hp * 128 + ((c ^ ((hp >> 1) & 7)) << 4));
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf, acc[g], 0, 0, 0);
                    }
                }
            }
        }
    }
#undef THIN_FETCH

    // ---- epilogue: this lane owns channels 4q .. 4q+3 of one pixel per group ----
    const int n0 = q * 4;
    if (n0 >= p.n) return;                           // zero columns (n % 4 == 0: a quad is real or padding as a whole)
    float4_t b = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) b = *(const float4_t*)(p.bias + n0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int y = y0 + wave * 2 + (g >> 1), x = x0 + (g & 1) * 16 + r;
        if (y >= p.ho || x >= p.wo) continue;
        const long long m = ((long long)img * p.ho + y) * p.wo + x;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (acc[g][j] + b[j]) * p.out_scale;
        if (OF32) {
            float4_t o = {v[0], v[1], v[2], v[3]};
            *(float4_t*)(p.out + (m * p.out_stride + n0) * 4) = o;
        } else {
            half4_t o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *(half4_t*)(p.out + (m * p.out_stride + n0) * 2) = o;
        }
    }
}

template <int KS>
int thin_launch(const ConvArgs& a, hipStream_t s) {
    const long long tiles_x = (a.wo + TPW - 1) / TPW, tiles_y = (a.ho + TPH - 1) / TPH;
    const long long grid = tiles_x * tiles_y * a.n_img;
    if (grid <= 0 || grid >= (1ll << 31)) return UAV_ESHAPE;
    constexpr int lds = ((TPH + KS - 1) * (TPW + KS - 1) + KS * KS * 16) * 128;
    static_assert(lds <= 64 * 1024, "two workgroups per CU");
    if (a.flags & UAV_CONV_OUT_F32)
        hipLaunchKernelGGL((conv_thin_kernel<KS, true>), dim3((unsigned)grid), dim3(256), lds, s, a, (unsigned)tiles_x, (unsigned)tiles_y);
    else
        hipLaunchKernelGGL((conv_thin_kernel<KS, false>), dim3((unsigned)grid), dim3(256), lds, s, a, (unsigned)tiles_x, (unsigned)tiles_y);
    return uav_launch_status();
}
}  // namespace

// Instances: 1x1 and 3x3 (conv_thin_ok in conv_gemm.hip admits nothing else).
int conv_launch_thin(const ConvArgs& a, hipStream_t s) {
    if (a.kh == 3 && a.kw == 3) return thin_launch<3>(a, s);
    if (a.kh == 1 && a.kw == 1) return thin_launch<1>(a, s);
    return UAV_ESHAPE;
}
