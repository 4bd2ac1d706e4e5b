"""float64 references of the small fp32 kernels — colour fix (csrc/colorfix.hip, K12), the non-GEMM kernels of RAFT (csrc/raft.hip,
K11b) and the scheduler kernels of csrc/elementwise.hip — with the cases and the pass marks of their edge-shape tests.

One `<kernel>_ref` per kernel, written in numpy float64 from the operation's definition (the reference's color_correction.py, ATen's
upsample_bicubic2d / upsample_bilinear2d / grid_sample / avg_pool2d, RAFT's upsample_flow, the DDIM formulas), and one
`check_<kernel>(impl, case)` that runs `impl` — a callable with the op's signature on CPU tensors: the GPU kernel behind a thin adapter
in tests/test_small_kernels_gpu.py, the rounded reference or a deliberately wrong variant in tests/test_small_kernels_cpu.py — on the
case's inputs and holds every output element against the reference.  A check returns Result(kernel, case, err, bar) of the element
closest to (or furthest over) its bar — its `parts` hold the Result of every tensor compared, for the record
(profiles/small_kernels_edge_parity.txt) — and raises AssertionError with the same figures when one is over.

Pass marks.  u = 2^-24 is the unit roundoff of fp32.  A mark that follows from counting roundings is stated at the check; where the
error depends on a library function or on polynomial weights (bicubic weights, rsqrtf, expf, tanhf, positions formed in fp32) it is
measured against the float64 reference, never against the kernel: 4 x the largest error of torch's own fp32 CPU op on the same inputs
(the factor covers another summation order and the device's math functions), and at least 2^-22 x the output's magnitude (so that a
case where torch happens to be exact sets no impossible mark)."""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
Result = collections.namedtuple("Result", "kernel case err bar parts", defaults=((),))


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
def f64(t):
    """tensor / array -> numpy float64"""
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def t32(a):
    """float64 array -> fp32 CPU tensor (one rounding)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32)))


def ulp32(a):
    return np.spacing(np.abs(f64(a)).astype(np.float32)).astype(np.float64)


def ulp16(a):
    return np.spacing(np.abs(f64(a)).astype(np.float16)).astype(np.float64)


def judge(kernel, case, got, ref, bar):
    """Every element of `got` within `bar` (scalar or per element; 0 = bit-exact value) of `ref`."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, f"{kernel} {case}: shape {got.shape}, expected {ref.shape}"
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), ref.shape)
    d = np.abs(got - ref)
    d = np.where(np.isfinite(got), d, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, d / np.where(bar > 0, bar, 1.0), np.where(d == 0, 0.0, np.inf))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    res = Result(kernel, str(case), float(d[i]), float(bar[i]))
    if not ratio[i] <= 1.0:
        raise AssertionError(f"{kernel} {case}: error {res.err:.3e} over the bar {res.bar:.3e} at element {i} "
                             f"(got {got[i]!r}, reference {ref[i]!r}); {int((ratio > 1).sum())} of {ratio.size} elements over")
    return res


def worst(results):
    """The result closest to its bar, carrying all of them as its parts."""
    w = max(results, key=lambda r: (r.err / r.bar) if r.bar > 0 else (0.0 if r.err == 0 else math.inf))
    return w._replace(parts=tuple(results))


def measured_bar(torch_fp32, ref, magnitude=None):
    """4 x the largest error of torch's fp32 CPU op against the float64 reference, at least 2^-22 x the output's magnitude."""
    ref = f64(ref)
    mag = float(np.abs(ref).max()) if magnitude is None else float(magnitude)
    return max(4.0 * float(np.abs(f64(torch_fp32) - ref).max()), 2.0 ** -22 * mag)


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def randn32(g, *shape, scale=1.0, shift=0.0):
    return (g.standard_normal(shape) * scale + shift).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# colour fix: uav_plane_stats_f32
# (kind, planes, hw).  "int": position-dependent integers in [-8, 8] — every sum is exact in fp32 and fp64, so the result is defined
# to the last bit and one dropped or double-counted element moves the sum by >= 1.  The kernel cuts a plane into 64 chunks of
# ceil(hw / 64) elements; 256 threads read a chunk 8 x 256 elements at a time.
PLANE_STATS_CASES = [
    ("int", 1, 1),                    # hw = 1: variance 0 by definition of the kernel (torch: nan); 63 empty chunks
    ("int", 3, 63),                   # fewer elements than chunks: chunks 63.. start past the end
    ("int", 5, 7681),                 # odd hw, planes at odd offsets; last chunk 58 elements short
    ("int", 2, 64 * 256 + 1),         # per-chunk length 257: thread 0 alone takes a second element; last chunk holds 194
    ("int", 70, 300),                 # planes 64.. are the second block of the finalize kernel
    ("int", 1, 1031 * 1021),          # per-chunk length 16 448 = 8 x 2048 + 64: nine rounds, the last 64 threads wide
    ("uniform", 2, 96 * 80),          # uniform [-1, 1]
    ("nearconst", 2, 96 * 80),        # 0.8 +- 1e-3: variance 3e-7 from sums of 0.64
    ("const", 2, 96 * 80),            # exactly constant planes (0.8 and 0.1, whose squares are not fp32 numbers): variance 0
]
STATS_EPS = 1e-5                      # the eps AdaIN adds to the variance (color_correction.py:54)


def plane_stats_input(case):
    kind, planes, hw = case
    if kind == "int":
        i = np.arange(hw, dtype=np.int64)[None, :]
        p = np.arange(planes, dtype=np.int64)[:, None]
        return (((i * 5 + (i // 17) * 3 + p * 7) % 17) - 8).astype(np.float32)
    g = rng(12, planes, hw, len(kind))
    if kind == "uniform":
        return g.uniform(-1, 1, (planes, hw)).astype(np.float32)
    if kind == "nearconst":
        return (0.8 + g.uniform(-1e-3, 1e-3, (planes, hw))).astype(np.float32)
    return np.repeat(np.array([[0.8], [0.1]], dtype=np.float32)[:planes], hw, axis=1)


def plane_stats_ref(x):
    """Per-plane mean and UNBIASED variance (torch.var's default, calc_mean_std) of (planes, hw); 0 for hw = 1."""
    x = f64(x)
    n = x.shape[1]
    mean = x.sum(axis=1) / n
    var = ((x - mean[:, None]) ** 2).sum(axis=1) / (n - 1) if n > 1 else np.zeros_like(mean)
    return mean, var


def check_plane_stats(impl, case):
    """impl(x (planes, hw) fp32) -> (mean, var) fp32 [planes].
    Integer data: mean within 1 fp32 ulp and variance within 2 ulp of the float64 values.  Other data: the mean by the measured rule
    (magnitude: max|x|, the size of the summands), and sqrt(var + 1e-5) — the quantity AdaIN divides by — RELATIVE to the reference,
    4 x the relative error of torch's fp32 `var` in the same quantity, at least 64 x 2^-24."""
    x = plane_stats_input(case)
    mean, var = impl(torch.from_numpy(x))
    rm, rv = plane_stats_ref(x)
    name = f"{case[0]} {case[1]}x{case[2]}"
    if case[0] == "int":
        return worst([judge("plane_stats_f32", name + " mean", mean, rm, ulp32(rm)),
                      judge("plane_stats_f32", name + " var", var, rv, np.where(rv > 0, 2 * ulp32(rv), 0.0))])
    xt = torch.from_numpy(x)
    bar_m = measured_bar(xt.mean(dim=1), rm, magnitude=np.abs(x).max())
    rs = np.sqrt(rv + STATS_EPS)
    ts = np.sqrt(f64(xt.var(dim=1)) + STATS_EPS)
    bar_s = max(4 * float(np.abs(ts / rs - 1).max()), 64 * U)
    gs = np.sqrt(np.maximum(f64(var), 0) + STATS_EPS)
    assert (f64(var) >= 0).all(), f"plane_stats_f32 {name}: negative variance {f64(var)}"
    return worst([judge("plane_stats_f32", name + " mean", mean, rm, bar_m),
                  judge("plane_stats_f32 sqrt(var+eps)", name + ", relative", gs / rs, np.ones_like(rs), bar_s)])


# ---------------------------------------------------------------------------------------------------------------------------------
# colour fix: uav_adain_apply_f32.  planes = 3 of hw elements; a thread owns 4 elements and takes the vector path when all 4 exist
# and the plane starts on a 16-byte boundary.
ADAIN_CASES = [
    1,          # one element: scalar tail only
    3,          # tail of 3; planes 1, 2 start misaligned
    4,          # exactly one vector per plane, every plane aligned
    5,          # vector + tail of 1 in plane 0; planes 1, 2 misaligned (base 5, 10)
    1023,       # one block, last thread has a tail of 3
    1024,       # exactly one full block
    1025,       # second x-block holding one scalar element
    7681,       # 8 blocks, odd planes misaligned
]
ADAIN_PLANES = 3


def adain_input(hw):
    g = rng(13, hw)
    x = randn32(g, ADAIN_PLANES, hw, scale=0.5, shift=0.1)
    cm = np.array([0.1, -0.2, 0.05], dtype=np.float32)
    cv = np.array([0.25, 0.01, 0.0], dtype=np.float32)          # plane 2: zero variance, the divisor is sqrt(eps)
    sm = np.array([0.3, 0.0, -0.45], dtype=np.float32)
    sv = np.array([0.04, 0.5, 0.09], dtype=np.float32)
    return x, cm, cv, sm, sv


def adain_ref(x, cm, cv, sm, sv, eps):
    """(x - cm) / sqrt(cv + eps) * sqrt(sv + eps) + sm per plane (color_correction.py:59-71)."""
    x, cm, cv, sm, sv = (f64(a) for a in (x, cm, cv, sm, sv))
    return (x - cm[:, None]) / np.sqrt(cv + eps)[:, None] * np.sqrt(sv + eps)[:, None] + sm[:, None]


def check_adain_apply(impl, hw):
    """impl(x (planes, hw), c_mean, c_var, s_mean, s_var, eps) -> out (planes, hw).  The statistics are the test's own numbers.
    Bar per element: 8 x 2^-24 x (|x - m| / cs * ss + |sm|) — the roundings of the subtraction, the two square roots of rounded
    sums, the division, the product and the final sum.  eps is the fp32 number the C ABI takes."""
    x, cm, cv, sm, sv = adain_input(hw)
    eps = float(np.float32(1e-5))
    out = impl(*(torch.from_numpy(a) for a in (x, cm, cv, sm, sv)), eps)
    ref = adain_ref(x, cm, cv, sm, sv, eps)
    bar = 8 * U * (np.abs(ref - f64(sm)[:, None]) + np.abs(f64(sm))[:, None])
    return judge("adain_apply_f32", f"3x{hw}", out, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# colour fix: uav_atrous_blur_f32.  (h, w, r), 2 planes; one thread per pixel, x-blocks of 256 columns.
ATROUS_CASES = [
    (1, 1, 1),          # every tap is the one pixel
    (1, 300, 2),        # one row: both vertical taps clamp; second x-block
    (5, 7, 16),         # r beyond both dimensions: all outer taps clamp to the borders
    (17, 16, 16),       # r == w: x + r = w clamps by one; y + r reaches the last row exactly for y = 0
    (40, 257, 1),       # a second x-block one column wide
    (33, 300, 8),       # interior, both borders and a second x-block at a middle dilation
]
ATROUS_PLANES = 2
WAVELET_SHAPE = (2, 3, 37, 300)


def atrous_input(case):
    h, w, r = case
    g = rng(14, h, w, r)
    return randn32(g, ATROUS_PLANES, h, w, scale=0.6), g.uniform(-1, 1, (ATROUS_PLANES, h, w)).astype(np.float32)


def atrous_blur_ref(x, r):
    """wavelet_blur (color_correction.py:73-91): replicate padding by r, then the 3x3 kernel [1 2 1]^T [1 2 1] / 16 with dilation r."""
    x = f64(x)
    h, w = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="edge")
    k = (0.25, 0.5, 0.25)
    out = np.zeros_like(x)
    for a in range(3):
        for b in range(3):
            out += k[a] * k[b] * p[..., a * r:a * r + h, b * r:b * r + w]
    return out


def check_atrous_blur(impl, case, preload):
    """impl(x (planes, h, w), r, high or None) -> (low, high or None); `high` accumulates x - low.
    The weights are powers of two, so only the 8 additions round: bar 16 x 2^-24 x max|x| (which also covers the subtraction and the
    accumulation into a preloaded `high` of at most that magnitude)."""
    x, hi0 = atrous_input(case)
    low, high = impl(torch.from_numpy(x), case[2], torch.from_numpy(hi0.copy()) if preload else None)
    ref = atrous_blur_ref(x, case[2])
    bar = 16 * U * float(np.abs(x).max())
    name = f"{case[0]}x{case[1]} r{case[2]}" + (" +high" if preload else "")
    res = [judge("atrous_blur_f32", name + " low", low, ref, bar)]
    if preload:
        res.append(judge("atrous_blur_f32", name + " high", high, f64(hi0) + (f64(x) - ref), bar))
    else:
        assert high is None
    return worst(res)


def wavelet_input():
    g = rng(15)
    return randn32(g, *WAVELET_SHAPE, scale=0.6), (g.uniform(0.1, 0.6, WAVELET_SHAPE)).astype(np.float32)


def wavelet_decomposition_ref(image, levels=5):
    """color_correction.py:93-106: high = sum_i (image_i - blur_{2^i}(image_i)), low = the last blur."""
    cur = f64(image)
    high = np.zeros_like(cur)
    for i in range(levels):
        low = atrous_blur_ref(cur, 2 ** i)
        high += cur - low
        cur = low
    return high, cur


def wavelet_reconstruction_ref(content, style):
    return wavelet_decomposition_ref(content)[0] + wavelet_decomposition_ref(style)[1]      # :108-118


def check_wavelet(impl):
    """impl = (decomposition, reconstruction): decomposition(image (B,C,H,W)) -> (high, low); reconstruction(content, style) -> image.
    Five levels: 5 x the one-level bar."""
    decomposition, reconstruction = impl
    content, style = wavelet_input()
    bar = 5 * 16 * U * float(max(np.abs(content).max(), np.abs(style).max()))
    high, low = decomposition(torch.from_numpy(content))
    rh, rl = wavelet_decomposition_ref(content)
    out = reconstruction(torch.from_numpy(content), torch.from_numpy(style))
    return worst([judge("wavelet_decomposition", "2x3x37x300 high", high, rh, bar),
                  judge("wavelet_decomposition", "2x3x37x300 low", low, rl, bar),
                  judge("wavelet_reconstruction", "2x3x37x300", out, wavelet_reconstruction_ref(content, style), bar)])


# ---------------------------------------------------------------------------------------------------------------------------------
# colour fix: uav_resize_bicubic_f32 at 4x (scale 1/4 given, as the CLI does).  (hi, wi), 2 planes.
BICUBIC_CASES = [
    (1, 1),             # all 16 taps clamp to the one pixel
    (1, 5),             # one row; columns clamp on both sides
    (2, 3),             # both row taps -1 and +2 clamp everywhere
    (3, 65),            # wo = 260: a second x-block of 4 columns
    (24, 20),           # interior rows and columns (the size of the golden fixture)
]
BICUBIC_PLANES = 2


def clamped(i, n):
    return min(max(i, 0), n - 1)


def cubic_weights(n_in, n_out, scale, a=-0.75, tap=clamped):
    """(n_out, n_in) matrix of ATen's upsample_bicubic2d (align_corners=False): source position scale * (dst + 0.5) - 0.5, the four
    cubic-convolution weights (A = -0.75) on taps floor - 1 .. floor + 2, each tap index clamped to the image (`tap`: the index rule,
    replaced by the wrong variants of tests/test_small_kernels_cpu.py)."""
    def near(t):
        return ((a + 2) * t - (a + 3)) * t * t + 1              # |t| <= 1
    def far(t):
        return ((a * t - 5 * a) * t + 8 * a) * t - 4 * a        # 1 < |t| < 2
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = scale * (o + 0.5) - 0.5
        fl = math.floor(src)
        t = src - fl
        for k, wk in enumerate((far(t + 1), near(t), near(1 - t), far(2 - t))):
            m[o, tap(fl - 1 + k, n_in)] += wk
    return m


def bicubic_ref(x, ho, wo, scale_h, scale_w):
    x = f64(x)
    return cubic_weights(x.shape[-2], ho, scale_h) @ x @ cubic_weights(x.shape[-1], wo, scale_w).T


def check_resize_bicubic(impl, case):
    """impl(x (planes, hi, wi), ho, wo, scale_h, scale_w) -> (planes, ho, wo).  Measured bar (the weights are cubic polynomials
    evaluated in fp32): F.interpolate(scale_factor=4, mode='bicubic') in fp32."""
    hi, wi = case
    x = randn32(rng(16, hi, wi), BICUBIC_PLANES, hi, wi, scale=0.7)
    out = impl(torch.from_numpy(x), 4 * hi, 4 * wi, 0.25, 0.25)
    ref = bicubic_ref(x, 4 * hi, 4 * wi, 0.25, 0.25)
    t = F.interpolate(torch.from_numpy(x)[None], scale_factor=4, mode="bicubic")[0]
    return judge("resize_bicubic_f32", f"{hi}x{wi} -> 4x", out, ref, measured_bar(t, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_instnorm_f32 on channels-last rows (n_img * hw, c); a workgroup owns 32 channels of one image, 8 row lanes each.
INSTNORM_CASES = [
    # (n_img, hw, c, data)
    (1, 1, 32, "randn"),        # one row: variance 0, output 0 (F.instance_norm refuses one spatial element)
    (2, 5, 40, "randn"),        # hw < 8 row lanes (lanes 5..7 idle), c % 32 != 0: the `ch < c` guard fires in the second slab
    (3, 300, 96, "randn"),      # the shape of tests/test_raft_gpu.py: 3 slabs, 37-38 rows per lane
    (1, 4099, 33, "randn"),     # odd hw, second slab holds one channel
    (3, 300, 96, "offset"),     # mean 50, std 0.1: the variance is lost unless the mean is removed first
]


def instnorm_input(case):
    n_img, hw, c, data = case
    g = rng(17, n_img, hw, c, len(data))
    if data == "offset":
        return randn32(g, n_img * hw, c, scale=0.1, shift=50.0)
    return randn32(g, n_img * hw, c, scale=2.0, shift=1.0)


def instnorm_ref(x, n_img, hw, relu, eps):
    """nn.InstanceNorm2d without affine (extractor.py:27-30): per image and channel, (x - mean) / sqrt(BIASED var + eps), then ReLU."""
    x = f64(x).reshape(n_img, hw, -1)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    y = (x - mean) / np.sqrt(var + eps)
    return (np.maximum(y, 0) if relu else y).reshape(n_img * hw, -1)


def check_instnorm(impl, case, relu):
    """impl(x rows, n_img, hw, relu, eps) -> rows.  Measured bar (rsqrtf, fp32 sums): F.instance_norm in fp32; hw = 1, which torch
    refuses, must give exactly 0."""
    n_img, hw, c, data = case
    x = instnorm_input(case)
    eps = float(np.float32(1e-5))
    out = impl(torch.from_numpy(x), n_img, hw, relu, eps)
    ref = instnorm_ref(x, n_img, hw, relu, eps)
    name = f"{n_img}x{hw}x{c} {data}" + (" relu" if relu else "")
    if hw == 1:
        return judge("instnorm_f32", name, out, ref, 0.0)
    t = F.instance_norm(torch.from_numpy(x).reshape(n_img, hw, c).permute(0, 2, 1), eps=1e-5).permute(0, 2, 1).reshape(-1, c)
    return judge("instnorm_f32", name, out, ref, measured_bar(F.relu(t) if relu else t, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: the elementwise kernels, one thread per element, blocks of 256
ELEMENTWISE_N = [1, 255, 256, 257, 77000]       # one thread; one short block; one full block; one element in a second block; 301 blocks
GRU_SHAPES = [(1, 1), (51, 5), (2, 128), (257, 1), (616, 125)]     # rows x c with rows * c = the sizes above


def check_add_relu(impl, n, relu):
    """impl(a, b, relu) -> a + b (ReLU).  One rounding of an exact float64 sum: bit-exact."""
    g = rng(18, n)
    a, b = randn32(g, n), randn32(g, n)
    s = f64(a) + f64(b)
    ref = f64(t32(np.maximum(s, 0) if relu else s))
    return judge("add_relu_f32", f"n={n}" + (" relu" if relu else ""), impl(torch.from_numpy(a), torch.from_numpy(b), relu), ref, 0.0)


def check_axpby(impl, n):
    """impl(x, z, a, b) -> a*x + b*z.  Two products and a sum, each rounded once (fewer with a fused multiply-add): at most
    1.5 ulp of the largest of |a x|, |b z| and the result; bar 2 ulp there."""
    g = rng(19, n)
    x, z = randn32(g, n), randn32(g, n)
    a, b = float(np.float32(0.7)), float(np.float32(-1.3))
    ax, bz = a * f64(x), b * f64(z)
    ref = ax + bz
    bar = 2 * ulp32(np.maximum(np.maximum(np.abs(ax), np.abs(bz)), np.abs(ref)))
    return judge("axpby_f32", f"n={n}", impl(torch.from_numpy(x), torch.from_numpy(z), a, b), ref, bar)


def gru_input(rows, c):
    g = rng(20, rows, c)
    return (g.uniform(0, 1, (rows, 2 * c)).astype(np.float32), randn32(g, rows, c), randn32(g, rows, c))


def gru_rh_ref(zr, h):
    c = h.shape[1]
    return f64(zr)[:, c:] * f64(h)                                   # update.py:48: r * h, r the second half of the z | r rows


def gru_blend_ref(zr, q, h):
    c = h.shape[1]
    z = f64(zr)[:, :c]
    return (1 - z) * f64(h) + z * f64(q)                             # update.py:50


def check_gru_rh(impl, shape):
    """impl(zr (rows, 2c), h (rows, c)) -> r * h.  One product, one rounding: bit-exact."""
    zr, h, _ = gru_input(*shape)
    ref = f64(t32(gru_rh_ref(zr, h)))
    return judge("gru_rh_f32", f"{shape[0]}x{shape[1]}", impl(torch.from_numpy(zr), torch.from_numpy(h)), ref, 0.0)


def check_gru_blend(impl, shape):
    """impl(zr, q, h) -> (1 - z) * h + z * q.  Bar: 2 ulp at |(1 - z) h| + |z q|, which bounds both products and the result."""
    zr, h, q = gru_input(*shape)
    c = shape[1]
    z = f64(zr)[:, :c]
    bar = 2 * ulp32(np.abs((1 - z) * f64(h)) + np.abs(z * f64(q)))
    out = impl(torch.from_numpy(zr), torch.from_numpy(q), torch.from_numpy(h.copy()))
    return judge("gru_blend_f32", f"{shape[0]}x{shape[1]}", out, gru_blend_ref(zr, q, h), bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_copy_cols_f32: dst[:, dcol:dcol+ncols] = act(src[:, scol:scol+ncols]) between row buffers of different strides
COPY_COLS_CASES = [
    # (src_stride, src_col, dst_stride, dst_col, ncols)
    (352, 3, 130, 126, 4),          # a window up to the last column of the destination; 4 columns: r = i / 4
    (128, 0, 384, 256, 128),        # whole source rows into the last third of wider rows
]
COPY_COLS_ROWS = [1, 300]
COPY_COLS_ACTS = [0, 1, 4]          # none, ReLU, tanh
DST_FILL = -77.25                   # what the destination holds before the call


def copy_cols_ref(src, scol, dst, dcol, ncols, act):
    v = f64(src)[:, scol:scol + ncols]
    v = np.maximum(v, 0) if act == 1 else np.tanh(v) if act == 4 else v
    out = f64(dst).copy()
    out[:, dcol:dcol + ncols] = v
    return out


def check_copy_cols(impl, case, rows, act):
    """impl(src (rows, sstride), scol, dst (rows, dstride), dcol, ncols, act) -> dst after the call, all columns.
    act 0 / 1: bit-exact; tanh: measured bar (torch.tanh in fp32).  Columns outside the window keep their bits."""
    ss, sc, ds, dc, nc = case
    src = randn32(rng(21, ss, rows, act), rows, ss, scale=1.5)
    dst = np.full((rows, ds), DST_FILL, dtype=np.float32)
    out = impl(torch.from_numpy(src), sc, torch.from_numpy(dst.copy()), dc, nc, act)
    ref = copy_cols_ref(src, sc, dst, dc, nc, act)
    bar = np.zeros_like(ref)
    if act == 4:
        full = np.full((rows, ds), DST_FILL, dtype=np.float32)
        full[:, dc:dc + nc] = torch.tanh(torch.from_numpy(src[:, sc:sc + nc])).numpy()
        bar[:, dc:dc + nc] = measured_bar(full[:, dc:dc + nc], ref[:, dc:dc + nc])
    return judge("copy_cols_f32", f"{ss}:{sc}->{ds}:{dc} x{nc} rows={rows} act={act}", out, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_avgpool2_f32 on P volumes of h x w at `src_stride` floats each
AVGPOOL_SHAPES = [(2, 2), (5, 4), (4, 5), (7, 9)]     # one output; odd h (last row dropped); odd w (last column dropped); both odd
AVGPOOL_PAD = [0, 3]                                  # src_stride = h * w, and h * w + 3
AVGPOOL_P = [1, 300]


def avgpool2_ref(src, src_stride, h, w, p_count):
    """F.avg_pool2d(2, stride 2) (corr.py:25): odd sizes floor, the last row / column is not read."""
    v = f64(src).reshape(p_count, src_stride)[:, :h * w].reshape(p_count, h, w)
    h2, w2 = h // 2, w // 2
    v = v[:, :2 * h2, :2 * w2].reshape(p_count, h2, 2, w2, 2)
    return v.mean(axis=(2, 4)).reshape(p_count, h2 * w2)


def check_avgpool2(impl, shape, pad, p_count):
    """impl(src (P, src_stride), src_stride, h, w, P) -> (P, (h/2) * (w/2)).  Three additions and an exact scaling:
    bar 3 x 2^-24 x the mean of the four magnitudes, whatever the order of the additions."""
    h, w = shape
    stride = h * w + pad
    src = randn32(rng(22, h, w, pad, p_count), p_count, stride)
    out = impl(torch.from_numpy(src), stride, h, w, p_count)
    bar = 3 * U * avgpool2_ref(np.abs(src), stride, h, w, p_count)
    return judge("avgpool2_f32", f"{h}x{w} stride={stride} P={p_count}", out, avgpool2_ref(src, stride, h, w, p_count), bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_resize_bilinear_f32 (align_corners=False), rows 0 and 1 of every plane scaled afterwards
BILINEAR_CASES = [
    # (hi, wi, ho, wo, row0_scale, row1_scale, planes)
    (1, 1, 3, 5, 1.0, 1.0, 2),              # one source pixel: both taps are that pixel
    (4, 6, 1, 1, 1.0, 1.0, 2),              # one output pixel at the centre (position 1.5, 2.5)
    (13, 17, 5, 4, 1.0, 1.0, 3),            # shrinking by non-integer factors
    (3, 3, 24, 24, 1.0, 1.0, 2),            # 8x: negative positions clamp to 0, positions past hi - 1 take the last row twice
    (7, 9, 7, 9, 1.0, 1.0, 2),              # equal sizes: must reproduce the input bit for bit
    (48, 56, 45, 52, 45 / 48, 52 / 56, 8),  # RAFT_bi's resize back, with the two row scales; 73 blocks
]


def linear_weights(n_in, n_out):
    """(n_out, n_in) matrix of ATen's upsample_bilinear2d (align_corners=False): position max(in/out * (dst + 0.5) - 0.5, 0), taps
    floor and floor + 1 (the last index twice at the far border)."""
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = max(n_in / n_out * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        lam = src - i0
        m[o, i0] += 1 - lam
        m[o, i1] += lam
    return m


def bilinear_ref(x, ho, wo, row0_scale=1.0, row1_scale=1.0):
    x = f64(x)
    out = linear_weights(x.shape[-2], ho) @ x @ linear_weights(x.shape[-1], wo).T
    out[..., 0, :] *= row0_scale                                        # raft_bi.py:11-16 scales ROWS 0 and 1 of both flow channels
    if ho > 1:
        out[..., 1, :] *= row1_scale
    return out


def check_resize_bilinear(impl, case):
    """impl(x (planes, hi, wi), ho, wo, row0_scale, row1_scale) -> (planes, ho, wo).  Measured bar (positions and weights are formed
    in fp32): F.interpolate(mode='bilinear') in fp32 with the rows scaled the same way; equal sizes: bit-exact.  The row scales are the
    fp32 numbers the C ABI takes."""
    hi, wi, ho, wo, r0, r1, planes = case
    x = randn32(rng(23, hi, wi, ho, wo), planes, hi, wi, scale=5.0)
    r0, r1 = float(np.float32(r0)), float(np.float32(r1))
    out = impl(torch.from_numpy(x), ho, wo, r0, r1)
    ref = bilinear_ref(x, ho, wo, r0, r1)
    name = f"{hi}x{wi} -> {ho}x{wo}"
    if (hi, wi) == (ho, wo):
        return judge("resize_bilinear_f32", name, out, f64(x), 0.0)
    t = F.interpolate(torch.from_numpy(x)[None], (ho, wo), mode="bilinear")[0]
    t[:, 0] *= r0
    if ho > 1:
        t[:, 1] *= r1
    return judge("resize_bilinear_f32", name, out, ref, measured_bar(t, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_corr_lookup_f32: per pixel a (2r+1)^2 window of bilinear samples in each of 4 correlation levels
LOOKUP_LEVELS = [(6, 7), (3, 3), (2, 1), (1, 1)]      # (h, w): the last two have a side of 1, where grid_sample's normalisation divides by 0
LOOKUP_CASES = [
    # (radius, out_stride, coord_stride, level strides beyond h * w)
    (4, 324, 2, 0),             # everything dense
    (4, 352, 4, 5),             # padded output rows (the GRU's 352-channel input), padded coordinates, padded levels
    (1, 36, 2, 5),
    (1, 40, 4, 0),
]
OUT_FILL = 1234.5


def lookup_coords():
    """(x, y) per pixel, in level-0 pixels; level l samples at x / 2^l."""
    w0 = LOOKUP_LEVELS[0][1]
    below = float(np.nextafter(np.float32(3.0), np.float32(0.0)))        # just below an integer: floor 2, weight 1 - 2^-22
    pts = [(0.0, 0.0), (2.0, 3.0), (6.0, 5.0),                            # exact integers, the last one the far corner
           (-1.0, -1.0), (-0.5, -0.5), (-0.5, 2.25),                      # on and inside the zero border; negative: floor, not truncation
           (w0 - 1.0, 1.5), (float(w0), 2.0), (w0 - 0.25, 5.75),          # last column; one past it; between the two
           (below, below), (below, 1.0), (1.3, 4.6), (3.75, 0.125),
           (1e4, 2.0), (-1e4, -1e4), (2.0, 1e4)]                          # far outside: every tap is zero padding
    return np.array(pts, dtype=np.float32)


def lookup_input(case):
    radius, ostride, cstride, lpad = case
    g = rng(24, radius, ostride, cstride, lpad)
    c = lookup_coords()
    p = c.shape[0]
    coords = np.full((p, cstride), 9e3, dtype=np.float32)               # padding columns hold a value that would show if read
    coords[:, :2] = c
    strides = [h * w + lpad for h, w in LOOKUP_LEVELS]
    levels = [randn32(g, p, s, scale=2.0) for s in strides]
    return levels, strides, coords


def corr_lookup_ref(levels, strides, hs, ws, coords, radius, floor=np.floor):
    """CorrBlock.__call__ (corr.py:29-50): out[p][l * win^2 + a * win + b] = sample of level l of pixel p at
    (x / 2^l + a - r, y / 2^l + b - r) — the FIRST window index moves x — where sample is F.grid_sample(align_corners=True,
    padding_mode='zeros') in pixel coordinates: bilinear, taps outside the image contribute 0."""
    coords = f64(coords)
    p, win = coords.shape[0], 2 * radius + 1
    out = np.zeros((p, 4 * win * win))
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    pi = np.arange(p)[:, None, None]
    for l in range(4):
        h, w = hs[l], ws[l]
        img = f64(levels[l]).reshape(p, strides[l])[:, :h * w].reshape(p, h, w)
        x = (coords[:, 0] / 2 ** l)[:, None, None] + d[None, :, None] + 0 * d[None, None, :]
        y = (coords[:, 1] / 2 ** l)[:, None, None] + d[None, None, :] + 0 * d[None, :, None]
        x0, y0 = floor(x), floor(y)
        acc = np.zeros_like(x)
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
                wgt = (1 - np.abs(x - (x0 + dx))) * (1 - np.abs(y - (y0 + dy)))
                ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                acc += np.where(ok, img[pi, np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)] * wgt, 0.0)
        out[:, l * win * win:(l + 1) * win * win] = acc.reshape(p, win * win)
    return out


def lookup_positions(coords, radius):
    """The exact sample positions (x, y) of every output column, (P, 4 * win^2) each."""
    coords = f64(coords)
    win = 2 * radius + 1
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    xs, ys = [], []
    for l in range(4):
        xs.append(np.repeat((coords[:, 0:1] / 2 ** l) + d[None, :], win, axis=1))
        ys.append(np.tile((coords[:, 1:2] / 2 ** l) + d[None, :], (1, win)))
    return np.concatenate(xs, axis=1), np.concatenate(ys, axis=1)


def check_corr_lookup(impl, case):
    """impl(levels, strides, hs, ws, coords (P, coord_stride), out (P, out_stride), radius) -> out after the call, all columns.
    Bar per element, M = max|level|: the position x / 2^l + (a - r) is one fp32 addition, off by at most ulp(x) / 2, and the zero-padded
    bilinear surface changes by at most 2 M per pixel along an axis: (ulp(x) + ulp(y)) M; plus 8 x 2^-24 x M for the weights, the
    four products and their sum.  A window entry more than a pixel outside its level is exactly 0; padding columns keep their bits."""
    radius, ostride, cstride, lpad = case
    levels, strides, coords = lookup_input(case)
    hs, ws = [h for h, _ in LOOKUP_LEVELS], [w for _, w in LOOKUP_LEVELS]
    win = 2 * radius + 1
    out0 = np.full((coords.shape[0], ostride), OUT_FILL, dtype=np.float32)
    out = impl([torch.from_numpy(l) for l in levels], strides, hs, ws, torch.from_numpy(coords), torch.from_numpy(out0.copy()), radius)
    ref = np.full(out0.shape, OUT_FILL, dtype=np.float64)
    ref[:, :4 * win * win] = corr_lookup_ref(levels, strides, hs, ws, coords, radius)
    x, y = lookup_positions(coords, radius)
    bar = np.zeros_like(ref)
    for l in range(4):
        sl = slice(l * win * win, (l + 1) * win * win)
        m = float(np.abs(levels[l][:, :hs[l] * ws[l]]).max())
        b = (ulp32(x[:, sl]) + ulp32(y[:, sl]) + 8 * U) * m
        outside = (x[:, sl] < -2) | (x[:, sl] > ws[l] + 1) | (y[:, sl] < -2) | (y[:, sl] > hs[l] + 1)
        bar[:, sl] = np.where(outside, 0.0, b)
    return judge("corr_lookup_f32", f"r={radius} out_stride={ostride} coord_stride={cstride} level_pad={lpad}", out, ref, bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# RAFT: uav_convex_upsample_f32: flow rows (N*h*w, flow_stride) + mask rows (N*h*w, 576 = 9 x 8 x 8) -> (N, 2, 8h, 8w)
CONVEX_CASES = [
    # (n, h, w, flow_stride, mask)
    (1, 1, 1, 2, "randn"),      # one pixel: 8 of the 9 neighbours are padding; 64 threads
    (2, 1, 5, 4, "randn"),      # one row: no vertical neighbours; padded flow rows
    (1, 3, 1, 2, "randn"),      # one column: no horizontal neighbours
    (2, 16, 20, 4, "randn"),    # interior pixels, two images, 160 blocks
    (2, 16, 20, 2, "wide"),     # mask entries of +-60: the softmax weights span 52 orders of magnitude
    (2, 1, 5, 2, "huge"),       # (beyond the issue's list) +-100: exp() of the raw entries overflows fp32 past 88.7, so this is the case
]                               # that needs the max subtraction; +-60 alone stays finite without it


def convex_input(case):
    n, h, w, fs, kind = case
    g = rng(25, n, h, w, fs, len(kind))
    flow = np.full((n * h * w, fs), 7e3, dtype=np.float32)              # padding columns would show if read
    flow[:, :2] = randn32(g, n * h * w, 2, scale=3.0)
    mask = randn32(g, n * h * w, 576)
    if kind != "randn":
        big = 60.0 if kind == "wide" else 100.0
        mask = (mask + g.choice([-big, 0.0, big], size=mask.shape, p=[0.1, 0.8, 0.1])).astype(np.float32)
    return flow, mask


def convex_upsample_ref(flow, mask, n, h, w):
    """RAFT.upsample_flow (raft.py:73-85): softmax over the 9 neighbours of mask (N,h,w,[9,8,8]), times the 3x3 zero-padded unfold of
    8 * flow, summed: out[n, c, 8y + sy, 8x + sx] = sum_k softmax_k(mask[n,y,x,:,sy,sx]) * 8 * flow[n, y + k/3 - 1, x + k%3 - 1, c]."""
    fl = f64(flow)[:, :2].reshape(n, h, w, 2)
    m = f64(mask).reshape(n, h, w, 9, 8, 8)
    m = np.exp(m - m.max(axis=3, keepdims=True))
    m = m / m.sum(axis=3, keepdims=True)
    fp = np.pad(8 * fl, [(0, 0), (1, 1), (1, 1), (0, 0)])
    out = np.zeros((n, 2, h, 8, w, 8))
    for k in range(9):
        nb = fp[:, k // 3:k // 3 + h, k % 3:k % 3 + w, :]                               # (n, h, w, 2)
        out += np.einsum("nyxab,nyxc->ncyaxb", m[:, :, :, k], nb)
    return out.reshape(n, 2, 8 * h, 8 * w)


def convex_torch(flow, mask, n, h, w):
    """The same through torch ops in the dtype of the inputs (the restatement of oracle/uav_oracle.py raft_upsample_flow)."""
    fl = flow[:, :2].reshape(n, h, w, 2).permute(0, 3, 1, 2)
    mk = mask.reshape(n, h, w, 576).permute(0, 3, 1, 2)
    mk = torch.softmax(mk.reshape(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * fl, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(mk * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)


def check_convex_upsample(impl, case):
    """impl(flow rows, mask rows, n, h, w) -> (n, 2, 8h, 8w).  Measured bar (expf): the torch ops of RAFT.upsample_flow in fp32."""
    n, h, w, fs, kind = case
    flow, mask = convex_input(case)
    out = impl(torch.from_numpy(flow), torch.from_numpy(mask), n, h, w)
    ref = convex_upsample_ref(flow, mask, n, h, w)
    t = convex_torch(torch.from_numpy(flow), torch.from_numpy(mask), n, h, w)
    return judge("convex_upsample_f32", f"{n}x{h}x{w} flow_stride={fs} {kind}", out, ref, measured_bar(t, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# scheduler: uav_cfg_ddim_v0(_f32), uav_ddim_vt(_f32).  cfg_ddim_v0 owns 8 elements per thread (fp16: one 16-byte vector when all 8
# exist), ddim_vt one.
SCHED_N = [1, 7, 8, 9, 8003]        # scalar tail only; 7 of 8; exactly one vector; a vector + a tail of 1; 4 blocks, tail of 3
SCHED_VARIANTS = [
    # (name, eps_text given, clip)
    ("cfg", True, False),
    ("cfg clip", True, True),           # clip_range 1.0, with |x0| up to ~3
    ("uncond", False, False),           # eps_text = None: the guided value is eps_uncond
    ("uncond clip", False, True),
]
SCHED_COEFS = dict(guidance=6.0, coef_sample=1.2, coef_eps=-0.7)
VT_COEFS = dict(coef_x0=0.9, coef_dir=0.4, eps_from_model=1.2, eps_from_sample=0.5)
VT_VARIANTS = [
    # (name, eps_from_x0, clip)
    ("plain", 0.0, False),
    ("x0 term", -0.35, False),          # eps_from_x0 != 0
    ("x0 term clip", -0.35, True),
    ("clip", 0.0, True),
]


def sched_input(n, dtype, tag):
    g = rng(26, n, tag)
    return [torch.from_numpy(randn32(g, n, scale=1.3)).to(dtype) for _ in range(3)]


def cfg_ddim_v0_ref(eu, ec, x, *, guidance, coef_sample, coef_eps, clip=False, clip_range=1.0, round_guided=None):
    """guided = eu + guidance * (ec - eu) (eu alone without a text branch); x0 = coef_sample * x + coef_eps * guided, clipped to
    +-clip_range.  `round_guided` rounds the guided value before x0 is formed (the fp16 kernel's documented rounding point)."""
    eu, x = f64(eu), f64(x)
    g = eu if ec is None else eu + guidance * (f64(ec) - eu)
    if round_guided is not None:
        g = round_guided(g)
    x0 = coef_sample * x + coef_eps * g
    return g, (np.clip(x0, -clip_range, clip_range) if clip else x0)


def ddim_vt_ref(x0, guided, x, *, coef_x0, coef_dir, eps_from_model, eps_from_sample, eps_from_x0=0.0, clip=False, clip_range=1.0):
    """prev = coef_x0 * a + coef_dir * (eps_from_model * guided + eps_from_sample * x + eps_from_x0 * a), a = x0 clipped."""
    a = f64(x0)
    if clip:
        a = np.clip(a, -clip_range, clip_range)
    return coef_x0 * a + coef_dir * (eps_from_model * f64(guided) + eps_from_sample * f64(x) + eps_from_x0 * a)


def _r16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def _kw32(kw):
    return {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in kw.items()}      # the fp32 numbers the C ABI takes


def check_cfg_ddim_v0(impl, n, variant, dtype):
    """impl(eps_uncond, eps_text or None, sample, **coefficients) -> (guided, x0).
    fp32: bar 8 x 2^-24 x the largest intermediate magnitude of the element.  fp16: guided within 1 fp16 ulp of the float64 value;
    x0 within 1 fp16 ulp of the float64 value formed from the guided value the op RETURNED (it is rounded to fp16 before x0 is
    formed)."""
    name, text, clip = variant
    eu, ec, x = sched_input(n, dtype, len(name))
    kw = _kw32(dict(SCHED_COEFS, clip=clip, clip_range=1.0))
    g, x0 = impl(eu, ec if text else None, x, **kw)
    tag = f"n={n} {name} {'fp16' if dtype == torch.float16 else 'fp32'}"
    rg, rx0 = cfg_ddim_v0_ref(eu, ec if text else None, x, **kw)
    d = np.abs(f64(ec) - f64(eu)) if text else 0.0
    mag_g = np.maximum(np.maximum(np.abs(f64(eu)), kw["guidance"] * d), np.abs(rg))
    if dtype == torch.float32:
        mag_x = np.maximum(np.maximum(np.abs(kw["coef_sample"] * f64(x)), np.abs(kw["coef_eps"] * rg)), mag_g)
        return worst([judge("cfg_ddim_v0_f32", tag + " guided", g, rg, 8 * U * mag_g),
                      judge("cfg_ddim_v0_f32", tag + " x0", x0, rx0, 8 * U * mag_x)])
    res = [judge("cfg_ddim_v0", tag + " guided", g, _r16(rg), ulp16(rg))]
    _, rx0 = cfg_ddim_v0_ref(eu, ec if text else None, x, round_guided=lambda _: f64(g), **kw)
    res.append(judge("cfg_ddim_v0", tag + " x0", x0, _r16(rx0), ulp16(rx0)))
    return worst(res)


def check_ddim_vt(impl, n, variant, dtype):
    """impl(x0, guided, sample, **coefficients) -> prev.  fp32: 8 x 2^-24 x the largest intermediate magnitude; fp16: 1 fp16 ulp of
    the float64 value."""
    name, e0, clip = variant
    x0, g, x = sched_input(n, dtype, 100 + len(name))
    kw = _kw32(dict(VT_COEFS, eps_from_x0=e0, clip=clip, clip_range=1.0))
    prev = impl(x0, g, x, **kw)
    ref = ddim_vt_ref(x0, g, x, **kw)
    a = np.clip(f64(x0), -1, 1) if clip else f64(x0)
    eps = kw["eps_from_model"] * f64(g) + kw["eps_from_sample"] * f64(x) + kw["eps_from_x0"] * a
    mag = np.max(np.abs([kw["eps_from_model"] * f64(g), kw["eps_from_sample"] * f64(x), kw["eps_from_x0"] * a, eps,
                         kw["coef_x0"] * a, kw["coef_dir"] * eps, ref]), axis=0)
    tag = f"n={n} {name} {'fp16' if dtype == torch.float16 else 'fp32'}"
    if dtype == torch.float32:
        return judge("ddim_vt_f32", tag, prev, ref, 8 * U * mag)
    return judge("ddim_vt", tag, prev, _r16(ref), ulp16(ref))


# ---------------------------------------------------------------------------------------------------------------------------------
def all_cases():
    """[(id, kernel key, check, arguments)]: every case of every kernel, the list both test files run.  `check(impls[key], *arguments)`."""
    out = []
    def add(key, check, *args):
        out.append((f"{key}-" + "-".join(str(a).replace(" ", "") for a in args), key, check, args))
    for c in PLANE_STATS_CASES:
        add("plane_stats", check_plane_stats, c)
    for hw in ADAIN_CASES:
        add("adain_apply", check_adain_apply, hw)
    for c in ATROUS_CASES:
        for preload in (False, True):
            add("atrous_blur", check_atrous_blur, c, preload)
    add("wavelet", check_wavelet)
    for c in BICUBIC_CASES:
        add("resize_bicubic", check_resize_bicubic, c)
    for c in INSTNORM_CASES:
        for relu in (False, True):
            add("instnorm", check_instnorm, c, relu)
    for n in ELEMENTWISE_N:
        for relu in (False, True):
            add("add_relu", check_add_relu, n, relu)
        add("axpby", check_axpby, n)
    for s in GRU_SHAPES:
        add("gru_rh", check_gru_rh, s)
        add("gru_blend", check_gru_blend, s)
    for c in COPY_COLS_CASES:
        for rows in COPY_COLS_ROWS:
            for act in COPY_COLS_ACTS:
                add("copy_cols", check_copy_cols, c, rows, act)
    for s in AVGPOOL_SHAPES:
        for pad in AVGPOOL_PAD:
            for p in AVGPOOL_P:
                add("avgpool2", check_avgpool2, s, pad, p)
    for c in BILINEAR_CASES:
        add("resize_bilinear", check_resize_bilinear, c)
    for c in LOOKUP_CASES:
        add("corr_lookup", check_corr_lookup, c)
    for c in CONVEX_CASES:
        add("convex_upsample", check_convex_upsample, c)
    for dtype in (torch.float32, torch.float16):
        for n in SCHED_N:
            for v in SCHED_VARIANTS:
                add("cfg_ddim_v0", check_cfg_ddim_v0, n, v, dtype)
            for v in VT_VARIANTS:
                add("ddim_vt", check_ddim_vt, n, v, dtype)
    return out


def _sched_out(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float16 if dtype == torch.float16 else np.float32)))


def _cfg_rounded(eu, ec, x, **kw):
    half = x.dtype == torch.float16
    g, x0 = cfg_ddim_v0_ref(eu, ec, x, round_guided=_r16 if half else None, **kw)
    return _sched_out(g, x.dtype), _sched_out(x0, x.dtype)


def reference_impls():
    """The float64 references behind the signatures of the ops, results rounded once to the op's output type: what every check must
    pass, and the base of the wrong variants."""
    def rounded(ref):
        return lambda *a: t32(ref(*a))
    return {
        "plane_stats": lambda x: tuple(t32(v) for v in plane_stats_ref(x)),
        "adain_apply": lambda x, cm, cv, sm, sv, eps: t32(adain_ref(x, cm, cv, sm, sv, eps)),
        "atrous_blur": lambda x, r, high: (t32(atrous_blur_ref(x, r)),
                                           None if high is None else t32(f64(high) + (f64(x) - atrous_blur_ref(x, r)))),
        "wavelet": (lambda im: tuple(t32(v) for v in wavelet_decomposition_ref(im)),
                    lambda c, s: t32(wavelet_reconstruction_ref(c, s))),
        "resize_bicubic": lambda x, ho, wo, sh, sw: t32(bicubic_ref(x, ho, wo, sh, sw)),
        "instnorm": lambda x, n_img, hw, relu, eps: t32(instnorm_ref(x, n_img, hw, relu, eps)),
        "add_relu": lambda a, b, relu: t32(np.maximum(f64(a) + f64(b), 0) if relu else f64(a) + f64(b)),
        "axpby": lambda x, z, a, b: t32(a * f64(x) + b * f64(z)),
        "gru_rh": lambda zr, h: t32(gru_rh_ref(zr, h)),
        "gru_blend": lambda zr, q, h: t32(gru_blend_ref(zr, q, h)),
        "copy_cols": rounded(copy_cols_ref),
        "avgpool2": rounded(avgpool2_ref),
        "resize_bilinear": rounded(bilinear_ref),
        "corr_lookup": lambda levels, strides, hs, ws, coords, out, radius: _lookup_into(levels, strides, hs, ws, coords, out, radius),
        "convex_upsample": rounded(convex_upsample_ref),
        "cfg_ddim_v0": _cfg_rounded,
        "ddim_vt": lambda x0, g, x, **kw: _sched_out(ddim_vt_ref(x0, g, x, **kw), x.dtype),
    }


def _lookup_into(levels, strides, hs, ws, coords, out, radius, ref=None):
    res = out.clone()
    win = 2 * radius + 1
    res[:, :4 * win * win] = t32((ref or corr_lookup_ref)(levels, strides, hs, ws, coords, radius))
    return res


def format_record(results):
    """One line per kernel: the measured error closest to its bar, that bar, and the case it occurred in."""
    by = collections.OrderedDict()
    for r in results:
        by.setdefault(r.kernel, []).append(r)
    lines = [f"{'kernel':<32}{'comparisons':>12}{'error':>12}{'bar':>12}  case"]
    for k, rs in by.items():
        w = worst(rs)
        lines.append(f"{k:<32}{len(rs):>12}{w.err:>12.3e}{w.bar:>12.3e}  {w.case}")
    return "\n".join(lines) + "\n"
