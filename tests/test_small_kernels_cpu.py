"""The edge-shape tests of the small fp32 kernels (tests/test_small_kernels_gpu.py) without a GPU: what makes them evidence.

  * pins: every float64 reference of tests/small_kernels_ref.py equals torch's own CPU op in float64, to 1e-12 relative, on every case
    torch accepts; the cases it refuses or defines differently are listed with the kernel's behaviour there;
  * the reference alone, rounded once to the op's output type, passes every check on every case of the GPU file, so each bar can be met;
  * every check rejects at least one named, value-only wrong variant of its op — the mistakes a kernel of this kind makes (a dropped
    strip, an unnormalised tail, a wrong clamp at one border, truncation for floor, ...)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import small_kernels_ref as R  # noqa: E402
import uav_oracle as O  # noqa: E402

CASES = R.all_cases()
REF = R.reference_impls()


def rel(a, b):
    a, b = R.f64(a), R.f64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---- pins -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PLANE_STATS_CASES, ids=str)
def test_pin_plane_stats(case):
    """torch.mean / torch.var (unbiased) in float64.  hw = 1: torch's unbiased variance is nan; the kernel documents 0."""
    x = d64(R.plane_stats_input(case))
    mean, var = R.plane_stats_ref(x)
    assert rel(mean, x.mean(dim=1)) <= 1e-12
    if case[2] == 1:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # torch warns that the degrees of freedom are <= 0
            assert torch.isnan(x.var(dim=1)).all() and (var == 0).all()
    else:
        assert float(np.abs(var - x.var(dim=1).numpy()).max()) <= 1e-12 * max(float(var.max()), 1e-5)


@pytest.mark.parametrize("hw", [h for h in R.ADAIN_CASES if h > 1])
def test_pin_adain_is_the_oracles(hw):
    """O.adain(content, style) in float64 = the statistics reference + the apply reference.  hw = 1 has no unbiased variance in torch."""
    x = d64(R.adain_input(hw)[0])[None, :, None]                                # (1, 3, 1, hw)
    g = torch.Generator().manual_seed(hw)
    style = torch.rand(x.shape, generator=g, dtype=torch.float64) * 0.5 + 0.1
    cm, cv = R.plane_stats_ref(x[0, :, 0])
    sm, sv = R.plane_stats_ref(style[0, :, 0])
    assert rel(R.adain_ref(x[0, :, 0], cm, cv, sm, sv, 1e-5), O.adain(x, style)[0, :, 0]) <= 1e-12


@pytest.mark.parametrize("case", R.ATROUS_CASES, ids=str)
def test_pin_atrous_blur(case):
    """F.conv2d on F.pad(mode='replicate') in float64, every case (replicate padding has no size limit), and the oracle's atrous_blur."""
    x = d64(R.atrous_input(case)[0])[None]
    r = case[2]
    k1 = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
    k = (k1[:, None] * k1[None, :])[None, None].repeat(x.shape[1], 1, 1, 1)
    t = F.conv2d(F.pad(x, (r,) * 4, mode="replicate"), k, groups=x.shape[1], dilation=r)
    ref = R.atrous_blur_ref(x[0], r)
    assert rel(ref, t[0]) <= 1e-12 and rel(ref, O.atrous_blur(x, r)[0]) <= 1e-12


def test_pin_wavelet():
    content, style = (d64(a) for a in R.wavelet_input())
    high, low = R.wavelet_decomposition_ref(content)
    oh, ol = O.wavelet_decomposition(content)
    assert rel(high, oh) <= 1e-12 and rel(low, ol) <= 1e-12
    assert rel(R.wavelet_reconstruction_ref(content, style), O.wavelet_reconstruction(content, style)) <= 1e-12


@pytest.mark.parametrize("case", R.BICUBIC_CASES, ids=str)
def test_pin_bicubic(case):
    """F.interpolate(scale_factor=4, mode='bicubic') in float64 (O.bicubic4), and the same with a size instead of the factor."""
    hi, wi = case
    x = d64(R.randn32(R.rng(16, hi, wi), R.BICUBIC_PLANES, hi, wi, scale=0.7))
    ref = R.bicubic_ref(x, 4 * hi, 4 * wi, 0.25, 0.25)
    assert rel(ref, O.bicubic4(x[None])[0]) <= 1e-12
    assert rel(ref, F.interpolate(x[None], size=(4 * hi, 4 * wi), mode="bicubic")[0]) <= 1e-12


def test_pin_bicubic_fractional_scale():
    x = torch.randn(1, 2, 9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert rel(R.bicubic_ref(x[0], 13, 7, 9 / 13, 11 / 7), F.interpolate(x, size=(13, 7), mode="bicubic")[0]) <= 1e-12


@pytest.mark.parametrize("case", R.INSTNORM_CASES, ids=str)
@pytest.mark.parametrize("relu", [False, True])
def test_pin_instnorm(case, relu):
    """F.instance_norm in float64.  hw = 1: torch refuses one spatial element; the kernel gives (x - x) * rsqrt(eps) = 0."""
    n_img, hw, c, _ = case
    x = d64(R.instnorm_input(case))
    ref = R.instnorm_ref(x, n_img, hw, relu, 1e-5)
    if hw == 1:
        with pytest.raises(ValueError):
            F.instance_norm(x.reshape(n_img, hw, c).permute(0, 2, 1), eps=1e-5)
        assert (ref == 0).all()
        return
    t = F.instance_norm(x.reshape(n_img, hw, c).permute(0, 2, 1), eps=1e-5).permute(0, 2, 1).reshape(-1, c)
    assert rel(ref, F.relu(t) if relu else t) <= 1e-12


@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES, ids=str)
def test_pin_avgpool2(shape):
    h, w = shape
    x = torch.randn(7, h * w + 3, dtype=torch.float64, generator=torch.Generator().manual_seed(h * w))
    t = F.avg_pool2d(x[:, :h * w].reshape(7, 1, h, w), 2, 2).reshape(7, -1)
    assert rel(R.avgpool2_ref(x, h * w + 3, h, w, 7), t) <= 1e-12


@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=str)
def test_pin_bilinear(case):
    hi, wi, ho, wo, r0, r1, planes = case
    x = d64(R.randn32(R.rng(23, hi, wi, ho, wo), planes, hi, wi, scale=5.0))
    t = F.interpolate(x[None], (ho, wo), mode="bilinear")[0]
    t[:, 0] *= r0                                                                # resize_flow_pytorch's row-indexed rescale
    if ho > 1:
        t[:, 1] *= r1
    assert rel(R.bilinear_ref(x, ho, wo, r0, r1), t) <= 1e-12


def test_pin_corr_lookup():
    """grid_sample(align_corners=True, zeros) through the oracle's _bilinear_sampler in float64 on the levels with both sides > 1, and
    O.raft_corr_lookup for the order of the 4 x 81 outputs (it returns fp32: compared to fp32 rounding).  Levels with a side of 1: the
    normalisation 2x / (w - 1) - 1 divides by zero and torch returns nan; the kernel samples in pixel coordinates, where a side of 1
    is like any other — those levels are held against the pixel-coordinate reference only."""
    for case in R.LOOKUP_CASES:
        radius = case[0]
        levels, strides, coords = R.lookup_input(case)
        hs, ws = [h for h, _ in R.LOOKUP_LEVELS], [w for _, w in R.LOOKUP_LEVELS]
        ref = R.corr_lookup_ref(levels, strides, hs, ws, coords, radius)
        p, win = coords.shape[0], 2 * radius + 1
        pyr = [d64(levels[l][:, :hs[l] * ws[l]]).reshape(p, 1, hs[l], ws[l]) for l in range(4)]
        d = torch.linspace(-radius, radius, win, dtype=torch.float64)
        delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)
        for l in (0, 1):
            cl = d64(coords[:, :2]).reshape(p, 1, 1, 2) / 2 ** l + delta.view(1, win, win, 2)
            t = O._bilinear_sampler(pyr[l], cl).reshape(p, win * win)
            assert float((t - d64(ref[:, l * win * win:(l + 1) * win * win])).abs().max()) <= 1e-12 * float(pyr[l].abs().max())
        assert torch.isnan(O._bilinear_sampler(pyr[3], d64(coords[:, :2]).reshape(p, 1, 1, 2))).all()
        two = O.raft_corr_lookup([q.float() for q in pyr[:2]], torch.from_numpy(coords[:, :2].T.copy()).reshape(1, 2, 1, p), r=radius)
        two = two.reshape(2 * win * win, p).T
        assert float((two.double() - d64(ref[:, :2 * win * win])).abs().max()) <= 1e-5


@pytest.mark.parametrize("case", R.CONVEX_CASES, ids=str)
def test_pin_convex_upsample(case):
    n, h, w, fs, _ = case
    flow, mask = (d64(a) for a in R.convex_input(case))
    ref = R.convex_upsample_ref(flow, mask, n, h, w)
    fl = flow[:, :2].reshape(n, h, w, 2).permute(0, 3, 1, 2)
    assert rel(ref, O.raft_upsample_flow(fl, mask.reshape(n, h, w, 576).permute(0, 3, 1, 2).contiguous())) <= 1e-12
    assert rel(ref, R.convex_torch(flow, mask, n, h, w)) <= 1e-12


def test_pin_scheduler_formulas():
    """DDIMScheduler.step's prediction of x0 and of the previous sample, written out in float64."""
    g = torch.Generator().manual_seed(2)
    eu, ec, x = (torch.randn(50, dtype=torch.float64, generator=g) for _ in range(3))
    gd, x0 = R.cfg_ddim_v0_ref(eu, ec, x, guidance=6.0, coef_sample=1.2, coef_eps=-0.7, clip=True, clip_range=1.0)
    tg = eu + 6.0 * (ec - eu)
    assert rel(gd, tg) <= 1e-12 and rel(x0, (1.2 * x - 0.7 * tg).clamp(-1, 1)) <= 1e-12
    prev = R.ddim_vt_ref(d64(x0), gd, x, coef_x0=0.9, coef_dir=0.4, eps_from_model=1.2, eps_from_sample=0.5, eps_from_x0=-0.35)
    assert rel(prev, 0.9 * d64(x0) + 0.4 * (1.2 * tg + 0.5 * x - 0.35 * d64(x0))) <= 1e-12


# ---- the reference alone passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,check,args", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_reference_passes(key, check, args):
    res = check(REF[key], *args)
    assert res.err <= res.bar


def test_every_kernel_has_cases():
    assert {c[1] for c in CASES} == set(REF) and len(CASES) > 150


# ---- each check can fail ------------------------------------------------------------------------------------------------------------
def _stats_skipping_second_strip(x):
    """statistics that skip elements >= 16384 of a chunk (a strip loop that runs once)"""
    x = R.f64(x)
    n = x.shape[1]
    per = -(-n // 64)
    kept = np.where((np.arange(n) % per) < 16384, 1.0, 0.0)[None]
    s, q = (x * kept).sum(axis=1), (x * x * kept).sum(axis=1)
    m = s / n
    return R.t32(m), R.t32((q - n * m * m) / (n - 1) if n > 1 else 0 * m)


def _stats_fp32_squares(x):
    """statistics whose variance is q - n m^2 with every square rounded to fp32"""
    x32 = np.asarray(x, dtype=np.float32)
    n = x32.shape[1]
    s, q = x32.astype(np.float64).sum(axis=1), (x32 * x32).astype(np.float64).sum(axis=1)
    m = s / n
    return R.t32(m), R.t32(np.maximum((q - n * m * m) / (n - 1), 0) if n > 1 else 0 * m)


def _adain_raw_tail(x, cm, cv, sm, sv, eps):
    """AdaIN that leaves the last hw % 4 elements unnormalised"""
    out = REF["adain_apply"](x, cm, cv, sm, sv, eps)
    k = x.shape[1] % 4
    if k:
        out[:, -k:] = x[:, -k:]
    return out


def _adain_misaligned_plane_takes_neighbour(x, cm, cv, sm, sv, eps):
    """AdaIN whose misaligned planes lose their first element to the neighbour (vector path taken on a misaligned base, rounded down)"""
    out = REF["adain_apply"](x, cm, cv, sm, sv, eps)
    for p in range(1, x.shape[0]):
        if (p * x.shape[1]) % 4:
            out[p, 0] = out[p - 1, -1]
    return out


def _blur_indexed(x, r, wside=0.25, reflect_left=False):
    x = R.f64(x)
    h, w = x.shape[-2:]
    ys, xs = np.arange(h), np.arange(w)
    ym, yp = np.clip(ys - r, 0, h - 1), np.clip(ys + r, 0, h - 1)
    xm, xp = np.clip(xs - r, 0, w - 1), np.clip(xs + r, 0, w - 1)
    if reflect_left:                                 # the left tap mirrors at column 0 instead of staying on it
        xm = np.where(xs - r < 0, np.clip(r - xs, 0, w - 1), xm)
    k = (wside, 0.5, 0.25)
    out = np.zeros_like(x)
    for a, yy in enumerate((ym, ys, yp)):
        for b, xx in enumerate((xm, xs, xp)):
            out += k[a] * k[b] * x[..., yy, :][..., xx]
    return out


def _blur_variant(**kw):
    def impl(x, r, high):
        low = _blur_indexed(x, r, **kw)
        return R.t32(low), None if high is None else R.t32(R.f64(high) + R.f64(x) - low)
    return impl


def _blur_high_overwrites(x, r, high):
    """blur whose `high` is overwritten instead of accumulated"""
    low = R.atrous_blur_ref(x, r)
    return R.t32(low), None if high is None else R.t32(R.f64(x) - low)


def _wavelet_four_levels():
    """wavelet split that stops after four levels"""
    return (lambda im: tuple(R.t32(v) for v in R.wavelet_decomposition_ref(im, levels=4)), REF["wavelet"][1])


def _bicubic_wrapped_top(x, ho, wo, sh, sw):
    """bicubic with the top tap unclamped-then-wrapped (row -1 read as the last row)"""
    def wrap_low(i, n):
        return i % n if i < 0 else min(i, n - 1)
    x = R.f64(x)
    return R.t32(R.cubic_weights(x.shape[-2], ho, sh, tap=wrap_low) @ x @ R.cubic_weights(x.shape[-1], wo, sw).T)


def _bicubic_a_half(x, ho, wo, sh, sw):
    """bicubic with A = -0.5 (the Catmull-Rom weights) instead of ATen's -0.75"""
    x = R.f64(x)
    return R.t32(R.cubic_weights(x.shape[-2], ho, sh, a=-0.5) @ x @ R.cubic_weights(x.shape[-1], wo, sw, a=-0.5).T)


def _instnorm_unbiased(x, n_img, hw, relu, eps):
    """instance norm with the unbiased variance"""
    v = R.f64(x).reshape(n_img, hw, -1)
    m = v.mean(axis=1, keepdims=True)
    y = (v - m) / np.sqrt(((v - m) ** 2).sum(axis=1, keepdims=True) / max(hw - 1, 1) + eps)
    return R.t32((np.maximum(y, 0) if relu else y).reshape(n_img * hw, -1))


def _instnorm_one_pass_fp32(x, n_img, hw, relu, eps):
    """instance norm with the one-pass variance E[x^2] - mean^2 in fp32"""
    v = np.asarray(x, dtype=np.float32).reshape(n_img, hw, -1)
    m = v.mean(axis=1, keepdims=True, dtype=np.float32)
    var = np.maximum((v * v).mean(axis=1, keepdims=True, dtype=np.float32) - m * m, 0)
    y = (v - m) / np.sqrt(var + np.float32(eps))
    return torch.from_numpy((np.maximum(y, 0) if relu else y).reshape(n_img * hw, -1).astype(np.float32))


def _instnorm_padding_channel_leaks(x, n_img, hw, relu, eps):
    """instance norm whose last channel of a partial slab takes the statistics of channel 0 (an unguarded lane)"""
    out = REF["instnorm"](x, n_img, hw, relu, eps)
    c = x.shape[1]
    if c % 32:
        v = R.f64(x).reshape(n_img, hw, c)
        m = v[:, :, :1].mean(axis=1, keepdims=True)
        s = np.sqrt(((v[:, :, :1] - m) ** 2).mean(axis=1, keepdims=True) + eps)
        y = ((v[:, :, -1:] - m) / s).reshape(n_img * hw)
        out[:, -1] = R.t32(np.maximum(y, 0) if relu else y)
    return out


def _last_of_partial_block_unwritten(key):
    def impl(*a, **k):
        out = REF[key](*a, **k).clone()
        if out.numel() % 256:
            out.view(-1)[-1] = 0.0
        return out
    return impl


def _copy_cols_shifted(src, scol, dst, dcol, ncols, act):
    """column copy that lands one column to the right"""
    out = dst.clone()
    out[:, dcol + 1:dcol + 1 + ncols] = REF["copy_cols"](src, scol, dst, dcol, ncols, act)[:, dcol:dcol + ncols][:, :dst.shape[1] - dcol - 1]
    return out


def _copy_cols_tanh_is_relu(src, scol, dst, dcol, ncols, act):
    """column copy whose act 4 (tanh) runs act 1 (ReLU)"""
    return REF["copy_cols"](src, scol, dst, dcol, ncols, 1 if act == 4 else act)


def _copy_cols_row_stride_swapped(src, scol, dst, dcol, ncols, act):
    """column copy that walks the source with the destination's row stride"""
    flat = torch.cat([src.reshape(-1), torch.zeros(dst.numel())])
    rows = src.shape[0]
    idx = torch.arange(rows)[:, None] * dst.shape[1] + scol + torch.arange(ncols)[None, :]
    fake = torch.zeros_like(src)
    fake[:, scol:scol + ncols] = flat[idx]
    return REF["copy_cols"](fake, scol, dst, dcol, ncols, act)


def _avgpool_packed_rows(src, stride, h, w, p):
    """avgpool that takes 2 * (w / 2) for the row pitch, so reads column w - 1 of the row above for odd w"""
    v = R.f64(src).reshape(p, stride)
    h2, w2 = h // 2, w // 2
    out = np.zeros((p, h2, w2))
    for y in range(h2):
        for x in range(w2):
            o = 2 * y * (2 * w2) + 2 * x
            out[:, y, x] = 0.25 * (v[:, o] + v[:, o + 1] + v[:, o + 2 * w2] + v[:, o + 2 * w2 + 1])
    return R.t32(out.reshape(p, h2 * w2))


def _avgpool_dense_volumes(src, stride, h, w, p):
    """avgpool that ignores src_stride (volumes taken as densely packed)"""
    flat = R.f64(src).reshape(-1)
    dense = np.stack([flat[i * h * w:(i + 1) * h * w] for i in range(p)])
    return R.t32(R.avgpool2_ref(dense, h * w, h, w, p))


def _bilinear_extrapolating(x, ho, wo, r0, r1):
    """bilinear that does not clamp negative source positions to 0 (extrapolates at the top / left border)"""
    def weights(n_in, n_out):
        m = np.zeros((n_out, n_in))
        for o in range(n_out):
            src = n_in / n_out * (o + 0.5) - 0.5
            i0 = min(max(int(np.floor(src)), 0), n_in - 1)
            i1 = i0 + (1 if i0 < n_in - 1 else 0)
            m[o, i0] += 1 - (src - i0)
            m[o, i1] += src - i0
        return m
    v = R.f64(x)
    out = weights(v.shape[-2], ho) @ v @ weights(v.shape[-1], wo).T
    out[..., 0, :] *= r0
    if ho > 1:
        out[..., 1, :] *= r1
    return R.t32(out)


def _bilinear_scales_on_channels(x, ho, wo, r0, r1):
    """bilinear that scales planes 0 and 1 (the flow channels) instead of rows 0 and 1"""
    out = R.bilinear_ref(x, ho, wo)
    out[0::2] *= r0
    out[1::2] *= r1
    return R.t32(out)


def _lookup_variant(trunc=False, swap=False):
    def ref(levels, strides, hs, ws, coords, radius):
        if swap:                                     # the second window index moves x
            win = 2 * radius + 1
            out = R.corr_lookup_ref(levels, strides, hs, ws, coords, radius)
            return out.reshape(-1, 4, win, win).transpose(0, 1, 3, 2).reshape(out.shape)
        return R.corr_lookup_ref(levels, strides, hs, ws, coords, radius, floor=np.trunc)      # truncation instead of floor
    return lambda levels, strides, hs, ws, coords, out, radius: R._lookup_into(levels, strides, hs, ws, coords, out, radius, ref=ref)


def _lookup_writes_padding(levels, strides, hs, ws, coords, out, radius):
    """lookup that zeroes the padding columns of its output rows"""
    res = REF["corr_lookup"](levels, strides, hs, ws, coords, out, radius)
    res[:, 4 * (2 * radius + 1) ** 2:] = 0
    return res


def _convex_no_max_subtraction(flow, mask, n, h, w):
    """convex upsampling whose fp32 softmax does not subtract the maximum"""
    m = torch.exp(mask.reshape(n, h, w, 9, 8, 8))
    m = (m / m.sum(dim=3, keepdim=True)).double().numpy()
    fp = np.pad(8 * R.f64(flow)[:, :2].reshape(n, h, w, 2), [(0, 0), (1, 1), (1, 1), (0, 0)])
    out = np.zeros((n, 2, h, 8, w, 8))
    for k in range(9):
        out += np.einsum("nyxab,nyxc->ncyaxb", m[:, :, :, k], fp[:, k // 3:k // 3 + h, k % 3:k % 3 + w, :])
    return R.t32(out.reshape(n, 2, 8 * h, 8 * w))


def _convex_transposed_neighbours(flow, mask, n, h, w):
    """convex upsampling whose neighbour k is (k % 3, k / 3) instead of (k / 3, k % 3)"""
    m = R.f64(mask).reshape(n, h, w, 3, 3, 64).transpose(0, 1, 2, 4, 3, 5).reshape(n * h * w, 576)
    return REF["convex_upsample"](flow, torch.from_numpy(m), n, h, w)


def _cfg_clip_before_guidance(eu, ec, x, *, guidance, coef_sample, coef_eps, clip=False, clip_range=1.0):
    """cfg_ddim_v0 that clips before the guidance: x0 = clip(cs x + ce eu) + ce (guided - eu)"""
    g, _ = R.cfg_ddim_v0_ref(eu, ec, x, guidance=guidance, coef_sample=coef_sample, coef_eps=coef_eps)
    if x.dtype == torch.float16:
        g = R._r16(g)
    x0 = coef_sample * R.f64(x) + coef_eps * R.f64(eu)
    if clip:
        x0 = np.clip(x0, -clip_range, clip_range)
    x0 = x0 + coef_eps * (g - R.f64(eu))
    return R._sched_out(g, x.dtype), R._sched_out(x0, x.dtype)


def _cfg_ignores_missing_text(eu, ec, x, **kw):
    """cfg_ddim_v0 that scales eps_uncond by (1 - guidance) when there is no text branch (reads it as zeros)"""
    return REF["cfg_ddim_v0"](eu, torch.zeros_like(eu) if ec is None else ec, x, **kw)


def _cfg_scalar_tail_skips_clip(eu, ec, x, **kw):
    """cfg_ddim_v0 whose scalar tail (the last n % 8 elements) skips the clip"""
    g, x0 = REF["cfg_ddim_v0"](eu, ec, x, **kw)
    k = x.numel() % 8
    if k:
        _, raw = REF["cfg_ddim_v0"](eu[-k:], None if ec is None else ec[-k:], x[-k:], **dict(kw, clip=False))
        x0[-k:] = raw
    return g, x0


def _vt_ignores_eps_from_x0(x0, g, x, **kw):
    """ddim_vt that ignores eps_from_x0"""
    return REF["ddim_vt"](x0, g, x, **dict(kw, eps_from_x0=0.0))


def _vt_clips_only_the_direction(x0, g, x, *, coef_x0, clip=False, clip_range=1.0, **kw):
    """ddim_vt that clips x0 inside the direction term only"""
    prev = R.ddim_vt_ref(x0, g, x, coef_x0=0.0, clip=clip, clip_range=clip_range, **kw) + coef_x0 * R.f64(x0)
    return R._sched_out(prev, x.dtype)


def _wavelet_low_band_from_content():
    """wavelet reconstruction that takes the low band from the content, not the style (returns the content)"""
    return (REF["wavelet"][0], lambda c, s: R.t32(sum(R.wavelet_decomposition_ref(c))))


MUTANTS = [
    ("plane_stats", "skips elements >= 16384 of a chunk", _stats_skipping_second_strip),
    ("plane_stats", "squares rounded to fp32 before they are summed", _stats_fp32_squares),
    ("plane_stats", "biased variance", lambda x: (R.t32(R.plane_stats_ref(x)[0]), R.t32(R.f64(x).var(axis=1)))),
    ("adain_apply", "last hw % 4 elements unnormalised", _adain_raw_tail),
    ("adain_apply", "first element of a misaligned plane taken from its neighbour", _adain_misaligned_plane_takes_neighbour),
    # (xm and xp exchanged at a border is NOT a wrong variant: the two taps carry the same weight, the sum is the same number)
    ("atrous_blur", "left tap reflected, not replicated, at the left border only", _blur_variant(reflect_left=True)),
    ("atrous_blur", "a tap weight of 0.124", _blur_variant(wside=0.248)),
    ("atrous_blur", "high overwritten, not accumulated", _blur_high_overwrites),
    ("wavelet", "four levels", _wavelet_four_levels()),
    ("wavelet", "low band of the reconstruction taken from the content", _wavelet_low_band_from_content()),
    ("resize_bicubic", "top tap unclamped, then wrapped", _bicubic_wrapped_top),
    ("resize_bicubic", "A = -0.5", _bicubic_a_half),
    ("instnorm", "unbiased variance", _instnorm_unbiased),
    ("instnorm", "one-pass fp32 variance", _instnorm_one_pass_fp32),
    ("instnorm", "unguarded lane of a partial slab", _instnorm_padding_channel_leaks),
    ("add_relu", "last element of a partial block unwritten", _last_of_partial_block_unwritten("add_relu")),
    ("add_relu", "ReLU on the first operand only", lambda a, b, relu: R.t32(np.maximum(R.f64(a), 0) + R.f64(b) if relu else R.f64(a) + R.f64(b))),
    ("axpby", "last element of a partial block unwritten", _last_of_partial_block_unwritten("axpby")),
    ("axpby", "a and b exchanged", lambda x, z, a, b: REF["axpby"](x, z, b, a)),
    ("gru_rh", "multiplies by z, the first half of the rows", lambda zr, h: R.t32(R.f64(zr)[:, :h.shape[1]] * R.f64(h))),
    ("gru_rh", "last element of a partial block unwritten", _last_of_partial_block_unwritten("gru_rh")),
    ("gru_blend", "z and 1 - z exchanged", lambda zr, q, h: REF["gru_blend"](zr, h, q)),
    ("gru_blend", "last element of a partial block unwritten", _last_of_partial_block_unwritten("gru_blend")),
    ("copy_cols", "lands one column to the right", _copy_cols_shifted),
    ("copy_cols", "tanh runs ReLU", _copy_cols_tanh_is_relu),
    ("copy_cols", "source walked with the destination's stride", _copy_cols_row_stride_swapped),
    ("avgpool2", "reads column w - 1 for odd w", _avgpool_packed_rows),
    ("avgpool2", "ignores src_stride", _avgpool_dense_volumes),
    ("resize_bilinear", "negative positions not clamped", _bilinear_extrapolating),
    ("resize_bilinear", "row scales applied to planes", _bilinear_scales_on_channels),
    ("corr_lookup", "truncation instead of floor for negative coordinates", _lookup_variant(trunc=True)),
    ("corr_lookup", "window indices exchanged", _lookup_variant(swap=True)),
    ("corr_lookup", "padding columns zeroed", _lookup_writes_padding),
    ("convex_upsample", "softmax without the max subtraction", _convex_no_max_subtraction),
    ("convex_upsample", "neighbours transposed", _convex_transposed_neighbours),
    ("cfg_ddim_v0", "clips before the guidance", _cfg_clip_before_guidance),
    ("cfg_ddim_v0", "no text branch read as zeros", _cfg_ignores_missing_text),
    ("cfg_ddim_v0", "scalar tail skips the clip", _cfg_scalar_tail_skips_clip),
    ("ddim_vt", "ignores eps_from_x0", _vt_ignores_eps_from_x0),
    ("ddim_vt", "clips x0 in the direction term only", _vt_clips_only_the_direction),
]


@pytest.mark.parametrize("key,name,impl", MUTANTS, ids=[f"{k}: {n}" for k, n, _ in MUTANTS])
def test_wrong_variant_is_rejected(key, name, impl):
    """Run the variant through every case of its kernel: at least one check must raise, with the measured error over the bar."""
    rejected = []
    for cid, k, check, args in CASES:
        if k != key:
            continue
        try:
            with np.errstate(all="ignore"):
                check(impl, *args)
        except AssertionError as e:
            assert "over the bar" in str(e) or "negative variance" in str(e), e
            rejected.append(cid)
    print(f"{key}: {name}: rejected by {len(rejected)} case(s): {rejected[:6]}")
    assert rejected, f"no case of {key} notices: {name}"


def test_every_kernel_has_a_wrong_variant():
    assert {m[0] for m in MUTANTS} == set(REF)
    for dtype in ("torch.float16", "torch.float32"):            # the scheduler kernels in both types
        assert any(c[1] == "cfg_ddim_v0" and dtype in c[0] for c in CASES) and any(c[1] == "ddim_vt" and dtype in c[0] for c in CASES)
