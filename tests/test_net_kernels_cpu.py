"""The edge-shape tests of the norm, temporal-attention and layout kernels (tests/test_net_kernels_gpu.py) without a GPU: what makes
them evidence.

  * pins: every float64 reference of tests/net_kernels_ref.py equals torch's own CPU op in float64 to 1e-12 relative; temporal attention
    equals the float64 formula of tests/test_kernels_gpu.py::test_temporal_attention.  For run time the GroupNorm pins leave out the
    shapes of 4097 instances and of 4096 rows and the LayerNorm pins the two of 16 390 rows: the same reference functions are pinned at
    every other shape, and nothing in them depends on the row or instance count;
  * the reference alone, rounded once to the op's output type (temporal attention: the evaluation with the two documented fp16
    roundings), passes every check on every case of the GPU file, so each bar can be met;
  * every check rejects named wrong variants of its op;
  * a numpy emulation of GroupNorm's statistics pass with plain fp32 sums of x and x * x — the form csrc/norm.hip had — fails the
    `nearconst` data and passes `randn`, so the cases see that defect.  (The emulation of the pivoted sums it has now passes all five kinds; that one is an illustration
    of the method kept in step with the kernel by hand and proves nothing about the GPU code, which the GPU file tests.)"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import net_kernels_ref as R  # noqa: E402

CASES = R.all_cases()
REF = R.reference_impls()


def rel(a, b):
    a, b = R.f64(a), R.f64(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def d64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


# ---- pins -----------------------------------------------------------------------------------------------------------------------
PIN_GN = [s for s in R.GN_SHAPES if s[4] <= 3 and s[5] <= 1025]


@pytest.mark.parametrize("shape", PIN_GN, ids=lambda s: R.gn_name(s, True).replace(" ", "_"))
def test_pin_groupnorm(shape):
    """torch's GroupNorm in float64 on the channels the groups cover = the tables of the reference applied by the apply reference."""
    c1, c2, c_real, groups, n_inst, rows, bcast, kind = shape
    _, _, x, gamma, beta = R.gn_input(shape, True)
    scale, shift, _ = R.gn_stats_ref(x, c_real, groups, R.GN_EPS, gamma, beta)
    t, mean, rstd = torch.native_group_norm(d64(x[:, :, :c_real].transpose(0, 2, 1)), d64(gamma[:c_real]), d64(beta[:c_real]), n_inst,
                                            c_real, rows, groups, R.GN_EPS)      # F.group_norm's kernel (F.group_norm refuses 1 x c x 1)
    m, r = (v.repeat_interleave(c_real // groups, 1) for v in (mean, rstd))
    assert rel(scale[:, :c_real], d64(gamma[:c_real]) * r) <= 1e-12
    assert rel(shift[:, :c_real], d64(beta[:c_real]) - m * r * d64(gamma[:c_real])) <= 1e-12
    assert (scale[:, c_real:] == 0).all() and (shift[:, c_real:] == 0).all()
    # y = x * scale + shift cancels where the mean is large against the spread: the tolerance is relative to the terms
    size = float((np.abs(x * scale[:, None, :]) + np.abs(shift[:, None, :])).max())
    for silu_on in (False, True):
        y = R.gn_apply_ref(x, scale, shift, silu_on)[:, :, :c_real]
        want = (F.silu(t) if silu_on else t).permute(0, 2, 1).numpy()
        assert float(np.abs(y - want).max()) <= 1e-12 * size


@pytest.mark.parametrize("case", [c for c in R.LN_CASES if c[0] <= 777], ids=str)
def test_pin_layernorm(case):
    x, gamma, beta = R.ln_input(case, True)
    t = F.layer_norm(d64(x), (case[1],), d64(gamma), d64(beta), R.LN_EPS)
    assert rel(R.layernorm_ref(x, gamma, beta, R.LN_EPS), t) <= 1e-12


def _torch_rope(x, cos, sin):
    """ref_rope of tests/test_kernels_gpu.py in float64, on the tables instead of the frequencies."""
    rd = cos.shape[-1] * 2
    if rd == 0:
        return x
    c2, s2 = cos.repeat_interleave(2, -1), sin.repeat_interleave(2, -1)
    xr, xp = x[..., :rd], x[..., rd:]
    x1, x2 = xr[..., 0::2], xr[..., 1::2]
    rot = torch.stack((-x2, x1), dim=-1).reshape(xr.shape)
    return torch.cat([xr * c2 + rot * s2, xp], dim=-1)


@pytest.mark.parametrize("case", R.TATTN_CASES, ids=str)
def test_pin_temporal_attention(case):
    c, heads, rot, t_len, hw, nb = case
    qkv, bias, cos, sin, scale = R.tattn_input(case)
    x = d64(qkv).reshape(nb, t_len, hw, 3, heads, c // heads).permute(3, 0, 2, 4, 1, 5)
    q, k, v = _torch_rope(x[0] * scale, d64(cos), d64(sin)), _torch_rope(x[1], d64(cos), d64(sin)), x[2]
    s = q @ k.transpose(-1, -2) + d64(bias)[None, None]
    s = s - s.amax(-1, keepdim=True)
    o = (torch.softmax(s, -1) @ v).permute(0, 3, 1, 2, 4).reshape(nb * t_len * hw, c)
    assert rel(R.tattn_ref(qkv, bias, cos, sin, scale, case)[0], o) <= 1e-12


def test_pin_elementwise():
    g = torch.Generator().manual_seed(3)
    x, w, b = (torch.randn(s, dtype=torch.float64, generator=g) for s in ((3, 40), (7, 40), (7,)))
    assert rel(R.linear_small_ref(x, w, b, True, True), F.silu(F.linear(F.silu(x), w, b))) <= 1e-12
    assert rel(R.linear_small_ref(x, w, None, False, False), F.linear(x, w)) <= 1e-12
    t = d64(R.TIMESTEPS)
    for dim, flip, shift in R.TEMB_CASES:
        if dim == 2 and shift == 1.0:
            assert np.isnan(R.timestep_embedding_ref(t, dim, flip, shift)).all()
            continue
        half = dim // 2                                                  # diffusers get_timestep_embedding, scale 1, max_period 10000
        emb = t[:, None] * torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float64) / (half - shift))[None]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
        if flip:
            emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
        assert rel(R.timestep_embedding_ref(t, dim, flip, shift), emb) <= 1e-12
    a, b2 = torch.randn(2, 4, 3, 5, generator=g).half(), torch.randn(2, 3, 3, 5, generator=g).half()
    want = F.pad(torch.cat([a, b2], 1).permute(0, 2, 3, 1).reshape(-1, 7), (0, 1))
    assert torch.equal(torch.from_numpy(R.pack_nhwc_ref(a.numpy(), b2.numpy(), 8, 1.0)), want)
    rows = torch.randn(2 * 3 * 5, 8, generator=g)
    want = rows[:, :3].clamp(-1, 1).reshape(2, 3, 5, 3).permute(0, 3, 1, 2).half()
    assert torch.equal(torch.from_numpy(R.unpack_ncthw_ref(rows.numpy(), 3, 2, 3, 5, False, -1.0, 1.0)), want)
    x32 = torch.from_numpy(R.wide_values(R.rng(1), (5, 8)))
    hi = x32.half()
    assert torch.equal(torch.from_numpy(R.hilo_ref(x32.numpy())), torch.cat([hi, (x32 - hi.float()).half()], 1))


# ---- the rounded reference passes every check ------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,check,args", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_rounded_reference_passes(key, check, args):
    res = check(REF[key], *args)
    assert res.err <= res.bar


def test_documented_roundings_stay_far_below_the_element_bar():
    """Temporal attention: the evaluation with the fp16 roundings of the rotated q and k stays at <= 0.15 of the per-element bar."""
    for case in R.TATTN_CASES:
        if case[3] == 1:
            continue
        ref, bar, _ = R.tattn_marks(case)
        qkv, bias, cos, sin, scale = R.tattn_input(case)
        got = R.f64(R.t16(R.tattn_ref(qkv, bias, cos, sin, scale, case, rounded=True)[0]))
        assert float((np.abs(got - ref) / bar).max()) <= 0.15, case


# ---- wrong variants are rejected -------------------------------------------------------------------------------------------------
def rejected(check, impl, *args):
    with pytest.raises(AssertionError):
        check(impl, *args)


def _gn_stats_variant(**kw):
    return lambda *a: REF["gn_scale_shift"](*a, **kw)


GN64 = (64, 0, 64, 32, 1, 513, False, "tiny")
GN_SEAM = (1280, 640, 1920, 32, 1, 37, False, "randn")
GN_PAD = (8, 0, 4, 2, 2, 9, False, "randn")


@pytest.mark.parametrize("f32", [False, True])
def test_groupnorm_statistics_variants_are_rejected(f32):
    chk = R.check_groupnorm_scale_shift
    rejected(chk, _gn_stats_variant(eps_mode="dropped"), GN64, f32)
    rejected(chk, _gn_stats_variant(eps_mode="outside"), GN64, f32)
    rejected(chk, _gn_stats_variant(unbiased=True), (24, 0, 24, 3, 2, 85, False, "randn"), f32)
    seam = np.arange(1920) // 60
    seam[1280:] = np.minimum((np.arange(1280, 1920) + 1) // 60, 31)      # the second source's channels found one channel late
    rejected(chk, _gn_stats_variant(group_of=seam), GN_SEAM, f32)
    rows = np.delete(np.arange(513), 511)                                # the last row of chunk 0 (512 rows per chunk) dropped
    rejected(chk, _gn_stats_variant(rows_used=rows), (64, 0, 64, 32, 1, 513, False, "randn"), f32)

    def pad_not_zeroed(*a):
        s, h = REF["gn_scale_shift"](*a)
        s[:, 4:], h[:, 4:] = 1.0, 0.0
        return s, h
    rejected(chk, pad_not_zeroed, GN_PAD, f32)


@pytest.mark.parametrize("f32", [False, True])
def test_groupnorm_apply_variants_are_rejected(f32):
    chk = R.check_groupnorm_apply
    shape = (320, 0, 320, 32, 3, 77, False, "randn")
    rejected(chk, lambda *a: REF["gn_apply"](*a, side="before"), shape, f32, True, 0)

    def raw_variant(**kw):
        def impl(x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode):
            y, _ = REF["gn_apply"](x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode)
            return y, torch.from_numpy(R.hilo_ref(R.gn_logical(x1, x2, x2_rows, n_inst, rows).reshape(n_inst * rows, -1), **kw))
        return impl
    rejected(chk, raw_variant(swapped=True), shape, f32, True, 2)
    if f32:                                                              # fp16 rows have lo = 0 either way
        rejected(chk, raw_variant(lo_from_unrounded=True), shape, f32, True, 2)

    def pad_not_zeroed(x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode):
        y, raw = REF["gn_apply"](x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode)
        y[:, 4:] = x1[:, 4:].half()
        return y, raw
    rejected(chk, pad_not_zeroed, GN_PAD, f32, False, 0)


def test_hilo_variants_are_rejected_by_the_cast_check():
    rejected(R.check_cast_f32_hilo, lambda x: torch.from_numpy(R.hilo_ref(x.numpy(), swapped=True)), (33, 320))
    rejected(R.check_cast_f32_hilo, lambda x: torch.from_numpy(R.hilo_ref(x.numpy(), lo_from_unrounded=True)), (33, 320))


@pytest.mark.parametrize("f32", [False, True])
def test_layernorm_variants_are_rejected(f32):
    tiny = (777, 520, "tiny")
    rejected(R.check_layernorm, lambda *a: REF["layernorm"](*a, eps_mode="dropped"), tiny, f32)
    rejected(R.check_layernorm, lambda *a: REF["layernorm"](*a, eps_mode="outside"), tiny, f32)
    rejected(R.check_layernorm, lambda *a: REF["layernorm"](*a, unbiased=True), (5, 8, "randn"), f32)

    def second_vector_dropped(x, gamma, beta, eps):                      # NV = 1 run on c = 520: channels 512.. never written
        y = REF["layernorm"](x, gamma, beta, eps)
        y[:, 512:] = 0
        return y
    rejected(R.check_layernorm, second_vector_dropped, (1, 520, "randn"), f32)


def test_finalize_variants_are_rejected():
    def one_chunk_dropped(part, *a):
        p = part.clone()
        p[:, :, -1] = 0                                                  # chunk 1024 of 1025: the block's second round not taken
        return REF["gn_finalize_partials"](p, *a)
    rejected(R.check_finalize_partials, one_chunk_dropped, (1025, 8, 8, 1))

    def source2_not_broadcast(p1, c1, g1, n1, p2, c2, g2, n2, *a):       # instance 1 reads past source 2's one instance: zeros here
        return REF["gn_finalize_partials2"](p1, c1, g1, n1, torch.cat([p2, torch.zeros_like(p2)], dim=2), c2, g2, 2 * n2, *a)
    rejected(R.check_finalize_partials2, source2_not_broadcast, (1, 16, 2, 2, 16, 8, 1, 4, 2))


TA_MID = (128, 2, 32, 8, 33, 2)
TA_SHORT = (1024, 8, 32, 5, 3, 1)


@pytest.mark.parametrize("kw,case", [
    (dict(bias_variant="transposed"), TA_MID), (dict(bias_variant="next head"), TA_MID), (dict(swap_pairs=True), TA_MID),
    (dict(rot_extra=8), TA_MID), (dict(softmax_len=8), TA_SHORT), (dict(rot_extra=8), (64, 2, 8, 3, 7, 1)),
    (dict(bias_variant="transposed"), (512, 16, 32, 8, 6, 1)), (dict(swap_pairs=True), (256, 2, 128, 8, 5, 1)),
], ids=str)
def test_temporal_attention_variants_are_rejected(kw, case):
    rejected(R.check_temporal_attention, lambda *a: REF["temporal_attention"](*a, **kw), case)


def test_elementwise_variants_are_rejected():
    rejected(R.check_timestep_embedding, lambda *a: REF["timestep_embedding"](*a, swap_halves=True), (256, 1, 0.0))
    rejected(R.check_timestep_embedding, lambda *a: REF["timestep_embedding"](*a, swap_halves=True), (2, 0, 0.0))
    rejected(R.check_timestep_embedding, lambda t, dim, flip, shift: REF["timestep_embedding"](t, dim, flip, 0.0), (320, 1, 1.0))
    rejected(R.check_pack_nhwc, lambda *a: REF["pack_nhwc"](*a, c2_stride_of_c1=True), (2, 4, 3, 3, 1, 8, False, 1.0))
    rejected(R.check_pack_nhwc, lambda s1, s2, c_pad, scale: REF["pack_nhwc"](s1, s2, c_pad, 1.0), (2, 4, 3, 2, 35, 8, True, 2.0))
    rejected(R.check_linear_small, lambda x, w, b, pre, post: REF["linear_small"](x, w, b, post, pre), (3, 520, 5, True, False, True))
    rejected(R.check_linear_small, lambda x, w, b, pre, post: REF["linear_small"](x[:, :512], w[:, :512], b, pre, post),
             (3, 520, 5, False, False, True))                            # the second round of the k loop not taken
    rejected(R.check_unpack_ncthw, lambda src, c, b, t, hw, df, lo, hi: REF["unpack_ncthw"](src, c, b, t, hw, df, *R.NO_CLAMP),
             (True, False, 3, 8, (-1.0, 1.0)))
    rejected(R.check_unpack_ncthw, lambda src, c, b, t, hw, df, lo, hi: REF["unpack_ncthw"](src.reshape(-1)[:src.shape[0] * c].reshape(-1, c),
                                                                                           c, b, t, hw, df, lo, hi),
             (False, True, 3, 8, (-1.0, 1.0)))                           # rows walked with stride c
    rejected(R.check_cast_f32_f16, lambda x: torch.from_numpy(np.where(np.arange(x.numel()) >= x.numel() // 8 * 8, 0, x.numpy())
                                                              .astype(np.float16)), 2049)      # the scalar tail not written
    rejected(R.check_sft_fuse, lambda dec, sc, sh, w, of: REF["sft_fuse"](dec, sc, sh, 1.0, of), 257, True, True)
    rejected(R.check_axpby_f16, lambda x, z, a, b: REF["axpby_f16"](x, z, b, a), 257)


# ---- the defect in the statistics pass is visible ---------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_fp32_sums_of_squares_fail_nearconst_and_pass_randn(f32):
    old, new = R.emulated(R.emulate_gn_sumsq), R.emulated(R.emulate_gn_pivoted)
    base = (64, 0, 64, 32, 1, 4096, False)
    R.check_groupnorm_scale_shift(old, base + ("randn",), f32)
    rejected(R.check_groupnorm_scale_shift, old, base + ("nearconst",), f32)
    for shape in R.GN_SHAPES:
        if shape[1] == 0 and shape[4] <= 3:
            R.check_groupnorm_scale_shift(new, shape, f32)
