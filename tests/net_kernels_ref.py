"""float64 references of the non-GEMM kernels every UNet / VAE layer runs through — GroupNorm and LayerNorm (csrc/norm.hip), per-pixel
temporal attention (csrc/temporal_attn.hip) and the layout, cast and embedding kernels of csrc/elementwise.hip — with the cases and the
pass marks of their edge-shape tests.  The plumbing (judge, worst, measured_bar, ulp16, ulp32, Result, format_record) and the rule for
pass marks are those of tests/small_kernels_ref.py: per element, against the float64 reference, never against the kernel under test.

One `<kernel>_ref` per kernel in numpy float64 from the operation's definition (include/uav_hip.h) and one `check_<kernel>(impl, case)`
that runs `impl` — a callable on CPU tensors: the GPU kernel behind a thin adapter in tests/test_net_kernels_gpu.py, the rounded
reference or a deliberately wrong variant in tests/test_net_kernels_cpu.py — and holds every output element against the reference.

Pass marks.  u = 2^-24.  An fp16 output gets 1/2 ulp16(reference) plus the op's fp32 error term.  Where that term follows from counting
roundings it is stated at the check (casts, hi|lo, pack / unpack, sft_fuse, axpby, the finalize kernels); where it depends on rsqrt,
exp, sin, cos or the summation order it is measured_bar(torch's own fp32 CPU op, float64 reference): 4 x torch's largest error, at least
2^-22 x the magnitude.  The marks of the `offset16`, `nearconst` and `const` data come from that same rule."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from small_kernels_ref import Result, U, f64, format_record, judge, measured_bar, rng, t32, ulp16, ulp32, worst  # noqa: F401

GN_EPS = 1e-6
LN_EPS = 1e-5
H16, F32 = torch.float16, torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
def t16(a):
    """float64 array -> fp16 CPU tensor (one rounding)"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float16)))


def as_np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def eps32(eps):
    return float(np.float32(eps))                    # the fp32 number the C ABI takes


def silu(a):
    return a / (1.0 + np.exp(-a))


def judge_bits(kernel, case, got, want):
    """Bit-exact: same dtype, same shape, the same bits in every element (so -0.0 and the payload of an infinity count)."""
    g, w = as_np(got), as_np(want)
    assert g.dtype == w.dtype and g.shape == w.shape, f"{kernel} {case}: {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
    bits = {2: np.uint16, 4: np.uint32}[g.dtype.itemsize]
    bad = g.view(bits) != w.view(bits)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{kernel} {case}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {i}: "
                             f"got {g[i]!r}, expected {w[i]!r}")
    return Result(kernel, str(case), 0.0, 0.0)


def norm_data(kind, g, shape, eps, offset):
    """The data kinds of the norm kernels, float64 before the rounding to the input type.  `const` is filled in by the caller (what is
    constant — a group or a row — differs)."""
    if kind == "randn":
        return 1.5 * g.standard_normal(shape) + 0.3
    if kind == "offset":
        return offset + g.standard_normal(shape)
    if kind == "nearconst":
        return 0.8 + g.uniform(-1e-3, 1e-3, shape)
    if kind == "tiny":
        return math.sqrt(eps) * g.standard_normal(shape)      # std = sqrt(eps): eps is half of the denominator
    raise ValueError(kind)


def affine(g, c):
    gamma = (1.0 + 0.1 * g.uniform(-1, 1, c)).astype(np.float32)
    beta = (g.choice([-1.0, 1.0], c) * g.uniform(0.05, 0.1, c)).astype(np.float32)
    return gamma, beta


def rounded_rows(a, f32):
    return np.ascontiguousarray(a.astype(np.float32 if f32 else np.float16))


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm: uav_groupnorm_scale_shift + uav_groupnorm_apply on channels-last rows [n_inst * rows][c1 + c2]
# (c1, c2, c_real, groups, n_inst, rows, x2 batch-broadcast, data kind).  256 threads: cvec = c / 8 vectors per row, rpp = 256 / cvec
# rows per pass; a chunk holds 16 passes of rows, capped at 8192 / n_inst chunks.
GN_SHAPES = [
    (8, 0, 8, 1, 1, 1, False, "randn"),             # one vector, rpp = 256, 255 threads without a row; one group over 8 numbers
    (8, 0, 8, 8, 1, 1, False, "randn"),             # cpg = 1 and rows = 1: variance 0, y = beta
    (24, 0, 24, 3, 2, 85, False, "randn"),          # cvec 3, rpp 85: thread 255 idle; exactly one pass
    (24, 0, 24, 3, 2, 86, False, "randn"),          # the second pass holds one row
    (320, 0, 320, 32, 3, 77, False, "randn"),       # cvec 40, rpp 6 (16 idle threads), cpg 10 straddles the 8-channel vectors
    (1280, 640, 1920, 32, 1, 37, False, "randn"),   # cvec 240, rpp 1, cpg 60: group 21 straddles the seam at 1280
    (2048, 0, 2048, 32, 1, 5, False, "randn"),      # the whole LDS array
    (2048, 0, 2048, 2048, 1, 5, False, "randn"),    # groups > 256: a thread writes 8 groups
    (8, 0, 8, 2, 4097, 40, False, "randn"),         # 8192 / 4097 = 1: one chunk per instance, blockIdx.y up to 4096
    (8, 0, 4, 2, 2, 9, False, "randn"),             # padding channels 4..7 (they hold 7.0): scale = shift = 0, y = 0
    (8, 0, 3, 3, 2, 9, False, "randn"),             # c_real 3, cpg 1
    (64, 64, 128, 32, 2, 50, True, "randn"),        # the second source exists once for both instances (x2_rows = half)
]
for _rows in (513, 1025, 4096):                     # cvec 8, rpp 32, 512 rows per chunk: 2, 3 and 8 chunks, the last one ragged or full
    for _kind in ("randn", "offset16", "nearconst", "const", "tiny"):
        GN_SHAPES.append((64, 0, 64, 32, 1, _rows, False, _kind))
GN_RAW_SHAPES = [s for s in GN_SHAPES if s[0] in (320, 1280)]       # apply also writes raw / hi|lo rows there


@functools.lru_cache(maxsize=None)
def gn_input(shape, f32):
    """-> x1, x2 (rounded rows as numpy, x2 None without a second source), X float64 (n_inst, rows, c) as the kernel sees it, gamma, beta."""
    c1, c2, c_real, groups, n_inst, rows, bcast, kind = shape
    c = c1 + c2
    g = rng(31, c1, c2, c_real, groups, n_inst, rows, len(kind), int(f32))
    cpg = c_real // groups
    if kind == "const":
        val = np.where((np.arange(n_inst)[:, None] + np.arange(groups)[None, :]) % 2 == 0, 0.8, 0.1)      # per (instance, group)
        x = np.repeat(val, cpg, axis=1)[:, None, :] + np.zeros((1, rows, 1))
    else:
        x = norm_data("offset" if kind == "offset16" else kind, g, (n_inst, rows, c), GN_EPS, 16.0)
    if c_real < c:
        x[:, :, c_real:] = 7.0
    x = rounded_rows(x.reshape(n_inst * rows, c), f32)
    x1 = np.ascontiguousarray(x[:, :c1])
    x2 = None
    if c2:
        x2 = np.ascontiguousarray(x[:, c1:])
        if bcast:
            x2 = np.ascontiguousarray(x2[:n_inst * rows // 2])
            x = np.concatenate([x1, np.concatenate([x2, x2], axis=0)], axis=1)
    gamma, beta = affine(g, c)
    return x1, x2, x.astype(np.float64).reshape(n_inst, rows, c), gamma, beta


def gn_name(shape, f32):
    c1, c2, c_real, groups, n_inst, rows, bcast, kind = shape
    return (f"c={c1}{'+' + str(c2) if c2 else ''}{' real=' + str(c_real) if c_real != c1 + c2 else ''} G={groups} inst={n_inst} "
            f"rows={rows}{' x2/2' if bcast else ''} {kind} {'fp32' if f32 else 'fp16'}")


def gn_stats_ref(x, c_real, groups, eps, gamma, beta, *, eps_mode="in", unbiased=False, group_of=None, rows_used=None):
    """GroupNorm's tables from X (n_inst, rows, c): per instance and group the mean and BIASED variance over (rows, c_real / groups)
    channels; scale = gamma * rstd, shift = beta - mean * rstd * gamma, rstd = 1 / sqrt(var + eps); channels c_real.. get 0.
    -> scale, shift, magnitude |beta| + |mean * rstd * gamma| of the shift (all (n_inst, c)).
    The keywords build the wrong variants of tests/test_net_kernels_cpu.py."""
    x = f64(x)
    n_inst, rows, c = x.shape
    cpg = c_real // groups
    if group_of is None:
        group_of = np.arange(c_real) // cpg
    if rows_used is not None:
        x = x[:, rows_used]
    ga, be = f64(gamma), f64(beta)
    scale, shift, mag = np.zeros((n_inst, c)), np.zeros((n_inst, c)), np.zeros((n_inst, c))
    if group_of is None or np.array_equal(group_of, np.arange(c_real) // cpg):
        xg = x[:, :, :c_real].reshape(n_inst, x.shape[1], groups, cpg)
        mean = xg.mean(axis=(1, 3))
        ssq = ((xg - mean[:, None, :, None]) ** 2).sum(axis=(1, 3))
        cnt = xg.shape[1] * cpg
    else:
        mean, ssq = np.zeros((n_inst, groups)), np.zeros((n_inst, groups))
        for gi in range(groups):
            xs = x[:, :, :c_real][:, :, group_of == gi]
            mean[:, gi] = xs.mean(axis=(1, 2))
            ssq[:, gi] = ((xs - mean[:, gi, None, None]) ** 2).sum(axis=(1, 2))
        cnt = x.shape[1] * cpg
    var = ssq / ((cnt - 1) if unbiased else cnt)
    rstd = {"in": 1 / np.sqrt(var + eps), "dropped": 1 / np.sqrt(np.maximum(var, 1e-300)), "outside": 1 / (np.sqrt(var) + eps)}[eps_mode]
    gof = np.arange(c_real) // cpg
    m, r = mean[:, gof], rstd[:, gof]
    scale[:, :c_real] = ga[:c_real] * r
    shift[:, :c_real] = be[:c_real] - m * r * ga[:c_real]
    mag[:, :c_real] = np.abs(be[:c_real]) + np.abs(m * r * ga[:c_real])
    return scale, shift, mag


def gn_stats_torch(x, c_real, groups, eps, gamma, beta):
    """torch's own fp32 GroupNorm statistics (native_group_norm's mean and rstd) and the tables formed from them in fp32."""
    n_inst, rows, c = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x[:, :, :c_real].transpose(0, 2, 1))).float()
    _, mean, rstd = torch.native_group_norm(xt, None, None, n_inst, c_real, rows, groups, eps)
    cpg = c_real // groups
    m, r = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    ga, be = torch.from_numpy(gamma[:c_real]), torch.from_numpy(beta[:c_real])
    return (ga * r).numpy(), (be - m * r * ga).numpy()


def check_groupnorm_scale_shift(impl, shape, f32):
    """impl(x1, x2 or None, x2_rows, c_real, n_inst, rows, groups, eps, gamma, beta) -> (scale, shift) fp32 (n_inst, c).
    scale RELATIVE to the reference and shift / (|beta| + |mean rstd gamma|), each by the measured rule against torch's fp32
    native_group_norm (4 x its largest error, at least 2^-22); padding channels exactly 0."""
    c1, c2, c_real, groups, n_inst, rows, bcast, kind = shape
    x1, x2, x, gamma, beta = gn_input(shape, f32)
    eps = eps32(GN_EPS)
    scale, shift = impl(torch.from_numpy(x1), None if x2 is None else torch.from_numpy(x2), x2.shape[0] if bcast else 0, c_real,
                        n_inst, rows, groups, eps, torch.from_numpy(gamma), torch.from_numpy(beta))
    rs, rh, mag = gn_stats_ref(x, c_real, groups, eps, gamma, beta)
    ts, th = gn_stats_torch(x, c_real, groups, eps, gamma, beta)
    name = gn_name(shape, f32)
    rs_, rh_, mag_ = rs[:, :c_real], rh[:, :c_real], mag[:, :c_real]
    one = np.ones_like(rs_)
    res = [judge("groupnorm_scale_shift scale", name + ", relative", f64(scale)[:, :c_real] / rs_, one, measured_bar(ts / rs_, one)),
           judge("groupnorm_scale_shift shift", name + ", over |beta|+|mean rstd gamma|", f64(shift)[:, :c_real] / mag_, rh_ / mag_,
                 measured_bar(th / mag_, rh_ / mag_, magnitude=1.0))]
    if c_real < c1 + c2:
        res.append(judge("groupnorm_scale_shift padding", name, torch.stack([scale, shift])[:, :, c_real:],
                         np.zeros((2, n_inst, c1 + c2 - c_real)), 0.0))
    return worst(res)


def gn_apply_ref(x, scale, shift, silu_on, side="after"):
    """y = act(x * scale + shift) per instance and channel, on the fp32 tables GIVEN (`side`: where the wrong variant puts SiLU)."""
    x = f64(x)
    if side == "before":
        x = silu(x)
    y = x * f64(scale)[:, None, :] + f64(shift)[:, None, :]
    return silu(y) if silu_on and side == "after" else y


def hilo_ref(x32, swapped=False, lo_from_unrounded=False):
    """[hi | lo] rows: hi = fp16(x), lo = fp16(x - hi) (x - hi is exact in fp32)."""
    x32 = np.asarray(x32, dtype=np.float32)
    hi = x32.astype(np.float16)
    lo = ((x32 - hi.astype(np.float32)) if not lo_from_unrounded else (x32 - x32)).astype(np.float16)
    return np.concatenate([lo, hi] if swapped else [hi, lo], axis=-1)


def check_groupnorm_apply(impl, shape, f32, silu_on, raw_mode):
    """impl(x1, x2 or None, x2_rows, n_inst, rows, scale, shift, silu, raw_mode) -> (y fp16 (n_inst * rows, c), raw fp16 or None).
    The tables are the test's own: the float64 reference tables rounded to fp32.  y: 1/2 ulp16(reference) + the measured rule against
    the same expression in torch fp32.  raw_mode 1: raw = fp16(x); 2: [hi | lo]; both bit-exact."""
    c1, c2, c_real, groups, n_inst, rows, bcast, kind = shape
    c = c1 + c2
    x1, x2, x, gamma, beta = gn_input(shape, f32)
    rs, rh, _ = gn_stats_ref(x, c_real, groups, eps32(GN_EPS), gamma, beta)
    scale, shift = t32(rs), t32(rh)
    y, raw = impl(torch.from_numpy(x1), None if x2 is None else torch.from_numpy(x2), x2.shape[0] if bcast else 0, n_inst, rows,
                  scale, shift, silu_on, raw_mode)
    ref = gn_apply_ref(x, scale, shift, silu_on).reshape(n_inst * rows, c)
    t = torch.from_numpy(x).float() * scale[:, None, :] + shift[:, None, :]
    t = (F.silu(t) if silu_on else t).reshape(n_inst * rows, c)
    name = gn_name(shape, f32) + (" silu" if silu_on else "") + ("", " raw", " hilo")[raw_mode]
    assert y.dtype == H16
    res = [judge("groupnorm_apply", name, y, ref, 0.5 * ulp16(ref) + measured_bar(t, ref))]
    x32 = x.reshape(n_inst * rows, c).astype(np.float32)
    if raw_mode == 1:
        res.append(judge_bits("groupnorm_apply raw", name, raw, x32.astype(np.float16)))
    elif raw_mode == 2:
        res.append(judge_bits("groupnorm_apply hi|lo", name, raw, hilo_ref(x32)))
    else:
        assert raw is None
    return worst(res)


# ---- the finalize kernels, fed synthetic partials: per (group, chunk) the float64 sum and sum of squares of random data, rounded once
# to fp32.  Layout [2][groups][chunks_total], the chunks of an instance contiguous.
# (chunks per instance, c, groups, n_inst)
FINALIZE_CASES = [
    (1, 8, 8, 1),               # cpg 1, one chunk: 1023 threads add nothing
    (1023, 8, 2, 3),            # cpg 4; one chunk short of the block
    (1025, 8, 8, 1),            # thread 0 adds a second chunk
    (1, 2048, 1, 3),            # cpg 2048: threads 0..1023 write two channels each
    (1025, 2048, 1, 1),
]
# (chunks, c1, groups1, n_inst1, c2, groups2, n_inst2, groups, n_inst): output cpg = (c1 + c2) / groups
FINALIZE2_CASES = [
    (1, 16, 2, 2, 16, 8, 1, 4, 2),          # cpg 8: source 1 at 1x (cpg 8), source 2 at 4x finer (cpg 2) and once for both instances
    (1025, 16, 4, 2, 16, 2, 2, 4, 2),       # source 1 at 2x finer, source 2 at 1x; groups 2, 3 lie wholly inside source 2
    (1023, 8, 8, 1, 24, 3, 1, 4, 3),        # cpg 8: 8 producer groups of one channel; n_inst 3 over sources that exist once
]
FIN_CHUNK_ROWS = 2


def fin_partials(g, n_inst, chunks, groups, cpg):
    """-> fp32 partials [2][groups][n_inst * chunks] of random data 1.5 N(0,1) + 0.3, FIN_CHUNK_ROWS rows per chunk."""
    d = 1.5 * g.standard_normal((groups, n_inst * chunks, FIN_CHUNK_ROWS * cpg)) + 0.3
    return np.stack([d.sum(axis=2), (d * d).sum(axis=2)]).astype(np.float32)


def fin_tables(s, q, n, eps, gamma, beta):
    """The contract on the partials, in float64: mean = S / n, var = Q / n - mean^2 (>= 0), rstd = 1 / sqrt(var + eps)."""
    mean = s / n
    var = np.maximum(q / n - mean * mean, 0.0)
    rstd = 1 / np.sqrt(var + eps)
    ga, be = f64(gamma), f64(beta)
    return ga * rstd, be - mean * rstd * ga, np.abs(be) + np.abs(mean * rstd * ga)


def finalize_ref(partials, chunks, c, n_inst, groups, eps, gamma, beta):
    p = f64(partials).reshape(2, groups, n_inst, chunks).sum(axis=3)                  # (2, groups, n_inst)
    cpg = c // groups
    s, q = (np.repeat(p[i].T, cpg, axis=1) for i in (0, 1))                           # (n_inst, c)
    return fin_tables(s, q, float(chunks * FIN_CHUNK_ROWS * cpg), eps, gamma, beta)


def fin_judge(kernel, name, scale, shift, rs, rh, mag):
    """Counting: the kernel rounds mean and rstd to fp32 (1/2 ulp each, relative), then scale = gamma * rstd (one product) and
    shift = beta - mean * rstd * gamma (two products and a difference): scale within 2 ulp32, shift within 4 ulp32 of
    |beta| + |mean rstd gamma|.  Its fp64 sums differ from the reference's by the order of addition only."""
    return worst([judge(kernel + " scale", name, scale, rs, 2 * ulp32(rs)), judge(kernel + " shift", name, shift, rh, 4 * ulp32(mag))])


def check_finalize_partials(impl, case):
    """impl(partials fp32 [2][groups][chunks_total], chunk_rows, c, n_inst, rows, groups, eps, gamma, beta) -> (scale, shift)."""
    chunks, c, groups, n_inst = case
    g = rng(32, *case)
    part = fin_partials(g, n_inst, chunks, groups, c // groups)
    gamma, beta = affine(g, c)
    eps = eps32(GN_EPS)
    scale, shift = impl(torch.from_numpy(part), FIN_CHUNK_ROWS, c, n_inst, chunks * FIN_CHUNK_ROWS, groups, eps,
                        torch.from_numpy(gamma), torch.from_numpy(beta))
    return fin_judge("groupnorm_finalize_partials", f"chunks={chunks} c={c} G={groups} inst={n_inst}", scale, shift,
                     *finalize_ref(part, chunks, c, n_inst, groups, eps, gamma, beta))


def finalize2_ref(p1, p2, case, eps, gamma, beta):
    chunks, c1, g1, n1, c2, g2, n2, groups, n_inst = case
    c = c1 + c2
    cpg = c // groups
    s, q = np.zeros((n_inst, c)), np.zeros((n_inst, c))
    for inst in range(n_inst):
        for go in range(groups):
            ch0 = go * cpg
            part, cs, gs, ns, off = (p1, c1, g1, n1, ch0) if ch0 < c1 else (p2, c2, g2, n2, ch0 - c1)
            cpgs = cs // gs
            k, pg0, si = cpg // cpgs, off // cpgs, inst % ns
            v = f64(part).reshape(2, gs, ns, chunks)[:, pg0:pg0 + k, si, :].sum(axis=(1, 2))
            s[inst, ch0:ch0 + cpg], q[inst, ch0:ch0 + cpg] = v[0], v[1]
    return fin_tables(s, q, float(chunks * FIN_CHUNK_ROWS * cpg), eps, gamma, beta)


def check_finalize_partials2(impl, case):
    """impl(p1, c1, groups1, n_inst1, p2, c2, groups2, n_inst2, chunk_rows, n_inst, rows, groups, eps, gamma, beta) -> (scale, shift):
    an output group is the sum of cpg / cpg_source consecutive producer groups of the source it lies in; instance i reads the chunks
    of instance i % n_inst_source."""
    chunks, c1, g1, n1, c2, g2, n2, groups, n_inst = case
    g = rng(33, *case)
    p1 = fin_partials(g, n1, chunks, g1, c1 // g1)
    p2 = fin_partials(g, n2, chunks, g2, c2 // g2)
    gamma, beta = affine(g, c1 + c2)
    eps = eps32(GN_EPS)
    scale, shift = impl(torch.from_numpy(p1), c1, g1, n1, torch.from_numpy(p2), c2, g2, n2, FIN_CHUNK_ROWS, n_inst,
                        chunks * FIN_CHUNK_ROWS, groups, eps, torch.from_numpy(gamma), torch.from_numpy(beta))
    name = f"chunks={chunks} c={c1}/{g1}x{n1}+{c2}/{g2}x{n2} G={groups} inst={n_inst}"
    return fin_judge("groupnorm_finalize_partials2", name, scale, shift, *finalize2_ref(p1, p2, case, eps, gamma, beta))


# ---- numpy emulations of the statistics pass in the kernel's own fp32 order (CPU only: they show what the cases can see)
def _gn_chunks(n_inst, rows, c):
    rpp = 256 // (c // 8)
    return max(1, min(-(-rows // (rpp * 16)), max(8192 // n_inst, 1), 2048))


def emulate_gn_sumsq(x, f32, c_real, groups, eps, gamma, beta):
    """The statistics pass with plain fp32 sums of x and x * x per thread (the form before the pivoted sums; the conv epilogue's fused
    partials keep it): thread (row lane, channel) adds its rows in order, the row lanes are added in order, then the channels of a
    group; the finalize pass adds the chunks in fp64 and takes var = Q / n - mean^2."""
    n_inst, rows, c = x.shape
    x = x.astype(np.float32)
    rpp, chunks, cpg = 256 // (c // 8), _gn_chunks(n_inst, rows, c), c_real // groups
    rpc = -(-rows // chunks)
    s_tot, q_tot = np.zeros((n_inst, groups)), np.zeros((n_inst, groups))
    for k in range(chunks):
        xc = x[:, k * rpc:(k + 1) * rpc]
        pad = (-xc.shape[1]) % rpp
        xc = np.concatenate([xc, np.zeros((n_inst, pad, c), np.float32)], axis=1).reshape(n_inst, -1, rpp, c)
        sm, sq = np.zeros((n_inst, rpp, c), np.float32), np.zeros((n_inst, rpp, c), np.float32)
        for i in range(xc.shape[1]):
            sm = sm + xc[:, i]
            sq = sq + xc[:, i] * xc[:, i]
        cs, cq = np.zeros((n_inst, c), np.float32), np.zeros((n_inst, c), np.float32)
        for r in range(rpp):
            cs, cq = cs + sm[:, r], cq + sq[:, r]
        gs, gq = np.zeros((n_inst, groups), np.float32), np.zeros((n_inst, groups), np.float32)
        for j in range(cpg):
            gs, gq = gs + cs[:, j:c_real:cpg], gq + cq[:, j:c_real:cpg]
        s_tot += gs
        q_tot += gq
    n = float(rows * cpg)
    mean = s_tot / n
    var = np.maximum(q_tot / n - mean * mean, 0)
    fm, fr = mean.astype(np.float32), (1 / np.sqrt(var + eps)).astype(np.float32)
    ga, be = gamma[:c_real], beta[:c_real]
    fm, fr = np.repeat(fm, cpg, 1), np.repeat(fr, cpg, 1)
    scale, shift = np.zeros((n_inst, c), np.float32), np.zeros((n_inst, c), np.float32)
    scale[:, :c_real] = ga * fr
    shift[:, :c_real] = be - fm * fr * ga
    return torch.from_numpy(scale), torch.from_numpy(shift)


def emulate_gn_pivoted(x, f32, c_real, groups, eps, gamma, beta):
    """ILLUSTRATION ONLY, kept in step with csrc/norm.hip by hand: it shows on the CPU that the method meets the marks of all five data
    kinds and says nothing about the GPU code (tests/test_net_kernels_gpu.py does).  The statistics pass as csrc/norm.hip has it: per
    chunk, row lane and channel fp32 sums of x - p and (x - p)^2 about the chunk's first row p; row lanes, channels of a group and
    chunks merged in fp64, a chunk's sum handed on as hi + lo and its M2 as one fp32."""
    n_inst, rows, c = x.shape
    x = x.astype(np.float32)
    rpp, chunks, cpg = 256 // (c // 8), _gn_chunks(n_inst, rows, c), c_real // groups
    chunks = min(chunks, 2048 * 2 * c // (3 * groups))
    rpc = -(-rows // chunks)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    parts = []
    for k in range(chunks):
        xc = x[:, k * rpc:(k + 1) * rpc]
        nr = xc.shape[1]
        if nr == 0:
            continue
        pv = xc[:, 0]
        pad = (-nr) % rpp
        xc = np.concatenate([xc, np.repeat(pv[:, None], pad, axis=1)], axis=1).reshape(n_inst, -1, rpp, c)
        sm, sq = np.zeros((n_inst, rpp, c), np.float32), np.zeros((n_inst, rpp, c), np.float32)
        for i in range(xc.shape[1]):
            f = xc[:, i] - pv[:, None]
            sm, sq = sm + f, sq + f * f
        cs, cq = sm.astype(np.float64).sum(axis=1), sq.astype(np.float64).sum(axis=1)
        d = cs / nr
        mk = (pv.astype(np.float64) + d)[:, :c_real].reshape(n_inst, groups, cpg)
        m2 = r32(np.maximum(cq - cs * d, 0))[:, :c_real].reshape(n_inst, groups, cpg)
        mg = mk.sum(axis=2) / cpg
        total = nr * mk.sum(axis=2)
        hi = r32(total)
        parts.append((nr * cpg, hi + r32(total - hi), r32((m2 + nr * (mk - mg[:, :, None]) ** 2).sum(axis=2))))
    n = float(rows * cpg)
    mean = sum(p[1] for p in parts) / n
    m2 = sum(p[2] + p[0] * (p[1] / p[0] - mean) ** 2 for p in parts)
    rstd = 1 / np.sqrt(m2 / n + eps)
    ga, be = gamma[:c_real], beta[:c_real]
    scale, shift = np.zeros((n_inst, c), np.float32), np.zeros((n_inst, c), np.float32)
    sc = (ga.astype(np.float64) * np.repeat(rstd, cpg, 1)).astype(np.float32)
    scale[:, :c_real] = sc
    shift[:, :c_real] = (be.astype(np.float64) - np.repeat(mean, cpg, 1) * sc.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(scale), torch.from_numpy(shift)


def emulated(emulation):
    """An emulation behind the signature of the scale/shift op."""
    def impl(x1, x2, x2_rows, c_real, n_inst, rows, groups, eps, gamma, beta):
        assert x2 is None
        return emulation(x1.numpy().reshape(n_inst, rows, -1), x1.dtype == F32, c_real, groups, eps, gamma.numpy(), beta.numpy())
    return impl


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm: uav_layernorm_f16 / uav_layernorm_f32in.  One wave per row, NV = ceil(c / 512) vectors per lane, 4 waves per block,
# at most 4096 blocks = 16384 rows before the grid-stride second pass.
LN_CASES = [(rows, c, "randn") for c in (8, 520, 1024, 1536, 2048) for rows in (1, 3, 5, 777)]
#   c = 8: 63 idle lanes; 520: NV 2, the second vector in lane 0 alone; 1024: NV 2 full; 1536: NV 3; 2048: NV 4.
#   rows 1, 3: a block with idle waves; 5: a second block of one wave
LN_CASES += [(16390, 8, "randn"), (16387, 520, "randn")]                     # waves 0..5 / 0..2 take a second row
LN_CASES += [(777, 520, k) for k in ("offset", "nearconst", "const", "tiny")]


@functools.lru_cache(maxsize=None)
def ln_input(case, f32):
    rows, c, kind = case
    g = rng(34, rows, c, len(kind), int(f32))
    if kind == "const":
        x = np.where(np.arange(rows)[:, None] % 2 == 0, 0.8, 0.1) + np.zeros((1, c))
    else:
        x = norm_data(kind, g, (rows, c), LN_EPS, 50.0)
    gamma, beta = affine(g, c)
    return rounded_rows(x, f32), gamma, beta


def layernorm_ref(x, gamma, beta, eps, *, eps_mode="in", unbiased=False):
    """(x - mean) / sqrt(BIASED var + eps) * gamma + beta over the last axis."""
    x = f64(x)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).sum(axis=1, keepdims=True) / (x.shape[1] - (1 if unbiased else 0))
    rstd = {"in": 1 / np.sqrt(var + eps), "dropped": 1 / np.sqrt(np.maximum(var, 1e-300)), "outside": 1 / (np.sqrt(var) + eps)}[eps_mode]
    return (x - mean) * rstd * f64(gamma) + f64(beta)


def check_layernorm(impl, case, f32):
    """impl(x rows fp16 or fp32, gamma, beta, eps) -> y fp16.  1/2 ulp16(reference) + the measured rule against F.layer_norm in fp32."""
    rows, c, kind = case
    x, gamma, beta = ln_input(case, f32)
    eps = eps32(LN_EPS)
    y = impl(torch.from_numpy(x), torch.from_numpy(gamma), torch.from_numpy(beta), eps)
    ref = layernorm_ref(x, gamma, beta, eps)
    t = F.layer_norm(torch.from_numpy(x).float(), (c,), torch.from_numpy(gamma), torch.from_numpy(beta), eps)
    assert y.dtype == H16
    return judge("layernorm_f32in" if f32 else "layernorm_f16", f"rows={rows} c={c} {kind}", y, ref, 0.5 * ulp16(ref) + measured_bar(t, ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# temporal attention: uav_temporal_attention_f16 on the fused projection rows [(b * T + t) * hw + p][3c] = [q | k | v].
# One wave per (pixel, 512-channel group), lane = 8 channels, LPH = d / 8 lanes per head.
# (c, heads, rot_dim, T, hw, n_batch)
TATTN_CASES = [
    (8, 1, 8, 8, 1, 1),             # LPH 1; rot_dim == d; one pixel: 3 idle waves, 63 dead lanes
    (32, 2, 0, 2, 5, 2),            # LPH 2; no rotary dims, no tables; T = 2
    (64, 2, 8, 3, 7, 1),            # LPH 4; the first lane of a head rotates, the other three do not
    (128, 2, 32, 8, 33, 2),         # LPH 8; 9 blocks, the last one wave
    (1024, 8, 32, 5, 3, 1),         # LPH 16; two full 512-channel groups
    (768, 3, 32, 8, 2, 1),          # LPH 32; group 1 holds 256 channels: 32 dead lanes
    (512, 1, 32, 4, 2, 1),          # LPH 64
    (64, 1, 32, 1, 9, 1),           # T = 1: the softmax is 1, the output v bit for bit
    (512, 16, 32, 8, 6, 1),         # heads * T * T = 1024 > 512: the round-1 kernel (tables read from global memory)
    (256, 2, 128, 8, 5, 1),         # T * rot_dim / 2 = 512 > 256: the round-1 kernel, rot_dim == d
]


def rope_tables(t_len, rot_dim):
    """cos / sin [T][rot_dim / 2] in fp32, as RotaryEmbedding(rot_dim) forms them: angle t / 10000^(2 i / rot_dim)."""
    if rot_dim == 0:
        return np.zeros((t_len, 0), np.float32), np.zeros((t_len, 0), np.float32)
    freqs = (1.0 / (10000 ** (torch.arange(0, rot_dim, 2).float() / rot_dim)))
    ang = torch.arange(t_len).float()[:, None] * freqs[None]
    return ang.cos().numpy(), ang.sin().numpy()


@functools.lru_cache(maxsize=None)
def tattn_input(case):
    c, heads, rot, t_len, hw, nb = case
    g = rng(35, *case)
    qkv = g.standard_normal((nb * t_len * hw, 3 * c)).astype(np.float16)
    bias = (0.5 * g.standard_normal((heads, t_len, t_len))).astype(np.float32)
    cos, sin = rope_tables(t_len, rot)
    return qkv, bias, cos, sin, float(np.float32((c // heads) ** -0.5))


def rope(x, cos, sin, rot, swap_pairs=False):
    """x (..., T, d): the first `rot` dims as interleaved pairs (a, b) -> (a cos - b sin, b cos + a sin), angle of token t, pair i."""
    if rot == 0:
        return x
    out = x.copy()
    a, b = x[..., 0:rot:2], x[..., 1:rot:2]
    if swap_pairs:
        a, b = b, a
    ra, rb = a * cos - b * sin, b * cos + a * sin
    out[..., 0:rot:2], out[..., 1:rot:2] = (rb, ra) if swap_pairs else (ra, rb)
    return out


def tattn_ref(qkv, bias, cos, sin, scale, case, *, rounded=False, bias_variant=None, swap_pairs=False, rot_extra=0, softmax_len=None):
    """The definition in include/uav_hip.h: q * scale -> RoPE on the first rot_dim dims of each head -> + bias[h][i][j] -> softmax over
    the T tokens of the pixel -> V.  rounded: the rotated q and k rounded to fp16, the kernel's two documented roundings.
    -> out (rows, c), and for the bar: sum_j p_ij |v_j| (rows, c) and sum_e |q_ie| |k_je| maximised over j (b, p, h, T)."""
    c, heads, rot, t_len, hw, nb = case
    d = c // heads
    x = f64(qkv).reshape(nb, t_len, hw, 3, heads, d).transpose(3, 0, 2, 4, 1, 5)                       # (3, b, p, h, t, d)
    cs, sn = f64(cos), f64(sin)                                                                        # (T, rot / 2)
    if rot_extra:                                                                                      # wrong variant: rot + 8 dims
        cs = np.concatenate([cs, cs[:, :rot_extra // 2]], axis=1)
        sn = np.concatenate([sn, sn[:, :rot_extra // 2]], axis=1)
    q = rope(x[0] * scale, cs, sn, rot + rot_extra, swap_pairs)
    k = rope(x[1], cs, sn, rot + rot_extra, swap_pairs)
    v = x[2]
    if rounded:
        q, k = q.astype(np.float16).astype(np.float64), k.astype(np.float16).astype(np.float64)
    b = f64(bias)
    if bias_variant == "transposed":
        b = b.transpose(0, 2, 1)
    elif bias_variant == "next head":
        b = np.roll(b, -1, axis=0)
    s = q @ k.transpose(0, 1, 2, 4, 3) + b[None, None]
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    den = e.sum(axis=-1, keepdims=True)
    if softmax_len is not None:                                                                        # wrong variant: 8 - T more
        den = den + (softmax_len - t_len) * np.exp(0.0 - s.max(axis=-1, keepdims=True))                # tokens of score 0, v = 0
    p = e / den
    back = lambda a: a.transpose(0, 3, 1, 2, 4).reshape(nb * t_len * hw, c)                            # (b, p, h, t, d) -> rows
    qk = (np.abs(q) @ np.abs(k).transpose(0, 1, 2, 4, 3)).max(axis=-1)                                 # (b, p, h, t)
    return back(p @ v), back(p @ np.abs(v)), qk


@functools.lru_cache(maxsize=None)
def tattn_marks(case):
    """-> reference, per-element bar, and the rms error of the twice-rounded float64 evaluation (output rounded to fp16) against the
    reference: the error the documented roundings alone cause."""
    qkv, bias, cos, sin, scale = tattn_input(case)
    c, heads, rot, t_len, hw, nb = case
    d = c // heads
    ref, pv, qk = tattn_ref(qkv, bias, cos, sin, scale, case)
    delta = (2.0 ** -10 + 2.0 ** -22 + (d + 8) * U) * qk                                               # (b, p, h, t)
    delta = np.repeat(delta.transpose(0, 3, 1, 2)[..., None], d, axis=-1).reshape(nb * t_len * hw, c)
    bar = (np.exp(2 * delta) - 1) * pv + 0.5 * ulp16(ref) + 16 * U * pv
    rounded = f64(t16(tattn_ref(qkv, bias, cos, sin, scale, case, rounded=True)[0]))
    return ref, bar, float(np.sqrt(np.mean((rounded - ref) ** 2)))


def check_temporal_attention(impl, case):
    """impl(qkv fp16 rows, n_batch, T, hw, c, heads, scale, cos, sin, rot_dim, bias) -> out fp16 (rows, c).
    1. per element: |err| <= (exp(2 delta_i) - 1) sum_j p_ij |v_j| + 1/2 ulp16(ref) + 16 u sum_j p_ij |v_j|, where
       delta_i = max_j (2^-10 + 2^-22 + (d + 8) u) sum_e |q_ie| |k_je| bounds the change of a score by the fp16 rounding of the
       rotated q and k (2^-11 each, their product 2^-22) and the fp32 dot product of d terms, reduction and bias addition;
    2. per case: the rms error is at most 2 x the rms error of the float64 evaluation with exactly those two roundings.
    T = 1: the output is v, bit for bit."""
    c, heads, rot, t_len, hw, nb = case
    qkv, bias, cos, sin, scale = tattn_input(case)
    out = impl(torch.from_numpy(qkv), nb, t_len, hw, c, heads, scale, torch.from_numpy(cos), torch.from_numpy(sin), rot,
               torch.from_numpy(bias))
    name = f"c={c} heads={heads} rot={rot} T={t_len} hw={hw} b={nb}"
    assert out.dtype == H16
    if t_len == 1:
        return judge_bits("temporal_attention", name + " (= v)", out, qkv[:, 2 * c:])
    ref, bar, rms_rounded = tattn_marks(case)
    res = judge("temporal_attention", name, out, ref, bar)
    rms = float(np.sqrt(np.mean((f64(out) - ref) ** 2)))
    r2 = Result("temporal_attention rms", name, rms, 2 * rms_rounded)
    assert rms <= r2.bar, f"temporal_attention {name}: rms error {rms:.3e} over 2 x {rms_rounded:.3e}, the documented roundings' own"
    return worst([res, r2])


# ---------------------------------------------------------------------------------------------------------------------------------
# elementwise: uav_linear_small.  One wave per output column, lane = 8 consecutive k (a second round past k = 512), MMAX 2 or 16.
LINEAR_CASES = []
for _i, (_m, _k, _n) in enumerate((m, k, n) for m in (1, 2, 3, 16) for k in (8, 520, 1280) for n in (1, 5, 1024)):
    LINEAR_CASES.append((_m, _k, _n, bool(_i & 1), bool(_i & 2), True))             # (m, k, n, pre-SiLU, post-SiLU, bias)
LINEAR_CASES += [(3, 520, 5, pre, post, True) for pre in (False, True) for post in (False, True)] + [(2, 520, 5, True, True, False)]


def linear_small_ref(x, w, b, pre, post):
    x = f64(x)
    y = (silu(x) if pre else x) @ f64(w).T + (0.0 if b is None else f64(b))
    return silu(y) if post else y


def check_linear_small(impl, case):
    """impl(x fp32 (m, k), w fp16 (n, k), b fp32 (n) or None, pre, post) -> y fp32 (m, n).  Measured rule (the order of the k sum,
    expf in SiLU) against the same expression in torch fp32."""
    m, k, n, pre, post, has_b = case
    g = rng(36, m, k, n, int(pre), int(post), int(has_b))
    x = g.standard_normal((m, k)).astype(np.float32)
    w = (g.standard_normal((n, k)) / math.sqrt(k)).astype(np.float16)
    b = g.standard_normal(n).astype(np.float32) if has_b else None
    y = impl(torch.from_numpy(x), torch.from_numpy(w), None if b is None else torch.from_numpy(b), pre, post)
    ref = linear_small_ref(x, w, b, pre, post)
    xt = torch.from_numpy(x)
    t = (F.silu(xt) if pre else xt) @ torch.from_numpy(w).float().T
    t = t if b is None else t + torch.from_numpy(b)
    t = F.silu(t) if post else t
    name = f"m={m} k={k} n={n}" + (" pre" if pre else "") + (" post" if post else "") + ("" if has_b else " no bias")
    return judge("linear_small", name, y, ref, measured_bar(t, ref))


# ---- uav_timestep_embedding: one thread per (row, frequency)
TIMESTEPS = np.array([0.0, 0.5, 34.0, 999.0], dtype=np.float32)
TEMB_CASES = [(dim, flip, shift) for dim in (2, 256, 320) for flip in (0, 1) for shift in (0.0, 1.0)]


def timestep_embedding_ref(t, dim, flip, shift, swap_halves=False):
    """diffusers get_timestep_embedding: arg = t * exp(-ln(10000) * j / (dim / 2 - shift)); [sin | cos], flip_sin_to_cos: [cos | sin].
    dim = 2 with shift 1 divides 0 by 0: the row is nan there as in diffusers."""
    half = dim // 2
    with np.errstate(divide="ignore", invalid="ignore"):
        arg = f64(t)[:, None] * np.exp(-math.log(10000.0) * np.arange(half) / (half - shift))[None]
    sn, cs = np.sin(arg), np.cos(arg)
    return np.concatenate([cs, sn] if bool(flip) != swap_halves else [sn, cs], axis=1)


def check_timestep_embedding(impl, case):
    """impl(t fp32 (m), dim, flip, freq_shift) -> fp32 (m, dim).  Measured rule (logf, expf, the fp32 argument of sinf / cosf at
    t = 999) against the same expression in torch fp32; an element the definition leaves nan must be nan."""
    dim, flip, shift = case
    out = impl(torch.from_numpy(TIMESTEPS), dim, flip, shift)
    ref = timestep_embedding_ref(TIMESTEPS, dim, flip, shift)
    name = f"dim={dim} flip={flip} shift={shift:g}"
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(f64(out)), nan), f"timestep_embedding {name}: nan where the definition has none, or the reverse"
    if nan.all():
        return Result("timestep_embedding", name + " (0/0: nan)", 0.0, 0.0)
    half = dim // 2
    tt = torch.from_numpy(TIMESTEPS)
    arg = tt[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / (half - shift))[None]
    t = torch.cat([arg.cos(), arg.sin()] if flip else [arg.sin(), arg.cos()], dim=1)
    keep = ~nan
    return judge("timestep_embedding", name, np.where(keep, f64(out), 0.0), np.where(keep, ref, 0.0),
                 measured_bar(np.where(keep, f64(t), 0.0), np.where(keep, ref, 0.0)))


# ---- uav_pack_nhwc: (B, C, T, H, W) [+ a second tensor] -> fp16 rows [B T hw][c_pad]; one thread per row
# (n_batch, c1, c2, T, hw, c_pad, fp32 source, scale)
PACK_CASES = [
    (2, 4, 3, 3, 1, 8, False, 1.0),         # 4 + 3 -> 8: one padding channel; hw = 1
    (1, 4, 0, 1, 257, 16, False, 1.0),      # 4 -> 16: the second vector is all padding; 257 rows: a second block of one thread
    (2, 4, 3, 2, 35, 8, True, 2.0),         # fp32 source, scale 2 (exact)
    (1, 4, 3, 1, 257, 8, True, 2.0),
]


def pack_nhwc_ref(s1, s2, c_pad, scale, c2_stride_of_c1=False):
    """fp16(scale * x) per element (the product is exact for the powers of two used), channels c1 + c2.. zero."""
    b, c1, t, hw = s1.shape
    out = np.zeros((b, t, hw, c_pad), np.float32)
    out[..., :c1] = np.asarray(s1, np.float32).transpose(0, 2, 3, 1)
    if s2 is not None:
        c2 = s2.shape[1]
        v = np.asarray(s2, np.float32)
        if c2_stride_of_c1:                  # wrong variant: batch b of the second tensor found with the first one's channel count
            v = np.concatenate([v.reshape(-1), np.zeros(b * (c1 - c2) * t * hw, np.float32)])[:b * c1 * t * hw].reshape(b, c1, t, hw)[:, :c2]
        out[..., c1:c1 + c2] = v.transpose(0, 2, 3, 1)
    return (out * np.float32(scale)).astype(np.float16).reshape(b * t * hw, c_pad)


def check_pack_nhwc(impl, case):
    """impl(src1 (B, c1, T, hw), src2 or None, c_pad, scale) -> fp16 rows.  Bit-exact."""
    b, c1, c2, t, hw, c_pad, f32, scale = case
    g = rng(37, b, c1, c2, t, hw, c_pad, int(f32))
    dt = np.float32 if f32 else np.float16
    s1 = g.standard_normal((b, c1, t, hw)).astype(dt)
    s2 = g.standard_normal((b, c2, t, hw)).astype(dt) if c2 else None
    out = impl(torch.from_numpy(s1), None if s2 is None else torch.from_numpy(s2), c_pad, scale)
    return judge_bits("pack_nhwc", f"b={b} c={c1}+{c2}->{c_pad} T={t} hw={hw} {'fp32' if f32 else 'fp16'} x{scale:g}", out,
                      pack_nhwc_ref(s1, s2, c_pad, scale))


# ---- uav_unpack_ncthw: rows [B T hw][src_stride] -> (B, c, T, hw), clamped
NO_CLAMP = (-3.0e38, 3.0e38)
# (src fp32, dst fp32, c, src_stride, clamp)
UNPACK_CASES = [(sf, df, 3, st, cl) for sf in (False, True) for df in (False, True) for st, cl in ((3, None), (8, (-1.0, 1.0)))]
UNPACK_GEOM = (2, 3, 43)                    # n_batch, T, hw: 258 rows, two threads in a second block


def unpack_ncthw_ref(src, c, b, t, hw, dst_f32, lo, hi):
    v = np.asarray(src, np.float32)[:, :c]
    v = np.minimum(np.maximum(v, np.float32(lo)), np.float32(hi))
    return np.ascontiguousarray(v.reshape(b, t, hw, c).transpose(0, 3, 1, 2)).astype(np.float32 if dst_f32 else np.float16)


def check_unpack_ncthw(impl, case):
    """impl(src rows (B T hw, src_stride), c, B, T, hw, dst fp32?, lo, hi) -> (B, c, T, hw).  Bit-exact: a clamp and one rounding."""
    sf, df, c, stride, clamp = case
    b, t, hw = UNPACK_GEOM
    g = rng(38, int(sf), int(df), stride)
    src = (1.5 * g.standard_normal((b * t * hw, stride))).astype(np.float32 if sf else np.float16)
    lo, hi = clamp or NO_CLAMP
    out = impl(torch.from_numpy(src), c, b, t, hw, df, lo, hi)
    name = f"{'fp32' if sf else 'fp16'}->{'fp32' if df else 'fp16'} stride={stride} clamp={'on' if clamp else 'off'}"
    return judge_bits("unpack_ncthw", name, out, unpack_ncthw_ref(src, c, b, t, hw, df, lo, hi))


# ---- casts: 8 elements per thread
CAST_N = [1, 7, 8, 2049]                    # scalar tail only; 7 of 8; one vector; 2 blocks, the last thread a tail of 1
HILO_CASES = [(1, 8), (33, 320)]


def wide_values(g, shape):
    """Magnitudes log-uniform in [1e-6, 6e4], random signs: fp16 subnormals, normals and the last binade below the overflow."""
    return (g.choice([-1.0, 1.0], shape) * np.exp(g.uniform(math.log(1e-6), math.log(6e4), shape))).astype(np.float32)


def check_cast_f32_f16(impl, n):
    """impl(x fp32 (n)) -> fp16 (n).  One rounding to nearest even: bit-exact against numpy's astype."""
    x = wide_values(rng(39, n), n)
    return judge_bits("cast_f32_f16", f"n={n}", impl(torch.from_numpy(x)), x.astype(np.float16))


def check_cast_f32_hilo(impl, case):
    """impl(x fp32 (rows, c)) -> fp16 (rows, 2c) = [hi | lo].  Bit-exact against numpy; and hi + lo reproduces x to
    max(2^-22 |x|, 2^-25): |x - hi| <= 2^-11 |x| and lo rounds it with another 2^-11, unless lo is an fp16 subnormal, whose spacing is
    2^-24."""
    rows, c = case
    x = wide_values(rng(40, rows, c), (rows, c))
    out = impl(torch.from_numpy(x))
    name = f"rows={rows} c={c}"
    res = [judge_bits("cast_f32_hilo", name, out, hilo_ref(x))]
    o = f64(out)
    res.append(judge("cast_f32_hilo hi+lo", name, o[:, :c] + o[:, c:], f64(x), np.maximum(2.0 ** -22 * np.abs(f64(x)), 2.0 ** -25)))
    return worst(res)


# ---- uav_sft_fuse, uav_axpby_f16: one thread per element
POINTWISE_N = [1, 257]
SFT_W = 0.75


def check_sft_fuse(impl, n, in_f32, out_f32):
    """impl(dec, scale, shift, w, out fp32?) -> dec + w (dec * scale + shift).  Two products and two sums in fp32, at most four
    roundings of at most 2^-24 (|dec| + |w| (|dec scale| + |shift|)) each; an fp16 output adds 1/2 ulp16(reference)."""
    g = rng(41, n, int(in_f32))
    dec, sc, sh = (g.standard_normal(n).astype(np.float32 if in_f32 else np.float16) for _ in range(3))
    w = eps32(SFT_W)
    out = impl(torch.from_numpy(dec), torch.from_numpy(sc), torch.from_numpy(sh), w, out_f32)
    d, s, h = f64(dec), f64(sc), f64(sh)
    ref = d + w * (d * s + h)
    bar = 4 * U * (np.abs(d) + abs(w) * (np.abs(d * s) + np.abs(h)))
    assert out.dtype == (F32 if out_f32 else H16)
    return judge("sft_fuse", f"n={n} {'fp32' if in_f32 else 'fp16'}->{'fp32' if out_f32 else 'fp16'}", out, ref,
                 bar if out_f32 else bar + 0.5 * ulp16(ref))


def check_axpby_f16(impl, n):
    """impl(x fp16, z fp16, a, b) -> fp16(a x + b z).  Two products and a sum in fp32: 3 roundings of at most 2^-24 (|a x| + |b z|);
    plus 1/2 ulp16(reference)."""
    g = rng(42, n)
    x, z = g.standard_normal(n).astype(np.float16), g.standard_normal(n).astype(np.float16)
    a, b = eps32(0.7), eps32(-1.3)
    out = impl(torch.from_numpy(x), torch.from_numpy(z), a, b)
    ref = a * f64(x) + b * f64(z)
    assert out.dtype == H16
    return judge("axpby_f16", f"n={n}", out, ref, 3 * U * (np.abs(a * f64(x)) + np.abs(b * f64(z))) + 0.5 * ulp16(ref))


# ---------------------------------------------------------------------------------------------------------------------------------
def all_cases():
    """[(id, kernel key, check, arguments)]: every case of every kernel, the list both test files run.  `check(impls[key], *arguments)`."""
    out = []

    def add(key, check, *args):
        out.append((f"{key}-" + "-".join(str(a).replace(" ", "") for a in args), key, check, args))
    for f32 in (False, True):
        for s in GN_SHAPES:
            add("gn_scale_shift", check_groupnorm_scale_shift, s, f32)
            for silu_on in (False, True):
                add("gn_apply", check_groupnorm_apply, s, f32, silu_on, 0)
        for s in GN_RAW_SHAPES:
            for raw_mode in (1, 2):
                add("gn_apply", check_groupnorm_apply, s, f32, True, raw_mode)
    for c in FINALIZE_CASES:
        add("gn_finalize_partials", check_finalize_partials, c)
    for c in FINALIZE2_CASES:
        add("gn_finalize_partials2", check_finalize_partials2, c)
    for f32 in (False, True):
        for c in LN_CASES:
            add("layernorm", check_layernorm, c, f32)
    for c in TATTN_CASES:
        add("temporal_attention", check_temporal_attention, c)
    for c in LINEAR_CASES:
        add("linear_small", check_linear_small, c)
    for c in TEMB_CASES:
        add("timestep_embedding", check_timestep_embedding, c)
    for c in PACK_CASES:
        add("pack_nhwc", check_pack_nhwc, c)
    for c in UNPACK_CASES:
        add("unpack_ncthw", check_unpack_ncthw, c)
    for n in CAST_N:
        add("cast_f32_f16", check_cast_f32_f16, n)
    for c in HILO_CASES:
        add("cast_f32_hilo", check_cast_f32_hilo, c)
    for n in POINTWISE_N:
        for in_f32 in (False, True):
            for out_f32 in (False, True):
                add("sft_fuse", check_sft_fuse, n, in_f32, out_f32)
        add("axpby_f16", check_axpby_f16, n)
    return out


def gn_logical(x1, x2, x2_rows, n_inst, rows):
    """The (n_inst, rows, c) float64 tensor the GroupNorm kernels see behind their two pointers."""
    a = f64(x1)
    if x2 is not None:
        b = f64(x2)
        a = np.concatenate([a, np.concatenate([b, b], axis=0) if x2_rows else b], axis=1)
    return a.reshape(n_inst, rows, -1)


def reference_impls():
    """The float64 references behind the signatures of the ops, results rounded once to the op's output type (temporal attention: the
    evaluation with the two documented roundings): what every check must pass, and the base of the wrong variants."""
    def gn_scale_shift(x1, x2, x2_rows, c_real, n_inst, rows, groups, eps, gamma, beta, **kw):
        s, h, _ = gn_stats_ref(gn_logical(x1, x2, x2_rows, n_inst, rows), c_real, groups, eps, gamma, beta, **kw)
        return t32(s), t32(h)

    def gn_apply(x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode, **kw):
        x = gn_logical(x1, x2, x2_rows, n_inst, rows)
        y = t16(gn_apply_ref(x, scale, shift, silu_on, **kw).reshape(n_inst * rows, -1))
        x32 = x.reshape(n_inst * rows, -1).astype(np.float32)
        raw = None if raw_mode == 0 else torch.from_numpy(x32.astype(np.float16) if raw_mode == 1 else hilo_ref(x32))
        return y, raw

    def fin(part, chunk_rows, c, n_inst, rows, groups, eps, gamma, beta):
        s, h, _ = finalize_ref(part, rows // chunk_rows, c, n_inst, groups, eps, gamma, beta)
        return t32(s), t32(h)

    def fin2(p1, c1, g1, n1, p2, c2, g2, n2, chunk_rows, n_inst, rows, groups, eps, gamma, beta):
        s, h, _ = finalize2_ref(p1, p2, (rows // chunk_rows, c1, g1, n1, c2, g2, n2, groups, n_inst), eps, gamma, beta)
        return t32(s), t32(h)

    def tattn(qkv, nb, t_len, hw, c, heads, scale, cos, sin, rot, bias, **kw):
        if t_len == 1 and not kw:
            return qkv[:, 2 * c:].clone()
        return t16(tattn_ref(qkv, bias, cos, sin, scale, (c, heads, rot, t_len, hw, nb), rounded=True, **kw)[0])

    def sft(dec, sc, sh, w, out_f32):
        d = f64(dec)
        v = d + w * (d * f64(sc) + f64(sh))
        return t32(v) if out_f32 else t16(v)

    return {
        "gn_scale_shift": gn_scale_shift, "gn_apply": gn_apply, "gn_finalize_partials": fin, "gn_finalize_partials2": fin2,
        "layernorm": lambda x, gamma, beta, eps, **kw: t16(layernorm_ref(x, gamma, beta, eps, **kw)),
        "temporal_attention": tattn,
        "linear_small": lambda x, w, b, pre, post: t32(linear_small_ref(x, w, b, pre, post)),
        "timestep_embedding": lambda t, dim, flip, shift, **kw: t32(timestep_embedding_ref(t, dim, flip, shift, **kw)),
        "pack_nhwc": lambda s1, s2, c_pad, scale, **kw: torch.from_numpy(
            pack_nhwc_ref(s1.numpy(), None if s2 is None else s2.numpy(), c_pad, scale, **kw)),
        "unpack_ncthw": lambda src, c, b, t, hw, df, lo, hi: torch.from_numpy(unpack_ncthw_ref(src.numpy(), c, b, t, hw, df, lo, hi)),
        "cast_f32_f16": lambda x: torch.from_numpy(x.numpy().astype(np.float16)),
        "cast_f32_hilo": lambda x: torch.from_numpy(hilo_ref(x.numpy())),
        "sft_fuse": sft,
        "axpby_f16": lambda x, z, a, b: t16(a * f64(x) + b * f64(z)),
    }
