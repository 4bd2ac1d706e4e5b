"""GroupNorm, LayerNorm (csrc/norm.hip), temporal attention (csrc/temporal_attn.hip) and the layout, cast and embedding kernels of
csrc/elementwise.hip, each against its float64 reference at the smallest shapes that reach each of its branches: the cases, references
and pass marks of tests/net_kernels_ref.py (tests/test_net_kernels_cpu.py shows without a GPU that the references are torch's ops, that
every bar can be met and that every check rejects a wrong kernel).

Every kernel is called through the C ABI with its destination INSIDE a larger buffer filled with a sentinel (Guarded of
tests/test_small_kernels_gpu.py): one element of slack behind, and in front one element, or eight fp16 / four fp32 elements where the
kernel moves 16-byte vectors.  The sentinels must keep their bits.  A refused call must return its documented code and leave the
sentinel-filled outputs untouched."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import net_kernels_ref as R  # noqa: E402
from test_small_kernels_gpu import SENTINEL, Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = R.all_cases()
F32, H16 = torch.float32, torch.float16
EINVAL, EALIGN, ESHAPE = -1, -2, -3


def make_impls(dev):
    from uav import _lib, ops
    lib = _lib.load()
    p = ops._p

    def call(name, *args):
        _lib.check(getattr(lib, name)(*args, ops._stream()), name)

    def d(t):
        """To the device; the caller keeps the result in a name for as long as a kernel reads it."""
        return None if t is None else t.to(dev)

    def g16(shape):
        return Guarded(dev, shape, dtype=H16, pre=8)

    def g32(shape, pre=1):
        return Guarded(dev, shape, dtype=F32, pre=pre)

    def gn_scale_shift(x1, x2, x2_rows, c_real, n_inst, rows, groups, eps, gamma, beta):
        c1, c2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
        scale, shift = g32((n_inst, c1 + c2)), g32((n_inst, c1 + c2))
        nb = lib.uav_groupnorm_workspace_bytes(n_inst, c1 + c2)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        x1, x2, gamma, beta = d(x1), d(x2), d(gamma), d(beta)
        call("uav_groupnorm_scale_shift", p(x1), p(x2), int(x1.dtype == F32), c1, c2, x2_rows, c_real, n_inst, rows, groups, eps,
             p(gamma), p(beta), p(scale.dst), p(shift.dst), p(ws), nb)
        return scale.result(), shift.result()

    def gn_apply(x1, x2, x2_rows, n_inst, rows, scale, shift, silu_on, raw_mode):
        c1, c2 = x1.shape[1], 0 if x2 is None else x2.shape[1]
        c = c1 + c2
        y = g16((n_inst * rows, c))
        raw = None if raw_mode == 0 else g16((n_inst * rows, c * raw_mode))
        x1, x2, scale, shift = d(x1), d(x2), d(scale), d(shift)
        call("uav_groupnorm_apply", p(x1), p(x2), int(x1.dtype == F32), c1, c2, x2_rows, n_inst, rows, p(scale), p(shift),
             int(silu_on), p(y.dst), None if raw is None else p(raw.dst), int(raw_mode == 2))
        return y.result(), None if raw is None else raw.result()

    def gn_finalize_partials(part, chunk_rows, c, n_inst, rows, groups, eps, gamma, beta):
        scale, shift = g32((n_inst, c)), g32((n_inst, c))
        part, gamma, beta = d(part), d(gamma), d(beta)
        call("uav_groupnorm_finalize_partials", p(part), part.shape[2], chunk_rows, c, n_inst, rows, groups, eps, p(gamma), p(beta),
             p(scale.dst), p(shift.dst))
        return scale.result(), shift.result()

    def gn_finalize_partials2(p1, c1, g1, n1, p2, c2, g2, n2, chunk_rows, n_inst, rows, groups, eps, gamma, beta):
        scale, shift = g32((n_inst, c1 + c2)), g32((n_inst, c1 + c2))
        p1, p2, gamma, beta = d(p1), d(p2), d(gamma), d(beta)
        call("uav_groupnorm_finalize_partials2", p(p1), p1.shape[2], c1, g1, n1, p(p2), p2.shape[2], c2, g2, n2, chunk_rows, n_inst,
             rows, groups, eps, p(gamma), p(beta), p(scale.dst), p(shift.dst))
        return scale.result(), shift.result()

    def layernorm(x, gamma, beta, eps):
        y = g16(x.shape)
        x, gamma, beta = d(x), d(gamma), d(beta)
        call("uav_layernorm_f32in" if x.dtype == F32 else "uav_layernorm_f16", p(x), p(y.dst), p(gamma), p(beta), x.shape[0],
             x.shape[1], eps)
        return y.result()

    def temporal_attention(qkv, nb, t_len, hw, c, heads, scale, cos, sin, rot, bias):
        out = g16((nb * t_len * hw, c))
        qkv, bias = d(qkv), d(bias)
        cos, sin = (d(cos), d(sin)) if rot else (None, None)
        call("uav_temporal_attention_f16", p(qkv), p(out.dst), nb, t_len, hw, c, heads, scale, p(cos), p(sin), rot, p(bias))
        return out.result()

    def linear_small(x, w, b, pre, post):
        y = g32((x.shape[0], w.shape[0]))
        x, w, b = d(x), d(w), d(b)
        call("uav_linear_small", p(x), p(w), p(b), p(y.dst), x.shape[0], x.shape[1], w.shape[0], int(pre), int(post))
        return y.result()

    def timestep_embedding(t, dim, flip, shift):
        out = g32((t.numel(), dim))
        t = d(t)
        call("uav_timestep_embedding", p(t), t.numel(), dim, flip, shift, p(out.dst))
        return out.result()

    def pack_nhwc(s1, s2, c_pad, scale):
        b, c1, t, hw = s1.shape
        dst = g16((b * t * hw, c_pad))
        s1, s2 = d(s1), d(s2)
        call("uav_pack_nhwc", p(s1), c1, p(s2), 0 if s2 is None else s2.shape[1], int(s1.dtype == F32), p(dst.dst), c_pad, b, t, hw,
             scale)
        return dst.result()

    def unpack_ncthw(src, c, b, t, hw, dst_f32, lo, hi):
        dst = Guarded(dev, (b, c, t, hw), dtype=F32 if dst_f32 else H16)
        src = d(src)
        call("uav_unpack_ncthw", p(src), src.shape[1], int(src.dtype == F32), p(dst.dst), int(dst_f32), c, b, t, hw, lo, hi)
        return dst.result()

    def cast_f32_f16(x):
        y = g16(x.shape)
        x = d(x)
        call("uav_cast_f32_f16", p(x), p(y.dst), x.numel())
        return y.result()

    def cast_f32_hilo(x):
        y = g16((x.shape[0], 2 * x.shape[1]))
        x = d(x)
        call("uav_cast_f32_hilo", p(x), p(y.dst), x.shape[0], x.shape[1])
        return y.result()

    def sft_fuse(dec, sc, sh, w, out_f32):
        out = Guarded(dev, dec.shape, dtype=F32 if out_f32 else H16)
        dec, sc, sh = d(dec), d(sc), d(sh)
        call("uav_sft_fuse", p(dec), p(sc), p(sh), p(out.dst), dec.numel(), w, int(dec.dtype == F32), int(out_f32))
        return out.result()

    def axpby_f16(x, z, a, b):
        y = Guarded(dev, x.shape, dtype=H16)
        x, z = d(x), d(z)
        call("uav_axpby_f16", p(x), p(z), p(y.dst), x.numel(), a, b)
        return y.result()

    return {
        "gn_scale_shift": gn_scale_shift, "gn_apply": gn_apply, "gn_finalize_partials": gn_finalize_partials,
        "gn_finalize_partials2": gn_finalize_partials2, "layernorm": layernorm, "temporal_attention": temporal_attention,
        "linear_small": linear_small, "timestep_embedding": timestep_embedding, "pack_nhwc": pack_nhwc, "unpack_ncthw": unpack_ncthw,
        "cast_f32_f16": cast_f32_f16, "cast_f32_hilo": cast_f32_hilo, "sft_fuse": sft_fuse, "axpby_f16": axpby_f16,
    }


@pytest.fixture(scope="module")
def impls(dev):
    return make_impls(dev)


@pytest.fixture(scope="module")
def record():
    """Collects the Result of every comparison; with UAV_PARITY_RECORD=<file> the table kept as
    profiles/net_kernels_edge_parity.txt is written there once the module has run."""
    results = []
    yield results
    out = os.environ.get("UAV_PARITY_RECORD")
    if out:
        with open(out, "w") as fh:
            fh.write(R.format_record(results))


@pytest.mark.parametrize("key,check,args", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_kernel_vs_float64(impls, record, key, check, args):
    res = check(impls[key], *args)
    record.extend(res.parts or (res,))
    print(f"{res.kernel} {res.case}: error {res.err:.3e}, bar {res.bar:.3e}")
    assert res.err <= res.bar


def test_wrappers_agree_with_the_c_abi(impls, dev):
    """ops.groupnorm, ops.layernorm, ops.temporal_attention and ops.cast_hilo return the bits of the direct calls above (same
    kernels, torch-allocated outputs)."""
    from uav import ops
    shape = (320, 0, 320, 32, 3, 77, False, "randn")
    x1, _, _, gamma, beta = R.gn_input(shape, True)
    x1, gamma, beta = (torch.from_numpy(a) for a in (x1, gamma, beta))
    eps = R.eps32(R.GN_EPS)
    sc, sh = impls["gn_scale_shift"](x1, None, 0, 320, 3, 77, 32, eps, gamma, beta)
    y, raw = impls["gn_apply"](x1, None, 0, 3, 77, sc, sh, True, 2)
    oy, oraw = ops.groupnorm(x1.to(dev), gamma.to(dev), beta.to(dev), n_inst=3, rows_per_inst=77, groups=32, eps=eps, silu=True,
                             want_raw="hilo")
    assert torch.equal(oy.cpu(), y) and torch.equal(oraw.cpu(), raw)
    for f32 in (False, True):
        x, gamma, beta = (torch.from_numpy(a) for a in R.ln_input((5, 520, "randn"), f32))
        got = ops.layernorm(x.to(dev), gamma.to(dev), beta.to(dev), R.eps32(R.LN_EPS)).cpu()
        assert torch.equal(got, impls["layernorm"](x, gamma, beta, R.eps32(R.LN_EPS)))
    case = (128, 2, 32, 8, 33, 2)
    c, heads, rot, t_len, hw, nb = case
    qkv, bias, cos, sin, scale = (torch.from_numpy(a) if not isinstance(a, float) else a for a in R.tattn_input(case))
    got = ops.temporal_attention(qkv.to(dev), n_batch=nb, t_len=t_len, hw=hw, c=c, heads=heads, scale=scale, rope_cos=cos.to(dev),
                                 rope_sin=sin.to(dev), rot_dim=rot, bias=bias.to(dev)).cpu()
    assert torch.equal(got, impls["temporal_attention"](qkv, nb, t_len, hw, c, heads, scale, cos, sin, rot, bias))
    x = torch.from_numpy(R.wide_values(R.rng(40, 33, 320), (33, 320)))
    assert torch.equal(ops.cast_hilo(x.to(dev)).cpu(), impls["cast_f32_hilo"](x))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refusals(dev):
    """[(id, entry point, arguments without the stream, expected code, the Guarded outputs)] — built on the device, small buffers."""
    from uav import ops
    p = ops._p
    keep = []                                                   # inputs stay alive until the calls are made

    def z(n, dtype=F32):
        t = torch.zeros(n, dtype=dtype, device=dev)
        keep.append(t)
        return t

    out = []

    def add(name, fn, args, code, outs):
        out.append((name, fn, args, code, outs))
    x, x2, ga, be = z(64 * 16, H16), z(64 * 16, H16), z(2048), z(2048)
    ws = z(1 << 16, torch.uint8)

    def gn(name, code, *, x1=x, xx2=None, c1=16, c2=0, x2_rows=0, c_real=None, n_inst=2, rows=4, groups=2, scale=True, shift=True,
           wsp=ws, ws_bytes=1 << 16):
        s, h = Guarded(dev, (4096,)), Guarded(dev, (4096,))
        add("scale_shift " + name, "uav_groupnorm_scale_shift",
            (None if x1 is None else p(x1), None if xx2 is None else p(xx2), 0, c1, c2, x2_rows, c1 + c2 if c_real is None else c_real,
             n_inst, rows, groups, 1e-6, p(ga), p(be), p(s.dst) if scale else None, p(h.dst) if shift else None,
             None if wsp is None else p(wsp), ws_bytes), code, [s, h])
    gn("x1 null", EINVAL, x1=None)
    gn("scale null", EINVAL, scale=False)
    gn("shift null", EINVAL, shift=False)
    gn("workspace null", EINVAL, wsp=None)
    gn("workspace too small", EINVAL, ws_bytes=2 * 2 * 3 * 4 - 1)
    gn("c1 % 8", ESHAPE, c1=12)
    gn("c2 % 8", ESHAPE, c1=8, c2=4, xx2=x2)
    gn("c > 2048", ESHAPE, c1=2056)
    gn("c2 without x2", ESHAPE, c1=8, c2=8)
    gn("c_real % groups", ESHAPE, c_real=15)
    gn("c_real > c", ESHAPE, c_real=24)
    gn("n_inst > 65535", ESHAPE, n_inst=65536, rows=1)
    gn("x2_rows not half", ESHAPE, c1=8, c2=8, xx2=x2, x2_rows=3)
    gn("x2_rows without c2", ESHAPE, x2_rows=4)

    sc, sh = z(4096), z(4096)

    def ap(name, code, *, x1=x, xx2=None, c1=16, c2=0, x2_rows=0, n_inst=2, rows=4, scale=sc, shift=sh, y=True):
        yy, raw = Guarded(dev, (64 * 16,), dtype=H16, pre=8), Guarded(dev, (64 * 16,), dtype=H16, pre=8)
        add("apply " + name, "uav_groupnorm_apply",
            (None if x1 is None else p(x1), None if xx2 is None else p(xx2), 0, c1, c2, x2_rows, n_inst, rows,
             None if scale is None else p(scale), None if shift is None else p(shift), 1, p(yy.dst) if y else None, p(raw.dst), 1),
            code, [yy, raw])
    ap("x1 null", EINVAL, x1=None)
    ap("scale null", EINVAL, scale=None)
    ap("y null", EINVAL, y=False)
    ap("c1 % 8", ESHAPE, c1=12)
    ap("c > 2048", ESHAPE, c1=2056)
    ap("c2 without x2", ESHAPE, c1=8, c2=8)
    ap("n_inst > 65535", ESHAPE, n_inst=65536, rows=1)
    ap("x2_rows not half", ESHAPE, c1=8, c2=8, xx2=x2, x2_rows=3)

    part = z(2 * 4 * 6)

    def fin(name, code, *, pp=part, chunks_total=6, chunk_rows=2, c=8, n_inst=2, rows=6, groups=4):
        s, h = Guarded(dev, (64,)), Guarded(dev, (64,))
        add("finalize_partials " + name, "uav_groupnorm_finalize_partials",
            (None if pp is None else p(pp), chunks_total, chunk_rows, c, n_inst, rows, groups, 1e-6, p(ga), p(be), p(s.dst), p(h.dst)),
            code, [s, h])
    fin("partials null", EINVAL, pp=None)
    fin("c % groups", ESHAPE, groups=3)
    fin("rows % chunk_rows", ESHAPE, rows=7)
    fin("chunks_total", ESHAPE, chunks_total=5)
    fin("n_inst > 65535", ESHAPE, n_inst=65536)

    def fin2(name, code, *, p1=part, c1=8, g1=4, n1=2, p2=part, c2=8, g2=4, n2=1, ct1=6, ct2=3, chunk_rows=2, n_inst=2, rows=6, groups=4):
        s, h = Guarded(dev, (64,)), Guarded(dev, (64,))
        add("finalize_partials2 " + name, "uav_groupnorm_finalize_partials2",
            (None if p1 is None else p(p1), ct1, c1, g1, n1, None if p2 is None else p(p2), ct2, c2, g2, n2, chunk_rows, n_inst, rows,
             groups, 1e-6, p(ga), p(be), p(s.dst), p(h.dst)), code, [s, h])
    fin2("partials2 null", EINVAL, p2=None)
    fin2("group straddles the seam", ESHAPE, groups=1, c1=8, c2=16, g2=8)          # cpg 24, c1 % cpg != 0
    fin2("producer group wider", ESHAPE, groups=8, g1=2)                            # cpg 2 % (c1 / groups1 = 4) != 0
    fin2("n_inst % n_inst2", ESHAPE, n_inst=3, n1=3, ct1=9, n2=2, ct2=6)
    fin2("chunks_total2", ESHAPE, ct2=4)

    def ln(name, code, fn="uav_layernorm_f16", *, xx=x, gamma=ga, beta=be, rows=4, c=16, y=True):
        yy = Guarded(dev, (64 * 16,), dtype=H16, pre=8)
        add(f"{fn[4:]} {name}", fn, (None if xx is None else p(xx), p(yy.dst) if y else None, None if gamma is None else p(gamma),
                                     None if beta is None else p(beta), rows, c, 1e-5), code, [yy])
    for fn in ("uav_layernorm_f16", "uav_layernorm_f32in"):
        ln("x null", EINVAL, fn, xx=None)
        ln("gamma null", EINVAL, fn, gamma=None)
        ln("beta null", EINVAL, fn, beta=None)
        ln("c % 8", ESHAPE, fn, c=12)
        ln("c > 2048", ESHAPE, fn, c=2056)
        ln("rows 0", ESHAPE, fn, rows=0)

    qkv, bias, tab = z(3 * 1024 * 9, H16), z(4096), z(4096)

    def ta(name, code, *, q=qkv, t_len=2, c=64, heads=2, rot=8, cos=tab, sin=tab, b=bias, o=True):
        oo = Guarded(dev, (9 * 1024,), dtype=H16, pre=8)
        add("temporal_attention " + name, "uav_temporal_attention_f16",
            (None if q is None else p(q), p(oo.dst) if o else None, 1, t_len, 1, c, heads, 0.125, None if cos is None else p(cos),
             None if sin is None else p(sin), rot, None if b is None else p(b)), code, [oo])
    ta("qkv null", EINVAL, q=None)
    ta("out null", EINVAL, o=False)
    ta("bias null", EINVAL, b=None)
    ta("T > 8", ESHAPE, t_len=9)
    ta("c % heads", ESHAPE, heads=3)
    ta("d = 24 not a power of two", ESHAPE, c=48)
    ta("d = 1024 does not divide 512", ESHAPE, c=1024, heads=1)
    ta("d = 4", ESHAPE, c=8)
    ta("rot_dim > d", ESHAPE, rot=40)
    ta("rot_dim % 8", ESHAPE, rot=4)
    ta("rot_dim > 0 without cos", EINVAL, cos=None)
    ta("rot_dim > 0 without sin", EINVAL, sin=None)

    xs, w16 = z(17 * 16), z(16 * 16, H16)

    def lin(name, code, *, xx=xs, w=w16, m=2, k=16, n=4, y=True):
        yy = Guarded(dev, (17 * 16,))
        add("linear_small " + name, "uav_linear_small", (None if xx is None else p(xx), None if w is None else p(w), p(be),
                                                         p(yy.dst) if y else None, m, k, n, 0, 0), code, [yy])
    lin("x null", EINVAL, xx=None)
    lin("w null", EINVAL, w=None)
    lin("y null", EINVAL, y=False)
    lin("m > 16", ESHAPE, m=17)
    lin("k % 8", ESHAPE, k=12)
    lin("n 0", ESHAPE, n=0)

    def temb(name, code, *, t=xs, dim=8, m=2):
        oo = Guarded(dev, (64,))
        add("timestep_embedding " + name, "uav_timestep_embedding", (None if t is None else p(t), m, dim, 1, 0.0, p(oo.dst)), code, [oo])
    temb("t null", EINVAL, t=None)
    temb("odd dim", ESHAPE, dim=7)
    temb("m 0", ESHAPE, m=0)

    def pack(name, code, *, s1=x, s2=x2, c1=4, c2=3, c_pad=8):
        dd = Guarded(dev, (6 * 16,), dtype=H16, pre=8)
        add("pack_nhwc " + name, "uav_pack_nhwc", (None if s1 is None else p(s1), c1, None if s2 is None else p(s2), c2, 0, p(dd.dst),
                                                   c_pad, 1, 2, 3, 1.0), code, [dd])
    pack("src1 null", EINVAL, s1=None)
    pack("c_pad < c1 + c2", ESHAPE, c1=8, c2=8)
    pack("c_pad % 8", ESHAPE, c_pad=12)
    pack("c2 without src2", ESHAPE, s2=None)

    def unpack(name, code, *, src=x, stride=8, c=3):
        dd = Guarded(dev, (6 * 8,), dtype=H16)
        add("unpack_ncthw " + name, "uav_unpack_ncthw", (None if src is None else p(src), stride, 0, p(dd.dst), 0, c, 1, 2, 3, -1.0, 1.0),
            code, [dd])
    unpack("src null", EINVAL, src=None)
    unpack("src_stride < c", ESHAPE, stride=2)

    xf = z(64)
    for name, off_x, off_y, n, code in (("x null", None, 0, 8, EINVAL), ("n 0", 0, 0, 0, EINVAL), ("x misaligned", 1, 0, 8, EALIGN),
                                        ("y misaligned", 0, 1, 8, EALIGN)):
        yy = Guarded(dev, (32,), dtype=H16, pre=8)
        add("cast_f32_f16 " + name, "uav_cast_f32_f16", (None if off_x is None else p(xf[off_x:]), p(yy.dst[off_y:]), n), code, [yy])
    for name, off_x, off_y, c, code in (("x null", None, 0, 8, EINVAL), ("c % 8", 0, 0, 12, ESHAPE), ("x misaligned", 1, 0, 8, EALIGN),
                                        ("y misaligned", 0, 1, 8, EALIGN)):
        yy = Guarded(dev, (64,), dtype=H16, pre=8)
        add("cast_f32_hilo " + name, "uav_cast_f32_hilo", (None if off_x is None else p(xf[off_x:]), p(yy.dst[off_y:]), 2, c), code, [yy])
    for name, dec, n in (("dec null", None, 8), ("n 0", xf, 0)):
        oo = Guarded(dev, (8,))
        add("sft_fuse " + name, "uav_sft_fuse", (None if dec is None else p(dec), p(xf), p(xf), p(oo.dst), n, 0.5, 1, 1), EINVAL, [oo])
    for name, xx, n in (("x null", None, 8), ("n 0", x, 0)):
        oo = Guarded(dev, (8,), dtype=H16)
        add("axpby_f16 " + name, "uav_axpby_f16", (None if xx is None else p(xx), p(x2), p(oo.dst), n, 0.5, 0.5), EINVAL, [oo])
    return out, keep


def test_refusals_return_their_code_and_write_nothing(dev):
    from uav import _lib, ops
    lib = _lib.load()
    cases, keep = _refusals(dev)
    wrong = []
    for name, fn, args, code, outs in cases:
        rc = getattr(lib, fn)(*args, ops._stream())
        if rc != code:
            wrong.append(f"{name}: returned {rc}, expected {code}")
            if rc == 0:
                continue                                        # it ran: what it wrote is its result, not a stray store
        for o in outs:
            got = o.result()                                    # asserts the slack
            assert bool((got == SENTINEL).all()), f"{name}: a refused call wrote into its output"
    torch.cuda.synchronize()
    assert not wrong, "; ".join(wrong)
    assert len(cases) >= 80
