"""The small fp32 kernels — colour fix (csrc/colorfix.hip), RAFT's non-GEMM kernels (csrc/raft.hip) and the scheduler kernels of
csrc/elementwise.hip — each against its float64 reference at the smallest shapes that reach each of its branches: the cases, references
and pass marks of tests/small_kernels_ref.py (tests/test_small_kernels_cpu.py shows without a GPU that the references are torch's ops,
that every bar can be met and that every check rejects a wrong kernel).

Every kernel is called through the C ABI with its destination INSIDE a larger buffer filled with a sentinel: one element of slack in
front and behind (four fp32 / eight fp16 elements in front where the kernel moves 16-byte vectors, whose pointers it expects aligned
like torch's allocations), and the padding columns of row buffers.  The sentinels must keep their bits.  Only the five-level wavelet
functions go through models_video.color_correction, which allocates its own tensors."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import small_kernels_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = R.all_cases()
SENTINEL = 31337.0
F32 = torch.float32


class Guarded:
    """A destination of `shape` inside a sentinel-filled buffer, `pre` elements in and `post` from the end."""

    def __init__(self, dev, shape, dtype=F32, pre=1, post=1, init=None):
        n = 1
        for s in shape:
            n *= int(s)
        self.buf = torch.full((pre + n + post,), SENTINEL, dtype=dtype, device=dev)
        self.dst = self.buf[pre:pre + n].view(*shape)
        if init is not None:
            self.dst.copy_(init)
        self.pre, self.n = pre, n

    def result(self):
        """The destination on the CPU, after checking the slack bit for bit."""
        bits = torch.int32 if self.buf.dtype == F32 else torch.int16
        want = torch.full((1,), SENTINEL, dtype=self.buf.dtype).view(bits).item()
        b = self.buf.cpu()
        slack = torch.cat([b[:self.pre], b[self.pre + self.n:]]).view(bits)
        assert bool((slack == want).all()), f"sentinel overwritten: {torch.cat([b[:self.pre], b[self.pre + self.n:]]).tolist()}"
        return b[self.pre:self.pre + self.n].view(*self.dst.shape).clone()


def make_impls(dev):
    from models_video import color_correction as CC
    from uav import _lib, ops
    lib = _lib.load()
    p = ops._p

    def call(name, *args):
        _lib.check(getattr(lib, name)(*args, ops._stream()), name)

    def d(t):
        """To the device; the caller keeps the result in a name for as long as a kernel reads it."""
        return None if t is None else t.to(dev)

    def plane_stats(x):
        planes, hw = x.shape
        mean, var = Guarded(dev, (planes,)), Guarded(dev, (planes,))
        nb = lib.uav_plane_stats_workspace_bytes(planes)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        x = d(x)
        call("uav_plane_stats_f32", p(x), planes, hw, p(mean.dst), p(var.dst), p(ws), nb)
        return mean.result(), var.result()

    def adain_apply(x, cm, cv, sm, sv, eps):
        planes, hw = x.shape
        out = Guarded(dev, x.shape, pre=4)
        x, cm, cv, sm, sv = (d(t) for t in (x, cm, cv, sm, sv))
        call("uav_adain_apply_f32", p(x), p(out.dst), planes, hw, p(cm), p(cv), p(sm), p(sv), eps)
        return out.result()

    def atrous_blur(x, r, high):
        planes, h, w = x.shape
        low = Guarded(dev, x.shape)
        hi = None if high is None else Guarded(dev, x.shape, init=high)
        x = d(x)
        call("uav_atrous_blur_f32", p(x), p(low.dst), None if hi is None else p(hi.dst), planes, h, w, r)
        return low.result(), None if hi is None else hi.result()

    def decomposition(image):
        high, low = CC.wavelet_decomposition(d(image))
        return high.cpu(), low.cpu()

    def resize_bicubic(x, ho, wo, sh, sw):
        planes, hi, wi = x.shape
        out = Guarded(dev, (planes, ho, wo))
        x = d(x)
        call("uav_resize_bicubic_f32", p(x), p(out.dst), planes, hi, wi, ho, wo, sh, sw)
        return out.result()

    def instnorm(x, n_img, hw, relu, eps):
        y = Guarded(dev, x.shape)
        x = d(x)
        call("uav_instnorm_f32", p(x), p(y.dst), n_img, hw, x.shape[1], eps, int(relu))
        return y.result()

    def add_relu(a, b, relu):
        o = Guarded(dev, a.shape)
        a, b = d(a), d(b)
        call("uav_add_relu_f32", p(a), p(b), p(o.dst), a.numel(), int(relu))
        return o.result()

    def axpby(x, z, a, b):
        y = Guarded(dev, x.shape)
        x, z = d(x), d(z)
        call("uav_axpby_f32", p(x), p(z), p(y.dst), x.numel(), a, b)
        return y.result()

    def gru_rh(zr, h):
        out = Guarded(dev, h.shape)
        zr, h = d(zr), d(h)
        call("uav_gru_gates_f32", p(zr), p(h), None, p(out.dst), h.shape[0], h.shape[1], 0)
        return out.result()

    def gru_blend(zr, q, h):
        hh = Guarded(dev, h.shape, init=h)                               # in place on h
        zr, q = d(zr), d(q)
        call("uav_gru_gates_f32", p(zr), p(hh.dst), p(q), p(hh.dst), h.shape[0], h.shape[1], 1)
        return hh.result()

    def copy_cols(src, scol, dst, dcol, ncols, act):
        o = Guarded(dev, dst.shape, init=dst)
        src = d(src)
        call("uav_copy_cols_f32", p(src), src.shape[1], scol, p(o.dst), dst.shape[1], dcol, ncols, src.shape[0], act)
        return o.result()

    def avgpool2(src, stride, h, w, p_count):
        o = Guarded(dev, (p_count, (h // 2) * (w // 2)))
        src = d(src)
        call("uav_avgpool2_f32", p(src), stride, h, w, p(o.dst), p_count)
        return o.result()

    def resize_bilinear(x, ho, wo, r0, r1):
        planes, hi, wi = x.shape
        o = Guarded(dev, (planes, ho, wo))
        x = d(x)
        call("uav_resize_bilinear_f32", p(x), p(o.dst), planes, hi, wi, ho, wo, r0, r1)
        return o.result()

    def corr_lookup(levels, strides, hs, ws, coords, out, radius):
        lv, coords = [d(l) for l in levels], d(coords)
        o = Guarded(dev, out.shape, init=out)
        call("uav_corr_lookup_f32", (C.c_void_p * 4)(*[p(l) for l in lv]), (C.c_int64 * 4)(*strides), (C.c_int32 * 4)(*hs),
             (C.c_int32 * 4)(*ws), p(coords), coords.shape[1], p(o.dst), out.shape[1], coords.shape[0], radius)
        return o.result()

    def convex_upsample(flow, mask, n, h, w):
        o = Guarded(dev, (n, 2, 8 * h, 8 * w))
        flow, mask = d(flow), d(mask)
        call("uav_convex_upsample_f32", p(flow), flow.shape[1], p(mask), p(o.dst), n, h, w)
        return o.result()

    def cfg_ddim_v0(eu, ec, x, *, guidance, coef_sample, coef_eps, clip, clip_range):
        half = x.dtype == torch.float16
        g = Guarded(dev, x.shape, dtype=x.dtype, pre=8 if half else 1)
        x0 = Guarded(dev, x.shape, dtype=x.dtype, pre=8 if half else 1)
        eu, ec, x = d(eu), d(ec), d(x)
        call("uav_cfg_ddim_v0" if half else "uav_cfg_ddim_v0_f32", p(eu), None if ec is None else p(ec), p(x), p(g.dst),
             p(x0.dst), x.numel(), guidance, coef_sample, coef_eps, int(clip), clip_range)
        return g.result(), x0.result()

    def ddim_vt(x0, g, x, *, coef_x0, coef_dir, eps_from_model, eps_from_sample, eps_from_x0, clip, clip_range):
        prev = Guarded(dev, x.shape, dtype=x.dtype)
        x0, g, x = d(x0), d(g), d(x)
        call("uav_ddim_vt" if x.dtype == torch.float16 else "uav_ddim_vt_f32", p(x0), p(g), p(x), p(prev.dst), x.numel(),
             coef_x0, coef_dir, eps_from_model, eps_from_sample, eps_from_x0, int(clip), clip_range)
        return prev.result()

    return {
        "plane_stats": plane_stats, "adain_apply": adain_apply, "atrous_blur": atrous_blur,
        "wavelet": (decomposition, lambda c, s: CC.wavelet_reconstruction(d(c), d(s)).cpu()),
        "resize_bicubic": resize_bicubic, "instnorm": instnorm, "add_relu": add_relu, "axpby": axpby, "gru_rh": gru_rh,
        "gru_blend": gru_blend, "copy_cols": copy_cols, "avgpool2": avgpool2, "resize_bilinear": resize_bilinear,
        "corr_lookup": corr_lookup, "convex_upsample": convex_upsample, "cfg_ddim_v0": cfg_ddim_v0, "ddim_vt": ddim_vt,
    }


@pytest.fixture(scope="module")
def impls(dev):
    return make_impls(dev)


@pytest.fixture(scope="module")
def record():
    """Collects the Result of every comparison; with UAV_PARITY_RECORD=<file> the table kept as
    profiles/small_kernels_edge_parity.txt is written there once the module has run."""
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
    """The uav.ops wrappers the models call return the bits of the direct calls above (same kernels, torch-allocated outputs)."""
    from uav import ops
    x = torch.from_numpy(R.plane_stats_input(("uniform", 2, 7680)))
    m, v = ops.plane_stats_f32(x.reshape(2, 96, 80).to(dev))
    rm, rv = impls["plane_stats"](x)
    assert torch.equal(m.cpu(), rm) and torch.equal(v.cpu(), rv)
    a, b = torch.from_numpy(R.randn32(R.rng(1), 257)), torch.from_numpy(R.randn32(R.rng(2), 257))
    assert torch.equal(ops.add_relu_f32(a.to(dev), b.to(dev), relu=True).cpu(), impls["add_relu"](a, b, True))
    assert torch.equal(ops.axpby_f32(a.to(dev), b.to(dev), 0.7, -1.3).cpu(), impls["axpby"](a, b, 0.7, -1.3))
    dst = torch.full((257, 5), R.DST_FILL)
    got = ops.copy_cols_f32(a.reshape(257, 1).to(dev), 0, dst.to(dev), 3, 1, act=4).cpu()
    assert torch.equal(got, impls["copy_cols"](a.reshape(257, 1), 0, dst, 3, 1, 4))
