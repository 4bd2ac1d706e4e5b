"""Thin output-channel conv kernel (csrc/conv_thin.hip: stride-1 1x1 / 3x3 convs with n <= 16) through ops.conv_gemm, against fp64
F.conv2d on the fp16-rounded inputs and weights.

The bar is relative, not a number fixed in advance: for every case the 128 x 128 tile kernel (the path these launches took before,
UAV_CONV_THIN=0) runs on the same inputs, and the thin kernel's maximum and rms error against fp64 must be at most 2x that path's.
Both accumulate in fp32 over the whole K and only the summation order may differ.  Every figure is printed (recorded in
profiles/conv_thin_parity.txt; as measured there the two kernels agree bit for bit — both walk K in 64-channel chunks with the taps
innermost — so the results cannot tell which kernel ran: the per-launch time does, profiles/conv_thin_launch_ab.txt).

Geometries (the patch of a workgroup is 8 x 32 output pixels): 5x7 = one patch with all four image borders inside it, 8x32 = exactly
one patch, 9x33 = one pixel more than a patch in each direction, 17x33 = several patches with tails; each with 1 and 3 images."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GEOMS = [(5, 7), (8, 32), (9, 33), (17, 33)]
N_IMGS = [1, 3]


@contextlib.contextmanager
def thin(on):
    """The switch is read at every eligible launch, so both paths run in this process."""
    old = os.environ.get("UAV_CONV_THIN")
    os.environ["UAV_CONV_THIN"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["UAV_CONV_THIN"]
        else:
            os.environ["UAV_CONV_THIN"] = old


def make_case(cin, n, ks, n_img, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_img, cin, h, w, generator=g).half()
    wgt = (torch.randn(n, cin, ks, ks, generator=g) * (cin * ks * ks) ** -0.5).half()
    bias = torch.randn(n, generator=g)
    ref = F.conv2d(x.double(), wgt.double(), bias.double(), padding=ks // 2)          # fp64 on the fp16-rounded operands
    rows = x.permute(0, 2, 3, 1).reshape(n_img * h * w, cin).contiguous()
    return rows, wgt, bias, ref.permute(0, 2, 3, 1).reshape(n_img * h * w, n)


def errors(out, ref, n):
    d = out[:, :n].double().cpu() - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("of32", [True, False], ids=["f32", "f16"])
@pytest.mark.parametrize("ks", [3, 1], ids=["3x3", "1x1"])
@pytest.mark.parametrize("n", [3, 4, 16])
@pytest.mark.parametrize("cin", [64, 128, 256])
def test_thin_vs_fp64_no_worse_than_tile128(dev, cin, n, ks, of32):
    from uav import ops
    fails = []
    for gi, (h, w) in enumerate(GEOMS):
        for n_img in N_IMGS:
            rows, wgt, bias, ref = make_case(cin, n, ks, n_img, h, w, seed=1000 * cin + 100 * n + 10 * gi + n_img + ks)
            wt = ops.pack_conv(wgt, bias, device=dev)
            kw = dict(n_img=n_img, t_len=1, hi=h, wi=w, out_f32=of32)
            a1 = rows.to(dev)
            with thin(True):
                y = ops.conv_gemm(a1, wt, **kw)
            with thin(False):
                y0 = ops.conv_gemm(a1, wt, **kw)
            assert y.shape == y0.shape == (n_img * h * w, wt.n) and y.dtype == (torch.float32 if of32 else torch.float16)
            if wt.n > n:                                   # 3 -> 4: the padding column has zero weights and zero bias
                assert float(y[:, n:].abs().max()) == 0.0
            (mx, rms), (mx0, rms0) = errors(y, ref, n), errors(y0, ref, n)
            print(f"conv_thin cin={cin} n={n} k={ks}x{ks} {'f32' if of32 else 'f16'} {n_img}x{h}x{w}: "
                  f"thin max {mx:.3e} rms {rms:.3e} | tile128 max {mx0:.3e} rms {rms0:.3e}")
            if not (mx <= 2.0 * mx0 and rms <= 2.0 * rms0):
                fails.append((n_img, h, w, mx, mx0, rms, rms0))
    assert not fails, fails


def test_residual_launch_keeps_its_path(dev):
    """Not eligible (residual given): the launch must take the 128 x 128 path whatever the switch says, bit for bit."""
    from uav import ops
    rows, wgt, bias, _ = make_case(128, 4, 3, 2, 9, 33, seed=7)
    wt = ops.pack_conv(wgt, bias, device=dev)
    res = torch.randn(rows.shape[0], 4, generator=torch.Generator().manual_seed(8)).half().to(dev)
    kw = dict(n_img=2, t_len=1, hi=9, wi=33, residual=res)
    with thin(True):
        a = ops.conv_gemm(rows.to(dev), wt, **kw)
    with thin(False):
        b = ops.conv_gemm(rows.to(dev), wt, **kw)
    assert torch.equal(a, b)


@pytest.mark.parametrize("of32", [True, False], ids=["f32", "f16"])
def test_rows_beyond_m_and_columns_beyond_n_untouched(dev, of32):
    from uav import ops
    n_img, h, w, n = 3, 9, 33, 4
    rows, wgt, bias, ref = make_case(64, n, 3, n_img, h, w, seed=21)
    wt = ops.pack_conv(wgt, bias, device=dev)
    m = n_img * h * w
    dt = torch.float32 if of32 else torch.float16
    buf = torch.full((m + 5, 12), 77.0, dtype=dt, device=dev)
    with thin(True):
        out = ops.conv_gemm(rows.to(dev), wt, n_img=n_img, t_len=1, hi=h, wi=w, out_f32=of32, out=buf)
    assert out is buf
    assert bool((buf[m:] == 77.0).all()) and bool((buf[:, n:] == 77.0).all())
    mx, _ = errors(buf[:m], ref, n)
    assert mx < (1e-4 if of32 else 1e-2)                   # the written part is the convolution (fp32 sum / fp16 rounding of |v| < 8)
