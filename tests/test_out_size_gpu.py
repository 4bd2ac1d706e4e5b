"""`--out-size` / `--out-scale` on the device: `uav_resize_aa_f32` (csrc/resize_aa.hip) against the float64 reference
tests/resize_aa_ref.py on the smallest shapes that reach each of its ways to go wrong, with the bytes around `dst` and the workspace
untouched; its determinism, its scalar mode and its refusals; the `ops` wrapper; and the program's files against the reference
encoder's planes of `upscale_clip(..., out_size=)`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import resize_aa_ref  # noqa: E402
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402
from test_stream_gpu import _Guarded  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, EALIGN, ESHAPE = -1, -2, -3

SHAPES = resize_aa_ref.SHAPES      # (hi, wi, ho, wo), planes — and what each shape reaches: listed there
TOL = 1e-5      # ~6x the 1.7e-6 of an fp32 emulation with exact positions on these shapes; a wrong tap or half a sample is >= 1e-2
                # (measured on an MI355X: 1.3e-6 at (32,32)->(50,44), see profiles/out_size_kernels.txt)


_case = resize_aa_ref.case


def _lib():
    from uav import _lib as L
    return L.load()


def _resize(dev, x, ho, wo, shift=0, src_shift=0):
    """`x` (planes, hi, wi) on the host through the C entry point, `dst` and the workspace in guarded buffers whose bases are `shift`
    bytes past an aligned address (and the source `src_shift` floats past one); the result as numpy, after the guards are checked."""
    lib = _lib()
    planes, hi, wi = x.shape
    hold = torch.empty(x.numel() + src_shift, dtype=torch.float32, device=dev)
    src = hold[src_shift:]
    src.copy_(x.reshape(-1))
    nb = lib.uav_resize_aa_workspace_bytes(planes, hi, wi, ho, wo)
    assert nb >= planes * hi * wo * 4
    dst, ws = _Guarded(planes * ho * wo * 4, dev, shift), _Guarded(nb, dev, shift)
    assert lib.uav_resize_aa_f32(src.data_ptr(), dst.ptr, planes, hi, wi, ho, wo, ws.ptr, nb, None) == 0
    torch.cuda.synchronize()
    assert dst.intact() and ws.intact(), "a guard around dst or the workspace was written"
    return dst.body().view(np.float32).reshape(planes, ho, wo).copy()


@pytest.mark.parametrize("shape,planes", SHAPES)
def test_kernel_equals_the_reference(dev, shape, planes):
    x, ref = _case(shape, planes)
    got = _resize(dev, x, *shape[2:])
    err = float(np.abs(got - ref).max())
    flat = float(np.abs(got[-1] - np.float32(0.7315)).max())
    print(f"{shape} x {planes} planes: max abs error {err:.2e}, constant plane {flat:.1e}")
    assert np.isfinite(got).all() and err < TOL
    assert flat <= 1e-6, "a constant plane must come back constant"
    if shape[:2] == shape[2:]:
        assert np.array_equal(got, x.numpy()), "equal sizes must copy"


@pytest.mark.parametrize("shape,planes", [SHAPES[0], SHAPES[4], SHAPES[5], SHAPES[6], SHAPES[10], SHAPES[11], SHAPES[12], SHAPES[13], SHAPES[14]])
def test_two_runs_and_the_scalar_mode_give_the_same_bits(dev, shape, planes):
    """`dst` and the workspace 4 bytes past a 16-byte boundary, and the source too: scalar accesses, the same values."""
    x, ref = _case(shape, planes)
    first = _resize(dev, x, *shape[2:])
    assert np.array_equal(first, _resize(dev, x, *shape[2:])), "two runs differ"
    assert np.array_equal(first, _resize(dev, x, *shape[2:], shift=4)), "dst / workspace off the 16-byte grid: other values"
    assert np.array_equal(first, _resize(dev, x, *shape[2:], shift=4, src_shift=1)), "all three off the 16-byte grid: other values"
    assert np.array_equal(first, _resize(dev, x, *shape[2:], src_shift=3))


def test_resize_matches_torch_within_torchs_own_error(dev):
    """The filter is the one of F.interpolate(mode='bicubic', antialias=True): 2e-4, the pass mark of the CPU test."""
    import torch.nn.functional as F
    for shape, planes in (SHAPES[0], SHAPES[5], SHAPES[11]):
        x, _ = _case(shape, planes)
        theirs = F.interpolate(x[None], size=shape[2:], mode="bicubic", antialias=True, align_corners=False)[0].numpy()
        assert np.abs(_resize(dev, x, *shape[2:]) - theirs).max() < 2e-4


def test_kernel_refuses_bad_arguments_before_any_launch(dev):
    lib = _lib()
    src = torch.zeros(2 * 16 * 24, device=dev)
    nb = lib.uav_resize_aa_workspace_bytes(2, 16, 24, 9, 14)
    dst, ws = _Guarded(2 * 9 * 14 * 4, dev), _Guarded(nb, dev)

    def call(planes=2, hi=16, wi=24, ho=9, wo=14, s=src.data_ptr(), d=dst.ptr, w=ws.ptr, n=nb):
        return lib.uav_resize_aa_f32(s, d, planes, hi, wi, ho, wo, w, n, None)
    assert call(s=None) == EINVAL and call(d=None) == EINVAL and call(w=None) == EINVAL
    for off in (1, 2, 3):
        assert call(s=src.data_ptr() + off) == EALIGN and call(d=dst.ptr + off) == EALIGN and call(w=ws.ptr + off) == EALIGN
    assert call(planes=0) == ESHAPE and call(planes=-1) == ESHAPE and call(planes=65536) == ESHAPE
    for kw in (dict(hi=0), dict(wi=0), dict(ho=0), dict(wo=0), dict(hi=-4), dict(wo=-1)):
        assert call(**kw) == ESHAPE
        args = {**dict(planes=2, hi=16, wi=24, ho=9, wo=14), **kw}
        assert lib.uav_resize_aa_workspace_bytes(*(args[k] for k in ("planes", "hi", "wi", "ho", "wo"))) == ESHAPE
    assert call(planes=1, hi=130, wi=2, ho=2, wo=2) == ESHAPE and call(planes=1, hi=2, wi=193, ho=2, wo=3) == ESHAPE    # n_in > 64 n_out
    assert lib.uav_resize_aa_workspace_bytes(1, 128, 2, 2, 2) > 0 and lib.uav_resize_aa_workspace_bytes(1, 129, 2, 2, 2) == ESHAPE
    assert call(n=nb - 1) == ESHAPE and call(n=0) == ESHAPE and call(n=-8) == ESHAPE
    torch.cuda.synchronize()
    for g in (dst, ws):
        assert g.intact() and (g.body() == 0xA5).all(), "a refused call wrote"
    assert call() == 0                                                          # ... and the arguments the refusals varied are good
    torch.cuda.synchronize()
    assert dst.intact() and ws.intact() and (dst.body().view(np.float32) == 0).all()


def test_ops_wrapper_folds_leading_dimensions(dev):
    from uav import _lib as L
    from uav import ops
    x, ref = _case((64, 96, 36, 54), 3)
    frames = torch.stack([x, x.flip(0)]).to(dev)                               # (T,3,H,W)
    out = ops.resize_aa_f32(frames, 36, 54)
    assert out.shape == (2, 3, 36, 54) and out.dtype == torch.float32 and out.is_contiguous()
    assert np.abs(out[0].cpu().numpy() - ref).max() < TOL and torch.equal(out[1], out[0].flip(0))
    assert torch.equal(ops.resize_aa_f32(frames[0, 0], 36, 54), out[0, 0])      # (H,W): one plane
    assert torch.equal(ops.resize_aa_f32(frames, 64, 96), frames)
    for bad in (frames.cpu(), frames.double(), frames[..., ::2], frames.permute(0, 1, 3, 2), frames.half()):
        with pytest.raises(L.UavError):
            ops.resize_aa_f32(bad, 36, 54)
    for ho, wo in ((0, 54), (36, 0), (36, 1)):                                  # 96 > 64 * 1
        with pytest.raises(L.UavError):
            ops.resize_aa_f32(frames, ho, wo)


def test_program_resizes_on_the_device(dev, tmp_path):
    """One fresh process on the tiny seeded checkpoints (see `_child`)."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-3000:])


# ---- child ---------------------------------------------------------------------------------------------------------------
def _child(tmp):
    import time
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import cli, ops, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)
    sources = {}
    for name, shape in (("in5", (5, 64, 96, 71)), ("tiled4", (4, 68, 160, 72))):
        rgb = _clip_u8(*shape).permute(0, 2, 3, 1).contiguous().numpy()
        video_io.write_y4m(name + ".y4m", *yuv_ref.encode(rgb, "bt601", True), "30000/1001", True)
        sources[name] = video_io.preprocess_planes(video_io.read_y4m(name + ".y4m"), dev, "auto")
    pipe, _ = cli.load_pipeline(base, device=dev)
    common = ["-s", "2", "--pretrained", base, "--device", "cuda:0"]
    opts = dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2, guidance_scale=6, noise_level=120)
    tile = (["--perform_tile", "--tile_size", "64"], dict(perform_tile=True, tile_size=64))
    # (input, size option, (H, W), further options, their keywords, format)
    jobs = (("in5", ["--out-size", "216x144"], (144, 216), [], {}, "420"),
            ("in5", ["--out-scale", "2.5"], (160, 240), ["--color_fix", "Wavelet"], dict(color_fix="Wavelet"), "420p10"),
            ("tiled4", ["--out-size", "400x170"], (170, 400)) + tile + ("444p10",),
            ("tiled4", ["--out-size", "401:171"], (171, 401)) + tile + ("444",))

    def gen():
        return torch.Generator(device=dev).manual_seed(10)
    full = {}
    for k, (name, size, (h, w), extra, kw, fmt) in enumerate(jobs):
        assert cli.main(["-i", name + ".y4m", "-o", f"o{k}", "--out-format", fmt] + common + size + extra) == 0
        got = open(f"o{k}/video/{name}_n120_g6_s2.y4m", "rb").read()
        source = sources[name]
        t = source.shape[2]
        frames = video_io.upscale_clip(pipe, source, generator=gen(), out_size=(h, w), **opts, **kw)
        key = (name, tuple(sorted(kw)))
        if key not in full:
            full[key] = video_io.upscale_clip(pipe, source, generator=gen(), **opts, **kw)
        assert full[key].shape == (t, 3, 4 * source.shape[-2], 4 * source.shape[-1])
        assert frames.shape == (t, 3, h, w) and frames.dtype == torch.float32
        assert torch.equal(frames, ops.resize_aa_f32(full[key], h, w)), "upscale_clip(out_size=) is not the resize of upscale_clip()"
        tag = yuv_fmt_ref.FORMATS[fmt][2] if fmt != "420" else "C420jpeg"
        head = f"YUV4MPEG2 W{w} H{h} F30000:1001 Ip A1:1 {tag} XCOLORRANGE=FULL\n".encode()
        host = frames.cpu().numpy()
        planes = yuv_ref.encode(yuv_fmt_ref.rgb_u8(host), "bt601", True) if fmt == "420" else yuv_fmt_ref.encode(host, fmt, "bt601", True)
        expect = yuv_fmt_ref.file_bytes(planes, head)
        assert got.startswith(head) and len(got) == len(expect)
        assert got == expect, f"{name} {size} {fmt}: the file is not the reference's planes of upscale_clip(..., out_size=)"
        assert host.std() > 0.05
        print(f"{name} {' '.join(size + extra)} {fmt}: {len(got)} bytes ok at {time.time() - start:.1f} s", flush=True)
    # no option, and the 4x size by name: the bytes of the path without a resize
    assert cli.main(["-i", "in5.y4m", "-o", "plain"] + common) == 0
    assert cli.main(["-i", "in5.y4m", "-o", "named", "--out-size", "384x256"] + common) == 0
    plain = open("plain/video/in5_n120_g6_s2.y4m", "rb").read()
    head = b"YUV4MPEG2 W384 H256 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    host = full[("in5", ())].cpu().numpy()
    assert plain == yuv_fmt_ref.file_bytes(yuv_ref.encode(yuv_fmt_ref.rgb_u8(host), "bt601", True), head)
    assert plain == open("named/video/in5_n120_g6_s2.y4m", "rb").read()
    print(f"child total {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
