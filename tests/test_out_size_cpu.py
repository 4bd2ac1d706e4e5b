"""`--out-size` / `--out-scale` without a GPU: the float64 reference of the antialiased cubic resize (tests/resize_aa_ref.py,
written from include/uav_hip.h) against torch's CPU implementation of the same filter, the arithmetic of `video_io.output_size`,
the parser's refusals, and the program end to end on the CPU stand-ins (in a child interpreter, as
tests/test_out_format_cpu.py does)."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import resize_aa_ref  # noqa: E402
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402

# (hi, wi, ho, wo): the shapes of the kernel's GPU test
SHAPES = sorted({shape for shape, _ in resize_aa_ref.SHAPES})


def _input(planes, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((planes, h, w), generator=g) * 0.8).clamp(-1.5, 1.5)


@pytest.mark.parametrize("hi,wi,ho,wo", SHAPES)
def test_reference_is_torchs_antialiased_bicubic(hi, wi, ho, wo):
    """Pass mark 2e-4: 3x the 6.5e-5 measured at 256 -> (255, 257), all of it torch's fp32 positions (the rest: <= 2.6e-5).
    torch forms a sample's centre in the tensor's type, so its fp32 error grows with the index: measured 1.0e-3 at 4096 -> 4095 and
    2e-4 to 3e-4 at 4096 -> 2160, the error the kernel is required NOT to have.  The shapes from 4096 columns up are therefore held against
    torch's float64 path, and so is every other shape: the same code with exact enough positions, measured 9e-13 at the worst
    (4096 -> 4095), held to 1e-9 — sums of up to 52 x 52 float64 products of values below 1.5 agree to ~1e-13 whatever their order, and
    a position or weight that differed between the two would show at 1e-6 or more."""
    x = _input(2, hi, wi, seed=hi + wi + ho + wo)
    ref = resize_aa_ref.resize(x.numpy(), ho, wo)
    assert ref.shape == (2, ho, wo)
    kw = dict(size=(ho, wo), mode="bicubic", antialias=True, align_corners=False)
    err64 = float(np.abs(F.interpolate(x[None].double(), **kw)[0].numpy() - ref).max())
    err32 = float(np.abs(F.interpolate(x[None], **kw)[0].numpy() - ref).max())
    print(f"({hi},{wi}) -> ({ho},{wo}): torch vs float64 reference: fp32 {err32:.2e}, float64 {err64:.2e}")
    assert err64 < 1e-9
    if wi < 4096:
        assert err32 < 2e-4
    if (hi, wi) == (ho, wo):
        assert np.array_equal(ref, x.numpy().astype(np.float64))


def test_reference_weights():
    for n_in, n_out, most in ((96, 54, 8), (64, 36, 8), (64, 27, 10), (96, 41, 10), (32, 50, 4), (256, 257, 4), (64, 5, 52), (16, 1, 16),
                              (256, 255, 4), (4096, 4095, 4), (4096, 2160, 8)):
        m, counts = resize_aa_ref.weight_matrix(n_in, n_out)
        assert np.abs(m.sum(axis=1) - 1).max() < 1e-14
        assert max(counts) == most <= min(n_in, -(-4 * n_in // n_out) if n_in >= n_out else 4), (n_in, n_out, max(counts))   # the kernel's table size
        assert min(counts) >= 2 or n_in == 1
    m, counts = resize_aa_ref.weight_matrix(48, 48)                            # equal sizes: (0, 1, 0, 0), a copy
    assert np.array_equal(m, np.eye(48)) and max(counts) == 4


def test_output_size_arithmetic():
    from uav.video_io import output_size
    assert output_size(256, 384, fmt="420") == (256, 384)
    # the ends of the range, as (W, H)
    assert output_size(256, 384, out_size=(96, 64), fmt="420") == (64, 96)
    assert output_size(256, 384, out_size=(384, 256), fmt="420") == (256, 384)
    assert output_size(256, 384, out_size=(216, 144), fmt="420p10") == (144, 216)
    for bad in ((94, 64), (96, 62), (386, 256), (384, 258), (0, 0), (216, 300), (400, 144)):
        with pytest.raises(ValueError, match="96x64 to 384x256"):
            output_size(256, 384, out_size=bad, fmt="444")
    # odd sides: 4:2:0 refuses them and says what it takes, 4:4:4 writes them
    for fmt in ("420", "420p10"):
        for odd in ((217, 144), (216, 145), (97, 65)):
            with pytest.raises(ValueError, match="even"):
                output_size(256, 384, out_size=odd, fmt=fmt)
    for fmt in ("444", "444p10"):
        assert output_size(256, 384, out_size=(217, 145), fmt=fmt) == (145, 217)
    # a scale: 2 * round(S * side / 2) of the network's input side, even for every format, inside the range
    assert output_size(256, 384, out_scale=2.25, fmt="420") == (144, 216)
    assert output_size(272, 640, out_scale=2.5, fmt="444") == (170, 400)
    assert output_size(1920, 2560, out_scale=2.25, fmt="420") == (1080, 1440)          # 480p -> 1080p
    assert output_size(256, 384, out_scale=1, fmt="420") == (64, 96) and output_size(256, 384, out_scale=4, fmt="420") == (256, 384)
    assert output_size(68, 100, out_scale=1, fmt="444") == (18, 26)                    # odd input sides 17 x 25: the even sizes of the range
    assert output_size(68, 100, out_scale=1.1, fmt="420") == (18, 28)
    for fmt in ("420", "444"):
        for s in (1, 1.3, 2, 2.999, 3.7, 4):
            h, w = output_size(68, 100, out_scale=s, fmt=fmt)
            assert h % 2 == 0 and w % 2 == 0 and 17 <= h <= 68 and 25 <= w <= 100
    for bad in (0.99, 4.01, 0, -2, float("nan")):
        with pytest.raises(ValueError, match="1 to 4"):
            output_size(256, 384, out_scale=bad, fmt="420")
    with pytest.raises(ValueError, match="not both"):
        output_size(256, 384, out_size=(216, 144), out_scale=2.25, fmt="420")
    with pytest.raises(ValueError):
        output_size(256, 384, out_size=(216, 144), fmt="422")


def _main(argv):
    from uav import cli
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        status = cli.main(argv)
    return status, err.getvalue()


def test_parser_and_refusals(tmp_path):
    """A bad value is one line on standard error and exit status 2, before any checkpoint is looked at."""
    from uav import cli
    clip = np.zeros((2, 16, 24, 3), dtype=np.uint8)
    path = str(tmp_path / "clip.npy")
    np.save(path, clip)
    base = ["-i", path, "--pretrained", str(tmp_path / "nowhere"), "--device", "cpu", "-o", str(tmp_path / "out")]
    p = cli.build_parser()
    assert p.parse_args(base).out_size is None and p.parse_args(base).out_scale is None
    assert "--out-size" in p.format_help() and "--out-scale" in p.format_help() and "--out-size" in cli.__doc__ and "--out-scale" in cli.__doc__
    assert cli._out_size_options(p.parse_args(base + ["--out-size", "54x36"])) == ((54, 36), None)
    assert cli._out_size_options(p.parse_args(base + ["--out-size", "54:36"])) == ((54, 36), None)
    assert cli._out_size_options(p.parse_args(base + ["--out-size", "54X36"])) == ((54, 36), None)
    assert cli._out_size_options(p.parse_args(base + ["--out-scale", "2.25"])) == (None, 2.25)
    bad = [["--out-size", "54"], ["--out-size", "54x"], ["--out-size", "x36"], ["--out-size", "54x36x2"], ["--out-size", "a:b"],
           ["--out-size", "5.4x36"], ["--out-size", "0x0"], ["--out-size", "=54x36"],                    # malformed
           ["--out-size", "54x36", "--out-scale", "2"],                                                 # both
           ["--out-scale", "0.5"], ["--out-scale", "4.5"], ["--out-scale", "two"], ["--out-scale", "nan"],
           ["--out-size", "22x16"], ["--out-size", "24x14"], ["--out-size", "98x64"], ["--out-size", "96x66"],      # outside 24x16 .. 96x64
           ["--out-size", "55x36"], ["--out-size", "54x37", "--out-format", "420p10"]]                  # odd sides in 4:2:0
    for extra in bad:
        status, err = _main(base + extra)
        lines = err.strip().splitlines()
        assert status == 2 and len(lines) == 1 and lines[0].startswith("upscale.py: error: --out-s"), (extra, status, err)
    status, err = _main(base + ["--out-size", "98x64"])
    assert "24x16 to 96x64" in err
    # an odd size is fine in 4:4:4: the run gets as far as the missing checkpoints
    status, err = _main(base + ["--out-size", "55x37", "--out-format", "444"])
    assert status == 2 and "--pretrained" in err and "--out-size" not in err
    assert not os.path.exists(str(tmp_path / "out"))


def test_program_resizes_on_the_cpu_stand_ins(tmp_path):
    """The program with `--out-size` / `--out-scale` on the tiny seeded checkpoints (see `_child`)."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-3000:])


# ---- child ---------------------------------------------------------------------------------------------------------------
def _install_colour_fix_stand_ins(ops):
    """torch stand-ins for the colour-fix ops the Wavelet job needs (uav.ops has no CPU path; tests/cpu_ops.py has none of these).
    Both sides of the comparison below run through them."""
    def atrous_blur_f32(x, radius, high=None):
        lead, (h, w) = x.shape[:-2], x.shape[-2:]
        k = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]]) / 16.0
        p = F.pad(x.reshape(-1, 1, h, w), (radius,) * 4, mode="replicate")
        low = F.conv2d(p, k[None, None], dilation=radius).reshape(*lead, h, w)
        if high is not None:
            high += x - low
        return low

    def axpby_f32(x, z, a, b):
        return a * x + b * z

    def resize_bicubic_f32(x, ho, wo, scale_h=None, scale_w=None):
        lead, (h, w) = x.shape[:-2], x.shape[-2:]
        return F.interpolate(x.reshape(1, -1, h, w), size=(ho, wo), mode="bicubic", align_corners=False).reshape(*lead, ho, wo)
    saved = {n: getattr(ops, n) for n in ("atrous_blur_f32", "axpby_f32", "resize_bicubic_f32")}
    ops.atrous_blur_f32, ops.axpby_f32, ops.resize_bicubic_f32 = atrous_blur_f32, axpby_f32, resize_bicubic_f32
    return saved


def _child(tmp):
    import cpu_ops
    import cpu_ops_fmt
    import cpu_ops_io
    import cpu_ops_resize
    from test_cli_dropin_cpu import CASES, _clip_u8, _write_pretrained
    from uav import cli, ops, video_io
    base = _write_pretrained(tmp)
    os.chdir(tmp)
    small = _clip_u8(*CASES["video_vae"][1])                                    # (3,C,16,24) uint8
    np.save("small.npy", small.permute(0, 2, 3, 1).contiguous().numpy())
    tiled = _clip_u8(*CASES["tile"][1])                                         # (2,C,68,160): two tiles at --tile_size 64
    np.save("tiled.npy", tiled.permute(0, 2, 3, 1).contiguous().numpy())
    tall = _clip_u8(1, 184, 16, 38)                                             # 4x is 736 rows: BT.709 by `--matrix auto`; 368 rows are BT.601
    np.save("tall.npy", tall.permute(0, 2, 3, 1).contiguous().numpy())
    a = ["--use_video_vae", "-s", "1", "-n", "100"]
    b = ["--perform_tile", "--tile_size", "64", "-s", "1"]
    ka = dict(steps=1, noise_level=100)
    kb = dict(steps=1, noise_level=120, perform_tile=True, tile_size=64)
    # (input, program options, upscale_clip options, video VAE, size options, (H, W), format, matrix)
    jobs = [("small", a, ka, True, ["--out-size", "54x36"], (36, 54), "420", "bt601"),
            ("small", a, ka, True, ["--out-size", "54:36", "--dump-rgb", "rgb.npy"], (36, 54), "420", "bt601"),
            ("small", a, ka, True, ["--out-scale", "2.25"], (36, 54), "420p10", "bt601"),
            ("small", a, ka, True, ["--out-size", "41x27", "--out-format", "444p10"], (27, 41), "444p10", "bt601"),
            ("small", a + ["--color_fix", "Wavelet"], dict(ka, color_fix="Wavelet"), True, ["--out-scale", "2.5"], (40, 60), "444", "bt601"),
            ("tiled", b, kb, False, ["--out-size", "400x170"], (170, 400), "420", "bt601"),
            ("small", a, ka, True, ["--out-scale", "2.5", "--matrix", "bt709"], (40, 60), "444p10", "bt709"),
            # `--matrix auto` goes by the rows WRITTEN: the file is the BT.601 encoding, though the 4x frames have 736 rows
            ("tall", a, ka, True, ["--out-size", "32x368"], (368, 32), "420", "bt601")]
    cpu_ops.install()
    cpu_ops_io.install()
    cpu_ops_fmt.install()
    cpu_ops_resize.install()
    saved = _install_colour_fix_stand_ins(ops)
    pipes = {}
    try:
        for k, (name, argv, kw, video_vae, size, (h, w), fmt, matrix) in enumerate(jobs):
            source = {"small": small, "tiled": tiled, "tall": tall}[name]
            common = ["-i", name + ".npy", "--pretrained", base, "--device", "cpu", "--fps", "8"] + argv
            extra = [] if "--out-format" in size or fmt == "420" else ["--out-format", fmt]
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                assert cli.main(common + ["-o", f"o{k}"] + size + extra) == 0
            save = f"{name}_n{kw['noise_level']}_g6_s1"
            assert os.listdir(f"o{k}/video") == [save + ".y4m"]                  # the file names do not change
            t, (h1, w1) = source.shape[0], source.shape[-2:]
            assert f"{t} frames {h1}x{w1} -> {h}x{w}, " in out.getvalue(), out.getvalue()
            if video_vae not in pipes:
                pipes[video_vae] = cli.load_pipeline(base, use_video_vae=video_vae, device=torch.device("cpu"))[0]
            pipe = pipes[video_vae]
            opts = dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", guidance_scale=6, **kw)
            clip = video_io.preprocess_frames(source)
            frames = video_io.upscale_clip(pipe, clip, generator=torch.Generator(device="cpu").manual_seed(10), out_size=(h, w), **opts)
            assert frames.shape == (t, 3, h, w) and frames.dtype == torch.float32 and frames.std() > 0.05
            if k in (0, 5):         # ... which is the resize of the 4x frames, chunk by chunk
                full = video_io.upscale_clip(pipe, clip, generator=torch.Generator(device="cpu").manual_seed(10), **opts)
                assert full.shape == (t, 3, 4 * h1, 4 * w1) and torch.equal(frames, ops.resize_aa_f32(full, h, w))
                chunks = list(video_io.upscale_clip_chunks(pipe, clip, generator=torch.Generator(device="cpu").manual_seed(10),
                                                           out_size=(h, w), **opts))
                assert [len(c) for c in chunks] == [min(3, t - s) for s in range(0, t, 3)] and torch.equal(torch.cat(chunks), frames)
            frames = frames.numpy()
            tag = yuv_fmt_ref.FORMATS[fmt][2] if fmt != "420" else "C420jpeg"
            header = f"YUV4MPEG2 W{w} H{h} F8:1 Ip A1:1 {tag} XCOLORRANGE=FULL\n".encode()
            planes = yuv_ref.encode(yuv_fmt_ref.rgb_u8(frames), matrix, True) if fmt == "420" else yuv_fmt_ref.encode(frames, fmt, matrix, True)
            expect = yuv_fmt_ref.file_bytes(planes, header)
            got = open(f"o{k}/video/{save}.y4m", "rb").read()
            sb = 1 if fmt in ("420", "444") else 2
            samples = h * w * 3 if fmt.startswith("444") else h * w * 3 // 2
            assert got.startswith(header) and len(got) == len(header) + t * (6 + samples * sb)
            assert got == expect, f"{name} {size} {fmt}: the file is not the reference's planes of upscale_clip(..., out_size=)"
            if "--dump-rgb" in size:
                assert np.array_equal(np.load("rgb.npy"), yuv_fmt_ref.rgb_u8(frames))
            print(f"{name} {' '.join(size)} {fmt}: {len(got)} bytes ok", flush=True)
        # the 4x size by name is no option at all: the same bytes, from the same path
        calls = []
        real = ops.resize_aa_f32
        ops.resize_aa_f32 = lambda *args: calls.append(args) or real(*args)
        common = ["-i", "small.npy", "--pretrained", base, "--device", "cpu", "--fps", "8"] + a
        for k, extra in enumerate(([], ["--out-size", "96x64"], ["--out-scale", "4"])):
            assert cli.main(common + ["-o", f"same{k}"] + extra) == 0
        ops.resize_aa_f32 = real
        plain = open("same0/video/small_n100_g6_s1.y4m", "rb").read()
        assert plain.startswith(b"YUV4MPEG2 W96 H64 F8:1 ") and not calls
        assert plain == open("same1/video/small_n100_g6_s1.y4m", "rb").read() == open("same2/video/small_n100_g6_s1.y4m", "rb").read()
        # ... and without the option the same clip is BT.709, as before: the two files differ in their matrix
        assert cli.main(["-i", "tall.npy", "--pretrained", base, "--device", "cpu", "--fps", "8", "-o", "tall4x", "--dump-rgb", "tall_rgb.npy"] + a) == 0
        rgb = np.load("tall_rgb.npy")
        assert rgb.shape == (1, 736, 64, 3)
        head = b"YUV4MPEG2 W64 H736 F8:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
        assert open("tall4x/video/tall_n100_g6_s1.y4m", "rb").read() == yuv_fmt_ref.file_bytes(yuv_ref.encode(rgb, "bt709", True), head)
    finally:
        for n, fn in saved.items():
            setattr(ops, n, fn)
        cpu_ops_resize.restore()
        cpu_ops_fmt.restore()
        cpu_ops_io.restore()
        cpu_ops.restore()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
