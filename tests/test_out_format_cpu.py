"""The output formats beside 8-bit 4:2:0 (`--out-format 444|420p10|444p10`) without a GPU: the numpy reference
(tests/yuv_fmt_ref.py, written from include/uav_hip.h) against the float64 conversion, the coefficient tables, the Y4M header
and writer, the parser, and the program end to end on the CPU stand-ins (in a child interpreter, as
tests/test_upscale_cli_cpu.py does)."""
import io
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
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402

NEW = ("444", "420p10", "444p10")


def _inputs():
    """(T,3,H,W) fp32: +-1, values outside [-1,1], the saturated primaries and their complements, a grey ramp through every
    12-bit level (x = 2 q / 4095 - 1 and the midpoints between levels) and noise."""
    rng = np.random.default_rng(3)
    noise = (rng.standard_normal((2, 3, 8, 16)) * 0.8).astype(np.float32)
    noise.reshape(-1)[:8] = [-1.0, 1.0, -1.5, 1.5, 0.0, 0.999999, -0.999999, 0.5]
    prim = np.array([[r, g, b] for r in (-1, 1) for g in (-1, 1) for b in (-1, 1)], dtype=np.float32)      # 8 corners of the cube
    prim = np.concatenate([prim, prim * 3])                                                              # ... and beyond them
    corners = np.zeros((1, 3, 8, 16), dtype=np.float32)
    corners[0] = np.repeat(prim.T.reshape(3, 1, 16), 8, axis=1)
    corners[0, :, 1::2] = np.roll(corners[0, :, 1::2], 3, axis=-1)           # 2x2 blocks that mix primaries
    levels = np.arange(8192, dtype=np.float64) / 2                             # 0, 0.5, 1, ... 4095.5
    ramp = (2 * levels / 4095 - 1).astype(np.float32).reshape(1, 1, 64, 128).repeat(3, axis=1)
    tint = ramp.copy()
    tint[:, 1] = ramp[:, 1, ::-1]                                              # colour ramps: G against R, B constant per row
    tint[:, 2] = ramp[:, 2, :, :1]
    return [noise, corners, ramp, tint]


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
@pytest.mark.parametrize("fmt", ["420p10", "444p10"])
def test_ten_bit_reference_is_within_its_bound_of_the_float64_conversion(fmt, matrix, full_range):
    """0.5 (final rounding) + 0.11 (12-bit RGB: half a 12-bit step is 0.125 10-bit steps, times the largest row sum of the
    matrix's magnitudes scaled by the range) + 0.09 (coefficient rounding: 3 entries x 0.5 / 65536 x 4095, x 4 / 4 in 4:2:0)
    < 0.75 ten-bit steps; every intermediate fits int32."""
    worst, levels = 0.0, set()
    for frames in _inputs():
        peak = []
        planes = yuv_fmt_ref.encode(frames, fmt, matrix, full_range, peak)
        assert peak[0] < 2 ** 31
        for p, e in zip(planes, yuv_fmt_ref.exact(frames, fmt, matrix, full_range)):
            assert p.dtype == np.uint16 and p.shape == e.shape and p.max() <= 1023
            worst = max(worst, float(np.abs(p.astype(np.float64) - np.clip(e, 0, 1023)).max()))
        levels |= set(np.unique(yuv_fmt_ref.rgb_q12(frames)).tolist())
    print(f"{fmt} {matrix} full_range={full_range}: worst {worst:.3f} ten-bit steps")
    assert levels == set(range(4096)), "the inputs miss 12-bit levels"
    assert worst < 0.75


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
def test_444_reference_shares_its_luma_with_the_420_encoder(matrix, full_range):
    for frames in _inputs():
        y, cb, cr = yuv_fmt_ref.encode(frames, "444", matrix, full_range)
        rgb = yuv_fmt_ref.rgb_u8(frames)
        assert np.array_equal(y, yuv_ref.encode(rgb, matrix, full_range)[0])
        assert y.dtype == cb.dtype == np.uint8 and cb.shape == cr.shape == y.shape
        # grey has no chroma, and a 4:4:4 sample is within the 8-bit path's own error (1 step: two roundings) of the 4:2:0 mean
    grey = np.full((1, 3, 4, 4), 0.25, dtype=np.float32)
    _, cb, cr = yuv_fmt_ref.encode(grey, "444", matrix, full_range)
    assert (cb == 128).all() and (cr == 128).all()
    _, cb, cr = yuv_fmt_ref.encode(grey, "444p10", matrix, full_range)
    assert (cb == 512).all() and (cr == 512).all()


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
def test_coefficient_tables(matrix, full_range):
    from uav import video_io
    k = yuv_ref.table(matrix, full_range)
    today = video_io.YuvCoefs(matrix, full_range, tuple(k["fy"] + k["fcb"] + k["fcr"] + [k["yo"]]),
                              (k["yo"], k["iy"], k["rcr"], k["gcb"], k["gcr"], k["bcb"]))
    for got in (video_io.yuv_coefficients(matrix, full_range), video_io.yuv_coefficients(matrix, full_range, depth=8),
                video_io.yuv_coefficients(matrix, full_range, 8)):
        assert got == today and type(got) is video_io.YuvCoefs and got._fields == ("matrix", "full_range", "forward", "inverse")
    k = yuv_fmt_ref.table10(matrix, full_range)
    ten = video_io.yuv_coefficients(matrix, full_range, depth=10)
    assert ten.forward == tuple(k["fy"] + k["fcb"] + k["fcr"] + [k["yo"]]) and ten.depth == 10
    assert (ten.matrix, ten.full_range) == (matrix, full_range)
    assert sum(k["fcb"]) in (-1, 0, 1) and sum(k["fcr"]) in (-1, 0, 1)      # grey stays at the centre
    with pytest.raises(ValueError):
        video_io.yuv_coefficients(matrix, full_range, depth=12)


def test_header_tags_per_format():
    from uav import video_io
    assert video_io.y4m_header(6, 4, 24, True) == b"YUV4MPEG2 W6 H4 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    assert video_io.y4m_header(6, 4, 24, False, fmt="420") == b"YUV4MPEG2 W6 H4 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n"
    for fmt, (chroma444, depth, tag) in yuv_fmt_ref.FORMATS.items():
        for full in (True, False):
            rng = "FULL" if full else "LIMITED"
            assert video_io.y4m_header(6, 4, "30000/1001", full, fmt=fmt) == f"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 {tag} XCOLORRANGE={rng}\n".encode()
        d = video_io.OUT_FORMATS[fmt]
        assert (d.name, d.chroma444, d.depth, d.tag, d.sample_bytes) == (fmt, chroma444, depth, tag, depth // 8 + (depth % 8 > 0))
    assert sorted(video_io.OUT_FORMATS) == ["420", "420p10", "444", "444p10"]
    with pytest.raises(ValueError):
        video_io.y4m_header(6, 4, 24, True, fmt="422")


def _planes(fmt, t=2, h=4, w=6, seed=0):
    chroma444, depth, _ = yuv_fmt_ref.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    dtype = np.uint8 if depth == 8 else np.uint16
    ch, cw = (h, w) if chroma444 else (h // 2, w // 2)
    return [rng.integers(0, 1 << depth, s, dtype=dtype) for s in ((t, h, w), (t, ch, cw), (t, ch, cw))]


@pytest.mark.parametrize("as_tensor", [False, True])
@pytest.mark.parametrize("fmt", NEW)
def test_writer_frame_sizes_and_byte_order(fmt, as_tensor, tmp_path):
    from uav import video_io
    chroma444, depth, tag = yuv_fmt_ref.FORMATS[fmt]
    y, cb, cr = _planes(fmt)
    y[0, 0, :2] = [(1 << depth) - 1, 1]                                        # 10 bits: FF 03 01 00 in the file
    give = [torch.from_numpy(p.astype(np.int16) if depth == 10 else p) for p in (y, cb, cr)] if as_tensor else [y, cb, cr]
    path = str(tmp_path / "out.y4m")
    with video_io.Y4MWriter(path, 6, 4, 24, False, fmt=fmt) as out:
        out.write(*(p[:1] for p in give))
        out.write(*(p[1:] for p in give))
        assert out.frames == 2
    data = open(path, "rb").read()
    assert not os.path.exists(path + ".part")
    header = f"YUV4MPEG2 W6 H4 F24:1 Ip A1:1 {tag} XCOLORRANGE=LIMITED\n".encode()
    assert data.startswith(header)
    sb = 2 if depth == 10 else 1
    csz = 24 if chroma444 else 6
    frame = (24 + 2 * csz) * sb
    assert len(data) == len(header) + 2 * (6 + frame)
    if depth == 10:
        assert data[len(header) + 6:len(header) + 10] == b"\xff\x03\x01\x00"
    pos = len(header)
    for i in range(2):                                                         # parsed back by hand
        assert data[pos:pos + 6] == b"FRAME\n"
        s = np.frombuffer(data, dtype="<u2" if depth == 10 else np.uint8, count=24 + 2 * csz, offset=pos + 6)
        assert np.array_equal(s[:24], y[i].ravel()) and np.array_equal(s[24:24 + csz], cb[i].ravel()) and np.array_equal(s[24 + csz:], cr[i].ravel())
        pos += 6 + frame
    assert data == yuv_fmt_ref.file_bytes((y, cb, cr), header)
    # write_y4m is one Writer.write; the reader keeps refusing what it cannot decode, naming the tag
    video_io.write_y4m(str(tmp_path / "again.y4m"), *give, 24, False, fmt=fmt)
    assert open(str(tmp_path / "again.y4m"), "rb").read() == data
    if depth == 10:
        with pytest.raises(ValueError, match=tag):
            video_io.read_y4m(path)
    else:
        clip = video_io.read_y4m(path)
        assert clip.colorspace == "C444" and np.array_equal(clip.cb, cb) and np.array_equal(clip.y, y)


@pytest.mark.parametrize("fmt", NEW)
def test_writer_refusals_leave_no_file_behind(fmt, tmp_path):
    from uav import video_io
    chroma444, depth, _ = yuv_fmt_ref.FORMATS[fmt]
    good = _planes(fmt)
    other = _planes("420p10" if chroma444 else "444p10")                       # the other chroma layout
    wrong_dtype = [p.astype(np.uint8 if depth == 10 else np.uint16) for p in good]
    bad = [other if depth == 10 else [p.astype(np.uint8) for p in other], wrong_dtype, [torch.from_numpy(p.astype(np.float32)) for p in good],
           [good[0][:, :2], good[1], good[2]], [good[0], good[1], good[2][:, :1]]]
    if depth == 10:
        bad.append([torch.from_numpy(p.astype(np.int16)).to(torch.uint8) for p in good])
    else:
        bad.append([torch.from_numpy(p).to(torch.int16) for p in good])
    for k, planes in enumerate(bad):
        path = str(tmp_path / f"bad{k}.y4m")
        with pytest.raises(ValueError):
            with video_io.Y4MWriter(path, 6, 4, 24, True, fmt=fmt) as out:
                out.write(*planes)
        with pytest.raises(ValueError):
            video_io.write_y4m(path, *planes, 24, True, fmt=fmt)
        assert os.listdir(str(tmp_path)) == [], f"case {k} left {os.listdir(str(tmp_path))}"
    with pytest.raises(ValueError):
        video_io.Y4MWriter(io.BytesIO(), 6, 4, 24, True, fmt="422")
    # the default format refuses the new formats' planes as it always did
    with pytest.raises(ValueError):
        video_io.write_y4m(str(tmp_path / "d.y4m"), *good, 24, True)
    assert os.listdir(str(tmp_path)) == []


def test_parser_default_and_choices(capsys):
    from uav import cli
    p = cli.build_parser()
    base = ["-i", "x.y4m", "--pretrained", "d"]
    assert p.parse_args(base).out_format == "420"
    for fmt in ("420",) + NEW:
        assert p.parse_args(base + ["--out-format", fmt]).out_format == fmt
    for bad in ("422", "420p12", "mono", ""):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--out-format", bad])
    capsys.readouterr()
    assert "--out-format" in p.format_help() and "--out-format" in cli.__doc__


def test_program_writes_every_format_on_the_cpu_stand_ins(tmp_path):
    """`--use_video_vae -s 1 -n 100` on the 3-frame 16x24 clip, once per format: each file holds exactly the reference's planes
    of the fp32 frames `upscale_clip` gives for the same job; `--out-format 420` and no option give the same bytes."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-2000:])


# ---- child ---------------------------------------------------------------------------------------------------------------
def _child(tmp):
    import cpu_ops
    import cpu_ops_fmt
    import cpu_ops_io
    from test_cli_dropin_cpu import CASES, _clip_u8, _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(tmp)
    os.chdir(tmp)
    clip_u8 = _clip_u8(*CASES["video_vae"][1])                                  # (T,C,H,W) uint8
    np.save("clip.npy", clip_u8.permute(0, 2, 3, 1).contiguous().numpy())
    common = ["-i", "clip.npy", "--use_video_vae", "-s", "1", "-n", "100", "--pretrained", base, "--device", "cpu", "--fps", "8"]
    cpu_ops.install()
    cpu_ops_io.install()
    cpu_ops_fmt.install()
    try:
        pipe, _ = cli.load_pipeline(base, use_video_vae=True, device=torch.device("cpu"))
        frames = video_io.upscale_clip(pipe, video_io.preprocess_frames(clip_u8), prompt="best quality, extremely detailed",
                                       negative_prompt="blur, worst quality", steps=1, guidance_scale=6, noise_level=100,
                                       generator=torch.Generator(device="cpu").manual_seed(10)).numpy()
        assert frames.shape == (3, 3, 64, 96) and frames.dtype == np.float32 and frames.std() > 0.05
        del pipe
        jobs = (("444", "bt601", []), ("420p10", "bt709", ["--matrix", "bt709"]), ("444p10", "bt601", []),
                ("444p10", "bt601", ["--dump-rgb", "rgb.npy"]))                  # ... and through the fp32 canvas of a chunk
        for k, (fmt, matrix, extra) in enumerate(jobs):
            assert cli.main(common + ["-o", f"o{k}", "--out-format", fmt] + extra) == 0
            out = f"o{k}/video/clip_n100_g6_s1.y4m"
            assert os.listdir(f"o{k}/video") == ["clip_n100_g6_s1.y4m"]
            header = f"YUV4MPEG2 W96 H64 F8:1 Ip A1:1 {yuv_fmt_ref.FORMATS[fmt][2]} XCOLORRANGE=FULL\n".encode()
            expect = yuv_fmt_ref.file_bytes(yuv_fmt_ref.encode(frames, fmt, matrix, True), header)
            got = open(out, "rb").read()
            assert len(got) == len(expect) and got == expect, f"{fmt} {extra}: the file is not the reference's planes of the fp32 frames"
            print(f"{fmt} {matrix} {extra}: {len(got)} bytes ok", flush=True)
        assert np.array_equal(np.load("rgb.npy"), yuv_fmt_ref.rgb_u8(frames))   # --dump-rgb stays uint8 RGB
        assert cli.main(common + ["-o", "plain"]) == 0
        assert cli.main(common + ["-o", "flag", "--out-format", "420"]) == 0
        plain = open("plain/video/clip_n100_g6_s1.y4m", "rb").read()
        assert plain == open("flag/video/clip_n100_g6_s1.y4m", "rb").read()
        header = b"YUV4MPEG2 W96 H64 F8:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
        assert plain == yuv_fmt_ref.file_bytes(yuv_ref.encode(yuv_fmt_ref.rgb_u8(frames), "bt601", True), header)
        # a frame no taller than the tiles' overlap has NO tile (tiling.tile_grid, the reference program's rule): black frames,
        # i.e. the planes of an all-zero clip, in every format
        black = np.zeros_like(frames)
        for fmt, expect in (("420", yuv_fmt_ref.file_bytes(yuv_ref.encode(yuv_fmt_ref.rgb_u8(black), "bt601", True), header)),
                            ("444p10", yuv_fmt_ref.file_bytes(yuv_fmt_ref.encode(black, "444p10", "bt601", True), header.replace(b"C420jpeg", b"C444p10")))):
            assert cli.main(common + ["-o", "none" + fmt, "--out-format", fmt, "--perform_tile", "--tile_size", "64"]) == 0
            assert open(f"none{fmt}/video/clip_n100_g6_s1.y4m", "rb").read() == expect
    finally:
        cpu_ops_fmt.restore()
        cpu_ops_io.restore()
        cpu_ops.restore()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
