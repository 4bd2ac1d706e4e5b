"""`--chroma sited` without a GPU: the numpy reference of the two siting-aware 4:2:0 conversions (tests/chroma_sited_ref.py,
written from include/uav_hip.h) against the float64 conversion and against today's replicate / block-mean pair, where a chroma
ramp ends up under each pairing, `video_io.chroma_siting`, the parser, and the program end to end on the CPU stand-ins (in a
child interpreter, as tests/test_out_format_cpu.py does)."""
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
import chroma_sited_ref as ref  # noqa: E402
import yuv_fmt_ref  # noqa: E402
import yuv_ref  # noqa: E402

SHAPES = [(2, 37, 51), (1, 1, 1), (1, 2, 3), (2, 40, 56)]


def _planes(t, h, w, seed):
    rng = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, 256, (t, h, w), dtype=np.uint8)
    cb = rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)
    cr = rng.integers(0, 256, (t, ch, cw), dtype=np.uint8)
    y.reshape(-1)[:4] = [0, 255, 16, 235][:y.size]
    cb.reshape(-1)[:2] = [0, 255][:cb.size]                                    # the extremes of every product
    cr.reshape(-1)[:2] = [255, 0][:cr.size]
    return y, cb, cr


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
@pytest.mark.parametrize("tag", sorted(ref.SITINGS))
def test_decoder_reference_is_within_its_bound_of_the_float64_conversion(tag, matrix, full_range):
    """One rounding of a sum in 1/2^20 steps: 0.5 for the rounding itself, and the coefficients' own rounding (0.5 / 65536 each)
    times at most 255 of luma and 128 of each chroma: 0.5 + (255 + 2 * 128) * 0.5 / 65536 = 0.504 < 0.51 eight-bit steps."""
    worst = 0.0
    for shape in SHAPES:
        y, cb, cr = _planes(*shape, seed=sum(shape))
        peak = []
        rgb = ref.decode(y, cb, cr, matrix, full_range, ref.SITINGS[tag], peak)
        assert rgb.shape == shape + (3,) and rgb.dtype == np.uint8 and peak[0] < 2 ** 31
        exact = np.clip(ref.decode_exact(y, cb, cr, matrix, full_range, ref.SITINGS[tag]), 0, 255)
        worst = max(worst, float(np.abs(rgb.astype(np.float64) - exact).max()))
    print(f"{tag} {matrix} full_range={full_range}: worst {worst:.4f} steps")
    assert worst < 0.51
    # the extremes of all three planes at once: every intermediate still fits int32
    for yv in (0, 255):
        for cbv in (0, 255):
            for crv in (0, 255):
                peak = []
                ref.decode(np.full((1, 2, 2), yv, np.uint8), np.full((1, 1, 1), cbv, np.uint8), np.full((1, 1, 1), crv, np.uint8),
                           matrix, full_range, ref.SITINGS[tag], peak)
                assert peak[0] < 2 ** 31


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
@pytest.mark.parametrize("tag", sorted(ref.SITINGS))
def test_constant_chroma_decodes_as_the_replicate_decoder_does(tag, matrix, full_range):
    """16 * c - 2048 = 16 * (c - 128): sums and rounding constant are today's times 16, the shift is 4 more — the same bytes."""
    for shape in SHAPES:
        y = _planes(*shape, seed=5)[0]
        for cbv, crv in ((128, 128), (0, 255), (255, 0), (90, 201)):
            cb = np.full((shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2), cbv, np.uint8)
            cr = np.full_like(cb, crv)
            assert np.array_equal(ref.decode(y, cb, cr, matrix, full_range, ref.SITINGS[tag]), yuv_ref.decode(y, cb, cr, matrix, full_range))


def test_a_chroma_ramp_is_up_sampled_exactly_at_both_sitings():
    """c[j, i] = 10 + 4 i + 6 j sits at luma (2i, 2j) when co-sited and at (2i + 0.5, 2j + 0.5) when centred; away from the
    clamped borders the up-sampled plane is that ramp at every luma position, exactly (in sixteenths)."""
    h, w = 24, 32
    j, i = np.meshgrid(np.arange(h // 2), np.arange(w // 2), indexing="ij")
    c = (10 + 4 * i + 6 * j).astype(np.uint8)[None]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for siting in ((True, True), (False, True), (False, False), (True, False)):
        dx, dy = (0.5 if siting[0] else 0.0), (0.5 if siting[1] else 0.0)
        want = 16 * 10 + 32 * (xx - dx) + 48 * (yy - dy)                        # 16 * (10 + 4 (x - dx) / 2 + 6 (y - dy) / 2)
        got = ref.upsample16(c, h, w, siting)[0]
        assert np.array_equal(got[2:-2, 2:-2], want[2:-2, 2:-2]), siting
    # odd sizes: chroma planes are ceil, the last luma row / column has a whole sample of its own
    assert ref.upsample16(np.array([[[7]]], np.uint8), 1, 1, (False, True)).tolist() == [[[112]]]
    assert ref.upsample16(np.array([[[0, 16]]], np.uint8), 2, 3, (False, True))[0].tolist() == [[0, 128, 256]] * 2
    assert ref.upsample16(np.array([[[0, 16]]], np.uint8), 2, 3, (True, True))[0].tolist() == [[0, 64, 192]] * 2


def _inputs():
    rng = np.random.default_rng(7)
    noise = (rng.standard_normal((2, 3, 8, 16)) * 0.8).astype(np.float32)
    noise.reshape(-1)[:8] = [-1.0, 1.0, -1.5, 1.5, 0.0, 0.999999, -0.999999, 0.5]
    prim = np.array([[r, g, b] for r in (-1, 1) for g in (-1, 1) for b in (-1, 1)], dtype=np.float32)      # 8 corners of the cube
    prim = np.concatenate([prim, prim * 3])
    corners = np.zeros((1, 3, 8, 16), dtype=np.float32)
    corners[0] = np.repeat(prim.T.reshape(3, 1, 16), 8, axis=1)
    corners[0, :, 1::2] = np.roll(corners[0, :, 1::2], 3, axis=-1)
    flat = [np.repeat(np.repeat(p.reshape(1, 3, 1, 1), 4, axis=2), 6, axis=3) for p in prim[:8]]         # a corner over a whole frame
    return [noise, corners] + flat


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
def test_encoder_reference_keeps_the_luma_and_the_grey_of_the_existing_encoders(matrix, full_range):
    for frames in _inputs():
        peaks = []
        y8, cb8, cr8 = ref.encode(frames, 8, matrix, full_range, peaks)
        y10, cb10, cr10 = ref.encode(frames, 10, matrix, full_range, peaks)
        assert max(peaks) < 2 ** 31
        assert np.array_equal(y8, yuv_ref.encode(yuv_fmt_ref.rgb_u8(frames), matrix, full_range)[0])
        assert np.array_equal(y10, yuv_fmt_ref.encode(frames, "420p10", matrix, full_range)[0])
        t, _, h, w = frames.shape
        for p, dtype, vmax in ((cb8, np.uint8, 255), (cr8, np.uint8, 255), (cb10, np.uint16, 1023), (cr10, np.uint16, 1023)):
            assert p.shape == (t, h // 2, w // 2) and p.dtype == dtype and p.max() <= vmax
    grey = np.full((1, 3, 4, 6), 0.25, dtype=np.float32)
    for depth, centre in ((8, 128), (10, 512)):
        _, cb, cr = ref.encode(grey, depth, matrix, full_range)
        assert (cb == centre).all() and (cr == centre).all()


def _ramp_q(depth, w=32, h=4):
    """(1,h,w,3) integer RGB: R, G constant, B a linear ramp with an even step (6 of 8 bits, 96 of 12)."""
    unit = 1 if depth == 8 else 16
    q = np.zeros((1, h, w, 3), dtype=np.int64)
    q[..., 0], q[..., 1] = 60 * unit, 90 * unit
    q[..., 2] = (20 + 6 * np.arange(w)) * unit
    return q


def _chroma444(q, depth, matrix, full_range):
    """The chroma of every pixel by itself (the 4:4:4 formula of include/uav_hip.h): Cb, Cr (T,H,W)."""
    k, centre, vmax = (yuv_ref.table(matrix, full_range), 128, 255) if depth == 8 else (yuv_fmt_ref.table10(matrix, full_range), 512, 1023)
    return [np.clip((((q * np.array(k[f], dtype=np.int64)).sum(-1) + 32768) >> 16) + centre, 0, vmax) for f in ("fcb", "fcr")]


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
@pytest.mark.parametrize("depth", [8, 10])
def test_encoder_reference_samples_a_ramp_at_the_even_column(depth, matrix, full_range):
    """q[2i-1] + 2 q[2i] + q[2i+1] = 4 q[2i] on a linear ramp, two rows: 8 q[2i], and (8 f.q + 2^18) >> 19 == (f.q + 2^15) >> 16.
    The 2x2 mean is the ramp half a pixel further: (q[2i] + q[2i+1]) / 2 = q[2i] + step / 2."""
    q = _ramp_q(depth)
    _, cb, cr = ref.encode_q(q, depth, matrix, full_range)
    cb444, cr444 = _chroma444(q, depth, matrix, full_range)
    assert np.array_equal(cb[:, :, 1:], cb444[:, ::2, 2::2]) and np.array_equal(cr[:, :, 1:], cr444[:, ::2, 2::2])
    assert len(np.unique(cb[0, 0])) == cb.shape[2]                              # ... and it is a ramp: every sample differs
    half = q.copy()
    half[..., 2] += 3 * (1 if depth == 8 else 16)                               # the ramp at x + 0.5
    hb, hr = _chroma444(half, depth, matrix, full_range)
    if depth == 8:
        _, mb, mr = yuv_ref.encode(q.astype(np.uint8), matrix, full_range)
        assert np.array_equal(mb, hb[:, ::2, ::2]) and np.array_equal(mr, hr[:, ::2, ::2])
        assert not np.array_equal(mb[:, :, 1:], cb[:, :, 1:])


@pytest.mark.parametrize("matrix,full_range", yuv_ref.PAIRS)
def test_where_a_chroma_ramp_ends_up_under_each_pairing(matrix, full_range):
    """Cb of the ramp above is linear in x with slope s = 6 * fcb[2] / 65536 steps per pixel (2.6 to 3).  `d` below is the mean
    over the interior of (up-sampled Cb - that line) / s: where the chroma of luma column x came from, x + d.
      left-sited encoder -> sited decoder under the same tag:  d = 0.   The encoder's samples are the rounded line at 2i (exact,
        previous test), an even column gets that sample and an odd one the mean of two: each within 0.5 steps of the line, so
        |d| <= 0.5 / s < 0.2.
      today's block mean -> sited decoder under the tag written (left):  the samples are the rounded line at 2i + 0.5, so
        d = +0.5 within the same 0.2: the half output pixel of the issue.
      left-sited encoder -> today's replicating decoder:  column x gets the line at 2 (x >> 1): d = 0 for even, -1 for odd x,
        -0.5 on average within 0.2: the half input pixel of the issue."""
    q = _ramp_q(8)
    k = yuv_ref.table(matrix, full_range)
    f = np.array(k["fcb"], dtype=np.float64) / 65536
    line = (q[0, 0].astype(np.float64) * f).sum(-1) + 128                       # Cb of every column, unrounded
    slope = 6 * f[2]
    assert 2.5 < slope <= 3.0 and np.allclose(np.diff(line), slope)
    _, sited_cb, _ = ref.encode_q(q, 8, matrix, full_range)
    _, mean_cb, _ = yuv_ref.encode(q.astype(np.uint8), matrix, full_range)
    h, w = q.shape[1:3]
    inner = slice(2, w - 2)

    def shift(up):                                                             # (h, w) in steps
        return float((up[:, inner] - line[inner]).mean() / slope)
    d_sited = shift(ref.upsample16(sited_cb, h, w, ref.LEFT)[0] / 16.0)
    d_mean = shift(ref.upsample16(mean_cb, h, w, ref.LEFT)[0] / 16.0)
    d_repl = shift(sited_cb.repeat(2, axis=1).repeat(2, axis=2)[0].astype(np.float64))
    d_today = shift(mean_cb.repeat(2, axis=1).repeat(2, axis=2)[0].astype(np.float64))
    print(f"{matrix} full_range={full_range}: sited/sited {d_sited:+.3f}, mean/sited {d_mean:+.3f}, sited/replicate {d_repl:+.3f}, "
          f"mean/replicate {d_today:+.3f} px")
    assert abs(d_sited) < 0.2
    assert abs(d_mean - 0.5) < 0.2
    assert abs(d_repl + 0.5) < 0.2
    assert abs(d_today) < 0.2              # today's two halves cancel between themselves; each is off against a tag-abiding peer


def test_chroma_siting_of_every_accepted_tag():
    from uav import video_io
    assert video_io.chroma_siting("C420jpeg") == (True, True)
    for tag in ("C420mpeg2", "C420", "", "C420p10"):
        assert video_io.chroma_siting(tag) == (False, True)
    assert video_io.chroma_siting("C420paldv") == (False, False)
    for tag, siting in ref.SITINGS.items():
        assert video_io.chroma_siting(tag) == siting
    for tag in video_io._CHROMA_420:                                            # every 4:2:0 tag the reader accepts
        assert len(video_io.chroma_siting(tag)) == 2
    for bad in ("C444", "C422", "C444p10", "mono", None):
        with pytest.raises(ValueError):
            video_io.chroma_siting(bad)
    # what is written: only a left-sited tag has a filter of its own
    for fmt, full, want in (("420", True, None), ("420", False, (False, True)), ("420p10", True, (False, True)),
                            ("420p10", False, (False, True)), ("444", False, None), ("444p10", True, None)):
        assert video_io.output_siting(fmt, full, "sited") == want
        assert video_io.output_siting(fmt, full, "replicate") is None and video_io.output_siting(fmt, full) is None
    with pytest.raises(ValueError):
        video_io.output_siting("420", False, "nearest")
    clip = video_io.Y4MClip(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8), None, (2, 2),
                            "C420mpeg2", False)
    with pytest.raises(ValueError):
        video_io.preprocess_planes(clip, "cpu", "bt601", chroma="nearest")
    with pytest.raises(ValueError):
        video_io.postprocess_planes(torch.zeros(1, 3, 2, 2), video_io.yuv_coefficients("bt601", False), "420", siting=(False, False))
    with pytest.raises(ValueError):
        next(video_io.upscale_clip_chunks(None, torch.zeros(1, 3, 1, 8, 8), prompt="", negative_prompt="", steps=1, guidance_scale=1,
                                          noise_level=1, generator=None, chroma="nearest"))


def test_parser_default_and_choices(capsys):
    from uav import cli
    p = cli.build_parser()
    base = ["-i", "x.y4m", "--pretrained", "d"]
    assert p.parse_args(base).chroma == "replicate"
    for mode in ("replicate", "sited"):
        assert p.parse_args(base + ["--chroma", mode]).chroma == mode
    for bad in ("left", "centre", "Sited", ""):
        with pytest.raises(SystemExit) as e:
            p.parse_args(base + ["--chroma", bad])
        assert e.value.code == 2
    capsys.readouterr()
    assert "--chroma" in p.format_help() and "--chroma" in cli.__doc__


def test_stand_ins_equal_the_reference():
    import cpu_ops_chroma
    from uav import video_io
    for matrix, full in yuv_ref.PAIRS:
        coefs = video_io.yuv_coefficients(matrix, full)
        for shape in SHAPES:
            y, cb, cr = _planes(*shape, seed=3 + sum(shape))
            for siting in ref.SITINGS.values():
                got = cpu_ops_chroma.yuv420_sited_to_clip_f32(*(torch.from_numpy(p) for p in (y, cb, cr)), coefs, siting)
                assert np.array_equal(got.numpy(), ref.clip_of(ref.decode(y, cb, cr, matrix, full, siting)))
        for frames in _inputs():
            for depth in (8, 10):
                got = cpu_ops_chroma.clip_to_yuv420_sited(torch.from_numpy(frames), video_io.yuv_coefficients(matrix, full, depth), depth)
                want = ref.encode(frames, depth, matrix, full)
                assert all(np.array_equal(g.numpy().astype(w.dtype), w) for g, w in zip(got, want))


def test_program_filters_chroma_on_the_cpu_stand_ins(tmp_path):
    """The program with `--chroma sited` / `replicate` / no option on the tiny seeded checkpoints (see `_child`)."""
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), str(tmp_path)], capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-3000:])


# ---- child ---------------------------------------------------------------------------------------------------------------
def _child(tmp):
    import cpu_ops
    import cpu_ops_chroma
    import cpu_ops_fmt
    import cpu_ops_io
    from test_cli_dropin_cpu import CASES, _clip_u8, _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(tmp)
    os.chdir(tmp)
    planes = {}
    for name, case in (("plain", "video_vae"), ("tiled", "tile")):               # (3,16,24) and (2,68,160): two tiles at --tile_size 64
        rgb = _clip_u8(*CASES[case][1]).permute(0, 2, 3, 1).contiguous().numpy()
        planes[name] = yuv_ref.encode(rgb, "bt601", False)
        video_io.write_y4m(name + ".y4m", *planes[name], 8, False)
        assert open(name + ".y4m", "rb").read(80).split(b"\n")[0].endswith(b"C420mpeg2 XCOLORRANGE=LIMITED")
    np.save("clip.npy", _clip_u8(*CASES["video_vae"][1]).permute(0, 2, 3, 1).contiguous().numpy())
    options = {"plain": (["--use_video_vae", "-s", "1", "-n", "100"], dict(steps=1, noise_level=100), True, "n100_g6_s1"),
               "tiled": (["--perform_tile", "--tile_size", "64", "-s", "1"], dict(steps=1, noise_level=120, perform_tile=True, tile_size=64),
                         False, "n120_g6_s1")}
    cpu_ops.install()
    cpu_ops_io.install()
    cpu_ops_fmt.install()
    cpu_ops_chroma.install()
    try:
        for name, (argv, kw, video_vae, save) in options.items():
            y, cb, cr = planes[name]
            t, h, w = y.shape
            pipe = cli.load_pipeline(base, use_video_vae=video_vae, device=torch.device("cpu"))[0]

            def upscaled(rgb):
                clip = video_io.preprocess_frames(torch.from_numpy(rgb).permute(0, 3, 1, 2).contiguous())
                out = video_io.upscale_clip(pipe, clip, prompt="best quality, extremely detailed", negative_prompt="blur, worst quality",
                                            guidance_scale=6, generator=torch.Generator(device="cpu").manual_seed(10), **kw).numpy()
                assert out.shape == (t, 3, 4 * h, 4 * w) and out.std() > 0.05
                return out
            sited = upscaled(ref.decode(y, cb, cr, "bt601", False, ref.LEFT))
            today = upscaled(yuv_ref.decode(y, cb, cr, "bt601", False))
            assert not np.array_equal(sited, today)
            del pipe
            common = ["-i", name + ".y4m", "--pretrained", base, "--device", "cpu"] + argv
            for fmt, depth, tag in (("420", 8, "C420mpeg2"), ("420p10", 10, "C420p10")):
                header = f"YUV4MPEG2 W{4 * w} H{4 * h} F8:1 Ip A1:1 {tag} XCOLORRANGE=LIMITED\n".encode()
                out = f"{name}_{fmt}"
                assert cli.main(common + ["-o", out, "--out-format", fmt, "--chroma", "sited"]) == 0
                assert os.listdir(out + "/video") == [f"{name}_{save}.y4m"]        # the file names do not change
                got = open(f"{out}/video/{name}_{save}.y4m", "rb").read()
                expect = yuv_fmt_ref.file_bytes(ref.encode(sited, depth, "bt601", False), header)
                assert len(got) == len(expect) and got == expect, f"{name} {fmt} sited: the file is not the reference composed by hand"
                print(f"{name} {fmt} sited: {len(got)} bytes ok", flush=True)
                # no option and `replicate`: today's decoder, today's encoder, today's bytes
                old = (yuv_ref.encode(yuv_fmt_ref.rgb_u8(today), "bt601", False) if fmt == "420" else
                       yuv_fmt_ref.encode(today, fmt, "bt601", False))
                for k, extra in enumerate(([], ["--chroma", "replicate"])):
                    assert cli.main(common + ["-o", f"{out}_r{k}", "--out-format", fmt] + extra) == 0
                    got = open(f"{out}_r{k}/video/{name}_{save}.y4m", "rb").read()
                    assert got == yuv_fmt_ref.file_bytes(old, header), f"{name} {fmt} {extra}: the default's bytes changed"
                print(f"{name} {fmt} replicate: ok", flush=True)
        # a `.npy` input is full-range RGB: nothing to up-sample, and 'C420jpeg' out is centre / centre — the block mean
        common = ["-i", "clip.npy", "--pretrained", base, "--device", "cpu", "--fps", "8"] + options["plain"][0]
        assert cli.main(common + ["-o", "npy_plain"]) == 0
        assert cli.main(common + ["-o", "npy_sited", "--chroma", "sited"]) == 0
        plain = open("npy_plain/video/clip_n100_g6_s1.y4m", "rb").read()
        assert plain.startswith(b"YUV4MPEG2 W96 H64 F8:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n")
        assert plain == open("npy_sited/video/clip_n100_g6_s1.y4m", "rb").read()
        print("npy: sited == plain", flush=True)
    finally:
        cpu_ops_chroma.restore()
        cpu_ops_fmt.restore()
        cpu_ops_io.restore()
        cpu_ops.restore()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
