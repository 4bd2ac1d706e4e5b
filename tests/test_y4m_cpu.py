"""The Y4M front end without a GPU: the fixed-point Y'CbCr tables (uav.video_io.yuv_coefficients) against a numpy reference
of the two conversions (tests/yuv_ref.py), and the YUV4MPEG2 reader / writer."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_ref  # noqa: E402


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
def test_coefficient_table_matches_the_formulas(matrix, full):
    from uav import video_io
    k, c = yuv_ref.table(matrix, full), video_io.yuv_coefficients(matrix, full)
    assert c.forward == tuple(k["fy"] + k["fcb"] + k["fcr"] + [k["yo"]])
    assert c.inverse == (k["yo"], k["iy"], k["rcr"], k["gcb"], k["gcr"], k["bcb"])
    assert all(isinstance(v, int) for v in c.forward + c.inverse)
    assert (c.matrix, c.full_range) == (matrix, full)
    with pytest.raises(ValueError):
        video_io.yuv_coefficients("bt2020", full)


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
def test_grey_ramp_has_neutral_chroma_and_spans_the_range(matrix, full):
    ramp = np.repeat(np.arange(256, dtype=np.uint8), 2)                         # 512 wide: every grey level in one 2x2 block
    rgb = np.broadcast_to(ramp[None, None, :, None], (1, 2, 512, 3)).copy()
    y, cb, cr = yuv_ref.encode(rgb, matrix, full)
    assert (cb == 128).all() and (cr == 128).all()
    lo, hi = (0, 255) if full else (16, 235)
    assert (y.min(), y.max()) == (lo, hi) and y[0, 0, 0] == lo and y[0, 0, -1] == hi
    assert (np.diff(y[0, 0].astype(int)) >= 0).all()


@pytest.mark.parametrize("matrix,full", yuv_ref.PAIRS)
def test_encode_decode_round_trip_on_constant_blocks(matrix, full):
    """On 2x2-constant images the chroma sub-sampling loses nothing, so the round trip shows the arithmetic's own error: at
    most 1 LSB (full range) or 2 LSB (limited: 219 luma / 224 chroma codes for 256 levels), every intermediate inside int32."""
    rng = np.random.default_rng(5)
    blocks = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    blocks[0, 0, :8] = corners                                                 # the extremes of every coefficient sum
    rgb = blocks.repeat(2, axis=1).repeat(2, axis=2)
    peak = []
    y, cb, cr = yuv_ref.encode(rgb, matrix, full, peak=peak)
    back = yuv_ref.decode(y, cb, cr, matrix, full, peak=peak)
    d = np.abs(back.astype(int) - rgb.astype(int))
    print(f"{matrix} full={full}: max {d.max()} mean {d.mean():.3f} LSB, largest intermediate {max(peak)}")
    assert d.max() <= (1 if full else 2)
    assert max(peak) < 2 ** 31


def _planes(t, h, w, seed):
    rng = np.random.default_rng(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return (rng.integers(0, 256, (t, h, w), dtype=np.uint8), rng.integers(0, 256, (t, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (t, ch, cw), dtype=np.uint8))


@pytest.mark.parametrize("t,h,w,fps,full", [(3, 40, 56, Fraction(30000, 1001), True), (2, 37, 51, Fraction(25), False), (1, 1, 1, 8, True)])
def test_write_read_round_trip_is_byte_identical(tmp_path, t, h, w, fps, full):
    import torch
    from uav import video_io
    y, cb, cr = _planes(t, h, w, seed=h)
    path = tmp_path / "a.y4m"
    video_io.write_y4m(path, y, cb, cr, fps, full)
    clip = video_io.read_y4m(path)
    assert np.array_equal(clip.y, y) and np.array_equal(clip.cb, cb) and np.array_equal(clip.cr, cr)
    assert clip.size == (h, w) and clip.full_range is full
    assert isinstance(clip.fps, Fraction) and clip.fps == Fraction(fps)
    assert clip.colorspace == ("C420jpeg" if full else "C420mpeg2")
    again = tmp_path / "b.y4m"
    video_io.write_y4m(again, torch.from_numpy(clip.y), torch.from_numpy(clip.cb), torch.from_numpy(clip.cr), clip.fps, clip.full_range)
    assert again.read_bytes() == path.read_bytes()
    got, got_fps = video_io.read_frames(str(path))
    assert np.array_equal(got.y, y) and got_fps == Fraction(fps)


def test_written_header_is_literal(tmp_path):
    from uav import video_io
    y, cb, cr = _planes(2, 4, 6, seed=1)
    video_io.write_y4m(tmp_path / "f.y4m", y, cb, cr, Fraction(30000, 1001), True)
    video_io.write_y4m(tmp_path / "l.y4m", y, cb, cr, 24, False)
    data = (tmp_path / "f.y4m").read_bytes()
    head = b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
    assert data.startswith(head + b"FRAME\n")
    assert len(data) == len(head) + 2 * (6 + 24 + 6 + 6) and data.count(b"FRAME\n") >= 2
    assert data[len(head) + 6:len(head) + 6 + 24] == y[0].tobytes()
    assert (tmp_path / "l.y4m").read_bytes().startswith(b"YUV4MPEG2 W6 H4 F24:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\nFRAME\n")


def test_hand_written_header_without_c_tag_and_with_frame_parameters(tmp_path):
    from uav import video_io
    y, cb, cr = _planes(2, 3, 5, seed=2)
    body = b"".join(b"FRAME Xsome=param Ip\n" + y[i].tobytes() + cb[i].tobytes() + cr[i].tobytes() for i in range(2))
    path = tmp_path / "hand.y4m"
    path.write_bytes(b"YUV4MPEG2 W5 H3 F25:1 A0:0 Xfoo\n" + body)
    clip = video_io.read_y4m(path)
    assert clip.colorspace == "" and clip.full_range is False and clip.fps == 25 and clip.size == (3, 5)
    assert np.array_equal(clip.y, y) and np.array_equal(clip.cb, cb) and np.array_equal(clip.cr, cr)
    # the range tag wins over the chroma tag's default, in both directions
    path.write_bytes(b"YUV4MPEG2 W5 H3 F25:1 Ip C420jpeg XCOLORRANGE=LIMITED\n" + body)
    assert video_io.read_y4m(path).full_range is False
    path.write_bytes(b"YUV4MPEG2 W5 H3 F25:1 Ip C420mpeg2 XCOLORRANGE=FULL\n" + body)
    assert video_io.read_y4m(path).full_range is True
    for tag in (b"C420paldv", b"C420"):
        path.write_bytes(b"YUV4MPEG2 W5 H3 F25:1 Ip " + tag + b"\n" + body)
        assert video_io.read_y4m(path).full_range is False


def test_c444_file_parses(tmp_path):
    from uav import video_io
    rng = np.random.default_rng(3)
    planes = rng.integers(0, 256, (2, 3, 3, 5), dtype=np.uint8)               # (T, plane, H, W)
    path = tmp_path / "c444.y4m"
    path.write_bytes(b"YUV4MPEG2 W5 H3 F24:1 Ip A1:1 C444\n" + b"".join(b"FRAME\n" + planes[i].tobytes() for i in range(2)))
    clip = video_io.read_y4m(path)
    assert clip.colorspace == "C444" and clip.cb.shape == (2, 3, 5) and clip.full_range is False
    assert np.array_equal(clip.y, planes[:, 0]) and np.array_equal(clip.cb, planes[:, 1]) and np.array_equal(clip.cr, planes[:, 2])


@pytest.mark.parametrize("tag", ["C422", "Cmono", "C420p10", "C444p10", "C444alpha", "It", "Ib", "Im", "XCOLORRANGE=WIDE"])
def test_unsupported_tags_raise_naming_the_tag(tmp_path, tag):
    from uav import video_io
    path = tmp_path / "bad.y4m"
    path.write_bytes(f"YUV4MPEG2 W4 H4 F24:1 {tag}\n".encode() + b"FRAME\n" + bytes(64))
    with pytest.raises(ValueError, match=tag):
        video_io.read_y4m(path)


def test_truncated_and_foreign_files_raise(tmp_path):
    from uav import video_io
    y, cb, cr = _planes(2, 4, 6, seed=4)
    good = tmp_path / "good.y4m"
    video_io.write_y4m(good, y, cb, cr, 24, True)
    data = good.read_bytes()
    cut = tmp_path / "cut.y4m"
    cut.write_bytes(data[:-5])
    with pytest.raises(ValueError, match="truncated"):
        video_io.read_y4m(cut)
    cut.write_bytes(b"RIFF....AVI LIST")
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        video_io.read_y4m(cut)
    cut.write_bytes(data[:data.index(b"\n") + 1])
    with pytest.raises(ValueError, match="FRAME"):
        video_io.read_y4m(cut)
    with pytest.raises(ValueError, match="unsupported input"):
        video_io.read_frames(str(tmp_path / "clip.mp4"))


def test_read_frames_npy_and_image_directory(tmp_path):
    from uav import video_io
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, (3, 6, 8, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", frames)
    got, fps = video_io.read_frames(str(tmp_path / "clip.npy"))
    assert np.array_equal(got, frames) and fps is None
    np.save(tmp_path / "bad.npy", frames.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        video_io.read_frames(str(tmp_path / "bad.npy"))
    Image = pytest.importorskip("PIL.Image")
    folder = tmp_path / "shots"
    folder.mkdir()
    for i in (2, 0, 1):
        Image.fromarray(frames[i]).save(folder / f"{i:04d}.png")
    got, fps = video_io.read_frames(str(folder))
    assert np.array_equal(got, frames) and fps is None
