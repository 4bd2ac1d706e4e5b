"""`--scenes auto` without a GPU: the torch stand-in of `ops.clip_scene_stats` against the numpy reference (tests/scene_ref.py),
the cut decision `video_io.scene_cuts` / `SceneCutter` on handcrafted and random statistics, `Y4MReader` against `read_y4m`,
and — in child interpreters, on tiny seeded checkpoints and the CPU stand-ins — `upscale_scenes_chunks` and the program."""
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
import cpu_ops_scene  # noqa: E402
import scene_ref  # noqa: E402
import yuv_ref  # noqa: E402

KERNEL_SHAPES = [(1, 1, 1), (2, 1, 1), (3, 2, 3), (2, 7, 9), (4, 16, 16), (3, 33, 65), (5, 64, 96), (2, 130, 258)]
PIXELS = 1000


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_stand_in_equals_the_reference(shape):
    from uav import video_io
    t, h, w = shape
    clip = (torch.rand(3, t, h, w, generator=torch.Generator().manual_seed(t * h + w)) * 2.6 - 1.3)
    hist, sad = cpu_ops_scene.clip_scene_stats(clip, video_io.yuv_coefficients("bt601", True))
    want_hist, want_sad = scene_ref.stats(clip.numpy())
    assert hist.dtype == torch.int32 and sad.dtype == torch.int64 and tuple(hist.shape) == (t, 64) and tuple(sad.shape) == (t,)
    assert np.array_equal(hist.numpy(), want_hist) and np.array_equal(sad.numpy(), want_sad)
    assert int(sad[0]) == 0 and hist.sum(dim=1).tolist() == [h * w] * t


# ---- scene_cuts on handcrafted statistics ------------------------------------------------------------------------------------------
def _flat(frames, bin_=10):
    """Statistics of `frames` identical frames: every pixel in one bin, no difference."""
    hist = np.zeros((frames, 64), dtype=np.int32)
    hist[:, bin_] = PIXELS
    return np.zeros(frames, dtype=np.int64), hist


def _cut_at(sad, hist, t, bin_, mad=50):
    sad[t] = mad * PIXELS
    hist[t:] = 0
    hist[t:, bin_] = PIXELS


def _both(sad, hist, **kw):
    from uav import video_io
    got = video_io.scene_cuts(sad, hist, PIXELS, **kw)
    assert got == scene_ref.cuts(sad, hist, PIXELS, **{k: v for k, v in kw.items() if k != "final"})
    return got


def test_a_clear_cut_is_a_cut():
    sad, hist = _flat(20)
    _cut_at(sad, hist, 10, 40)
    assert _both(sad, hist) == [10]
    assert _both(sad, hist, final=False) == [10]


def test_motion_and_fades_are_not_cuts():
    sad, hist = _flat(30)
    sad[1:] = 60 * PIXELS                                                       # fast motion: high MAD, the histogram stands still
    assert _both(sad, hist) == []
    sad, hist = _flat(30)
    for i in range(10):                                                         # a fade over 10 frames: a tenth of the pixels per frame
        hist[10 + i:, 10] -= PIXELS // 10
        hist[10 + i:, 40] += PIXELS // 10
    sad[10:20] = 3 * PIXELS
    mad, hd = scene_ref.measures(sad, hist, PIXELS)
    assert hd[10:20].min() == hd[10:20].max() == 0.1 and hist[-1, 40] == PIXELS
    assert _both(sad, hist) == []
    sad[10:20] = 60 * PIXELS                                                    # ... and each criterion alone is not enough either way
    assert _both(sad, hist, threshold=(24.0, 0.30)) == []


def test_close_candidates_and_stubs_stay_with_their_neighbour():
    sad, hist = _flat(30)
    _cut_at(sad, hist, 10, 40)
    _cut_at(sad, hist, 13, 20)                                                  # a second candidate 3 frames on
    assert _both(sad, hist) == [10]
    for t in (1, 5, 7):                                                         # nearer than min_len to the start
        sad, hist = _flat(30)
        _cut_at(sad, hist, t, 40)
        assert _both(sad, hist) == []
    for t in (23, 25, 29):                                                      # ... or to the end
        sad, hist = _flat(30)
        _cut_at(sad, hist, t, 40)
        assert _both(sad, hist) == []
    sad, hist = _flat(30)
    _cut_at(sad, hist, 8, 40)
    _cut_at(sad, hist, 22, 20)                                                  # exactly min_len from either end
    assert _both(sad, hist) == [8, 22]
    assert _both(sad, hist, min_len=9) == []


def test_max_len_forces_splits_and_obeys_the_tail_rule():
    sad, hist = _flat(40)
    assert _both(sad, hist, max_len=12) == [12, 24]                             # 36 would leave a tail of 4 frames
    assert _both(sad, hist, max_len=16) == [16, 32]                             # a tail of exactly min_len frames
    assert _both(sad, hist, max_len=0) == []
    _cut_at(sad, hist, 10, 40)
    assert _both(sad, hist, max_len=12) == [10, 22]                             # counted from the accepted cut; 34 is too near the end
    _cut_at(sad, hist, 12, 20)
    assert _both(sad, hist, max_len=12, min_len=2) == [10, 12, 24, 36]
    from uav import video_io
    with pytest.raises(ValueError):
        video_io.scene_cuts(sad, hist, PIXELS, max_len=4, min_len=8)


def test_thresholds_are_inclusive():
    for sad_t, moved, want in ((24 * PIXELS, 300, [10]), (24 * PIXELS - 1, 300, []), (24 * PIXELS, 299, [])):
        sad, hist = _flat(20)
        sad[10] = sad_t
        hist[10:, 10] -= moved
        hist[10:, 40] += moved
        assert _both(sad, hist, threshold=(24.0, 0.30)) == want, (sad_t, moved)


def _random_statistics(rng):
    frames = int(rng.integers(1, 81))
    pixels = 100
    hist = np.zeros((frames, 64), dtype=np.int32)
    row = rng.multinomial(pixels, np.ones(64) / 64)
    for t in range(frames):
        if rng.random() < 0.3:
            row = rng.multinomial(pixels, rng.dirichlet(np.ones(64) * 0.05))    # a few bins hold everything: large distances
        hist[t] = row
    sad = rng.integers(0, 60 * pixels, frames).astype(np.int64)
    min_len = int(rng.integers(1, 11))
    max_len = int(rng.choice([0, 0, min_len, min_len + int(rng.integers(0, 25))]))
    return sad, hist, pixels, dict(threshold=(float(rng.integers(0, 50)), float(rng.random()) * 0.8), min_len=min_len, max_len=max_len)


def test_the_stream_form_gives_the_whole_form_for_every_way_of_cutting_the_input():
    from uav import video_io
    rng = np.random.default_rng(2024)
    with_cuts = 0
    for _ in range(200):
        sad, hist, pixels, kw = _random_statistics(rng)
        frames = len(sad)
        whole = video_io.scene_cuts(sad, hist, pixels, **kw)
        assert whole == scene_ref.cuts(sad, hist, pixels, **kw), kw
        with_cuts += bool(whole)
        for piece in (1, 5, 48, frames):
            cutter = video_io.SceneCutter(pixels, **kw)
            reported = []
            for i in range(0, frames, piece):
                new = cutter.push(sad[i:i + piece], hist[i:i + piece])
                assert all(cutter.frames - t >= kw["min_len"] for t in new)   # only once min_len further frames are known
                reported += new
                assert reported == video_io.scene_cuts(sad[:cutter.frames], hist[:cutter.frames], pixels, final=False, **kw)
            reported += cutter.finish()
            assert reported == cutter.cuts == whole, (piece, kw)
    assert with_cuts > 100                                                      # the random statistics do produce cuts


# ---- Y4MReader ------------------------------------------------------------------------------------------------------------------------
class _Pipe:
    """A binary stream that cannot seek or tell, and counts what it hands out."""

    def __init__(self, data, name=None):
        self._fh, self.consumed = io.BytesIO(data), 0
        if name is not None:
            self.name = name

    def read(self, n=-1):
        out = self._fh.read(n)
        self.consumed += len(out)
        return out

    def readline(self, n=-1):
        out = self._fh.readline(n)
        self.consumed += len(out)
        return out


def _y4m_bytes(t, h, w, fmt="420", seed=0):
    from uav import video_io
    rng = np.random.default_rng(seed)
    ch, cw = (h, w) if fmt == "444" else ((h + 1) // 2, (w + 1) // 2)
    planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((t, h, w), (t, ch, cw), (t, ch, cw))]
    out = io.BytesIO()
    with video_io.Y4MWriter(out, w, h, "30000/1001", False, fmt) as writer:
        writer.write(*planes)
    return out.getvalue()


def _read_in_pieces(reader, n):
    pieces = []
    while True:
        piece = reader.read(n)
        if piece is None:
            return pieces
        pieces.append(piece)


@pytest.mark.parametrize("fmt,shape", [("420", (5, 7, 9)), ("420", (4, 6, 8)), ("444", (5, 7, 9))])
def test_reader_in_pieces_equals_read_y4m(tmp_path, fmt, shape):
    from uav import video_io
    data = _y4m_bytes(*shape, fmt=fmt, seed=3)
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    whole = video_io.read_y4m(str(path))
    for source in (str(path), _Pipe(data)):
        with video_io.Y4MReader(source) as reader:
            assert (reader.fps, reader.size, reader.colorspace, reader.full_range) == (whole.fps, whole.size, whole.colorspace, whole.full_range)
            assert reader.frames_read == 0
            pieces = _read_in_pieces(reader, 2)
            assert [len(p.y) for p in pieces] == [2] * (shape[0] // 2) + [1] * (shape[0] % 2) and reader.frames_read == shape[0]
            assert reader.read(2) is None
        for name in ("y", "cb", "cr"):
            assert np.array_equal(np.concatenate([getattr(p, name) for p in pieces]), getattr(whole, name))
        assert all(p[3:] == whole[3:] for p in pieces)
    # nothing is read past the frames asked for
    pipe = _Pipe(data)
    reader = video_io.Y4MReader(pipe)
    header = data.index(b"\n") + 1
    assert pipe.consumed == header
    frame = (len(data) - header) // shape[0]
    reader.read(2)
    assert pipe.consumed == header + 2 * frame


def _message(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_reader_raises_what_read_y4m_raises(tmp_path):
    from uav import video_io
    data = _y4m_bytes(3, 6, 8)
    header = data.index(b"\n") + 1
    frame = (len(data) - header) // 3

    def both(blob, name="bad.y4m"):
        path = tmp_path / name
        path.write_bytes(blob)
        want = _message(lambda: video_io.read_y4m(str(path)))
        assert _message(lambda: _read_in_pieces(video_io.Y4MReader(str(path)), 2)) == want
        assert _message(lambda: video_io.read_y4m(_Pipe(blob, "pipe"))) == _message(lambda: _read_in_pieces(video_io.Y4MReader(_Pipe(blob, "pipe")), 2))
        assert _message(lambda: _read_in_pieces(video_io.Y4MReader(_Pipe(blob)), 2)).startswith("<stream>: ")
        return want
    assert "frame 2 is truncated ('FRAME' with 67 of 72 bytes)" in both(data[:-5])
    assert "frame 1 is truncated" in both(data[:header + frame + 6 + 10])
    assert f"'FRAME' expected at byte {header + frame}" in both(data[:header + frame] + b"junk\n" + data[header + frame:])
    assert f"'FRAME' expected at byte {header + 2 * frame}" in both(data[:header + 2 * frame] + b"FRA")
    assert "no 'FRAME' in the file" in both(data[:header])
    for tags, word in (("W8 H6 C420p10", "C420p10"), ("W8 H6 C422", "C422"), ("W8 H6 Cmono", "Cmono"), ("W8 H6 It", "interlaced"),
                       ("W8 H6 Im", "interlaced"), ("H6", "W / H"), ("W8", "W / H"), ("Wx8 H6", "malformed"), ("W8 H6 F30", "malformed"),
                       ("W8 H6 XCOLORRANGE=WIDE", "range tag")):
        assert word in both(f"YUV4MPEG2 {tags}\n".encode() + data[header:])
    assert "not a YUV4MPEG2 file" in both(b"\0\0\0 ftypisom" + data)
    assert "not a YUV4MPEG2 file" in both(b"YUV4MPEG2 W8 H6")                   # no newline at all
    with pytest.raises(OSError):
        video_io.Y4MReader(str(tmp_path / "nowhere.y4m"))


# ---- upscale_scenes_chunks and the program, in child interpreters -----------------------------------------------------------------
def _in_child(check, tmp_path):
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), check, str(tmp_path)],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, f"{check} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"


def test_scene_chunks_equal_clip_chunks_per_scene_with_one_generator(tmp_path):
    """17 frames of 16x24 in two synthetic scenes (9 + 8): the chunks are those of `upscale_clip_chunks` on each scene in turn
    with one shared generator; with thresholds nothing can reach, those of `upscale_clip_chunks` on the whole clip."""
    _in_child("_check_chunks", tmp_path)


def test_program_writes_the_same_bytes_for_a_clip_without_a_cut(tmp_path):
    _in_child("_check_same_bytes", tmp_path)


def test_program_reads_its_input_in_pieces_and_reports_the_scenes(tmp_path):
    """Scenes of 9 and 70 frames through a standard input that counts: the first frames are written before the input has been
    read to its end, and the per-video line names 2 scenes and the cut."""
    _in_child("_check_pieces", tmp_path)


def test_bad_scene_options_end_the_program_with_one_line(tmp_path):
    _in_child("_check_errors", tmp_path)


class _StandIns:
    def __enter__(self):
        import cpu_ops
        import cpu_ops_io
        cpu_ops.install()
        cpu_ops_io.install()
        cpu_ops_scene.install()

    def __exit__(self, *exc):
        import cpu_ops
        import cpu_ops_io
        cpu_ops_scene.restore()
        cpu_ops_io.restore()
        cpu_ops.restore()


def _y4m_of(rgb, fps="24"):
    """(T,h,w,3) uint8 RGB, even sides -> the bytes of a full-range BT.601 4:2:0 file."""
    from uav import video_io
    out = io.BytesIO()
    with video_io.Y4MWriter(out, rgb.shape[2], rgb.shape[1], fps, True) as writer:
        writer.write(*yuv_ref.encode(rgb, "bt601", True))
    return out.getvalue()


def _seen_by_the_network(blob):
    """The clip the program makes of a .y4m input, (1,3,T,h,w), on the stand-ins."""
    from uav import video_io
    with _StandIns():
        return video_io.preprocess_planes(video_io.read_y4m(_Pipe(blob)), "cpu", "auto")


def _check_chunks(tmp_path, monkeypatch):
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(str(tmp_path))
    lengths = [9, 8]
    clip = torch.from_numpy(scene_ref.clip_of(scene_ref.scenes_u8(lengths, 16, 24))).unsqueeze(0)
    assert scene_ref.assert_fixture(clip[0].numpy(), lengths) == [9]
    with _StandIns():
        pipe, _ = cli.load_pipeline(base, device="cpu")
        kw = dict(prompt="best quality", negative_prompt="blur", steps=1, guidance_scale=6, noise_level=120)

        def gen():
            return torch.Generator().manual_seed(10)

        def pieces(n):
            return (clip[:, :, i:i + n] for i in range(0, clip.shape[2], n))
        one = gen()
        want = [c for a, b in ((0, 9), (9, 17)) for c in video_io.upscale_clip_chunks(pipe, clip[:, :, a:b].contiguous(), generator=one, **kw)]
        assert [c.shape[0] for c in want] == [3, 3, 3, 3, 3, 2] and tuple(want[0].shape[1:]) == (3, 64, 96)
        for n in (17, 5):
            chunks = video_io.upscale_scenes_chunks(pipe, pieces(n), generator=gen(), **kw)
            assert chunks.scenes == []
            got = list(chunks)
            assert chunks.scenes == [(0, 9), (9, 17)] and chunks.frames == 17
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), f"pieces of {n}"
        whole = list(video_io.upscale_clip_chunks(pipe, clip, generator=gen(), **kw))
        assert not all(torch.equal(g, w) for g, w in zip(got, whole))          # the cut does change the result
        chunks = video_io.upscale_scenes_chunks(pipe, pieces(5), scene=((256.0, 1.0), 8, 0), generator=gen(), **kw)
        got = list(chunks)
        assert chunks.scenes == [(0, 17)]
        assert len(got) == len(whole) and all(torch.equal(g, w) for g, w in zip(got, whole))
        # planes instead of frames go through unchanged as well
        coefs = video_io.yuv_coefficients("bt601", True)
        planes = list(video_io.upscale_scenes_chunks(pipe, pieces(17), generator=gen(), coefs=coefs, **kw))
        assert all(torch.equal(p, q) for c, w in zip(planes, want) for p, q in zip(c, video_io.postprocess_planes(w, coefs)))
        with pytest.raises(ValueError):
            list(video_io.upscale_scenes_chunks(pipe, iter(()), generator=gen(), **kw))
        with pytest.raises(ValueError):
            video_io.upscale_scenes_chunks(pipe, pieces(5), scene=((24.0, 0.3), 8, 4), generator=gen(), **kw)


def _common(base):
    return ["--use_video_vae", "-s", "1", "--pretrained", base, "--device", "cpu"]


def _check_same_bytes(tmp_path, monkeypatch):
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    blob = _y4m_of(scene_ref.scenes_u8([10], 16, 24))
    assert scene_ref.assert_fixture(_seen_by_the_network(blob)[0].numpy(), [10]) == []
    open("calm.y4m", "wb").write(blob)
    np.save("still.npy", scene_ref.scenes_u8([10], 16, 24))
    out = io.StringIO()
    import contextlib
    with _StandIns(), contextlib.redirect_stdout(out):
        for name in ("calm.y4m", "still.npy"):
            assert cli.main(["-i", name, "-o", "off"] + _common(base)) == 0
            assert cli.main(["-i", name, "-o", "auto", "--scenes", "auto"] + _common(base)) == 0
    for name in ("calm", "still"):
        off = open(f"off/video/{name}_n120_g6_s1.y4m", "rb").read()
        assert off == open(f"auto/video/{name}_n120_g6_s1.y4m", "rb").read() and off.count(b"FRAME\n") >= 10
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
    assert len(lines) == 4 and "scene" not in lines[0] and "scene" not in lines[2]
    assert all("10 frames 16x24 -> 64x96, 1 tile(s), 1 scene(s), " in ln for ln in (lines[1], lines[3])), lines


def _check_pieces(tmp_path, monkeypatch):
    import types
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    lengths = [9, 70]
    blob = _y4m_of(scene_ref.scenes_u8(lengths, 16, 24))
    assert scene_ref.assert_fixture(_seen_by_the_network(blob)[0].numpy(), lengths) == [9]
    assert sum(lengths) > cli.PIECE_FRAMES + 8 + lengths[0]                     # scene 2 reaches beyond one piece and the look-ahead
    pipe = _Pipe(blob)
    monkeypatch.setattr(sys, "stdin", types.SimpleNamespace(buffer=pipe))
    seen = []
    write = video_io.Y4MWriter.write

    def counting_write(self, *planes):
        seen.append((self.frames, pipe.consumed))
        return write(self, *planes)
    monkeypatch.setattr(video_io.Y4MWriter, "write", counting_write)
    import contextlib
    out = io.StringIO()
    with _StandIns(), contextlib.redirect_stdout(out):
        assert cli.main(["-i", "-", "-o", "out", "--scenes", "auto", "--save_image"] + _common(base)) == 0
    frame = (len(blob) - blob.index(b"\n") - 1) // sum(lengths)
    assert seen[0] == (0, blob.index(b"\n") + 1 + cli.PIECE_FRAMES * frame) and seen[0][1] < len(blob), seen[0]
    assert [c for f, c in seen if f < 9] == [seen[0][1]] * 3                    # the whole first scene is written from the first piece
    assert pipe.consumed == len(blob)
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
    assert len(lines) == 1 and "stdin: 79 frames 16x24 -> 64x96, 1 tile(s), 2 scene(s) (cuts at 9), " in lines[0], lines
    written = video_io.read_y4m("out/video/stdin_n120_g6_s1.y4m")
    assert written.y.shape == (79, 64, 96)
    assert sorted(os.listdir("out/frame/stdin_n120_g6_s1")) == [f"{i:04d}.png" for i in range(79)]     # numbered through the scenes
    # an input cut short in a later piece ends the program with one line and no output file
    err = io.StringIO()
    monkeypatch.setattr(sys, "stdin", types.SimpleNamespace(buffer=_Pipe(blob[:-7])))
    with _StandIns(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        assert cli.main(["-i", "-", "-o", "short", "--scenes", "auto"] + _common(base)) == 2
    lines = [ln for ln in err.getvalue().splitlines() if "Loading weights" not in ln and ln.strip()]     # (the checkpoints' progress bars)
    assert len(lines) == 1 and lines[0].startswith("upscale.py: error: ") and "frame 78 is truncated" in lines[0], err.getvalue()
    assert os.listdir("short/video") == []


def _check_errors(tmp_path, monkeypatch):
    import contextlib
    from uav import cli
    monkeypatch.chdir(tmp_path)
    np.save("clip.npy", scene_ref.scenes_u8([2], 16, 24))
    common = ["-i", "clip.npy", "--pretrained", "no_checkpoints_here", "--device", "cpu"]
    for extra, word in ((["--scene-threshold", "soft"], "--scene-threshold"), (["--scene-threshold", "24"], "--scene-threshold"),
                        (["--scene-threshold=-1:0.3"], "--scene-threshold"), (["--scene-threshold", "24:1.5"], "--scene-threshold"),
                        (["--scene-threshold", "24:-0.1"], "--scene-threshold"), (["--scene-threshold", "nan:0.3"], "--scene-threshold"),
                        (["--scene-threshold", "24:0.3:1"], "--scene-threshold"), (["--scene-min", "0"], "--scene-min"),
                        (["--scene-min", "few"], "--scene-min"), (["--scene-max", "4"], "--scene-max"),
                        (["--scene-min", "12", "--scene-max", "11"], "--scene-max"), (["--scene-max=-3"], "--scene-max")):
        for scenes in (["--scenes", "auto"], []):
            err = io.StringIO()
            with contextlib.redirect_stderr(err):
                assert cli.main(common + scenes + extra) == 2, extra
            lines = err.getvalue().strip().splitlines()
            assert len(lines) == 1 and lines[0].startswith(f"upscale.py: error: {word}: "), (extra, err.getvalue())
    err = io.StringIO()                                                         # good values get as far as the checkpoints
    with contextlib.redirect_stderr(err):
        assert cli.main(common + ["--scenes", "auto", "--scene-threshold", "30:0.5", "--scene-min", "4", "--scene-max", "4"]) == 2
    assert "--pretrained" in err.getvalue()
    # with `auto`, an unreadable input still fails before the checkpoints are looked at
    open("ten.y4m", "wb").write(b"YUV4MPEG2 W4 H4 F24:1 Ip C420p10\nFRAME\n" + bytes(48))
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        assert cli.main(["-i", "ten.y4m", "--scenes", "auto"] + common[2:]) == 2
    assert len(err.getvalue().strip().splitlines()) == 1 and "C420p10" in err.getvalue()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    with pytest.MonkeyPatch.context() as mp:
        from pathlib import Path
        {"_check_chunks": _check_chunks, "_check_same_bytes": _check_same_bytes, "_check_pieces": _check_pieces,
         "_check_errors": _check_errors}[sys.argv[1]](Path(sys.argv[2]), mp)
