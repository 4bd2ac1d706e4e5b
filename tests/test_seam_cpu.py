"""`--scene-overlap` without a GPU: which cuts `SceneCutter` calls forced, the torch stand-in of `ops.frame_axpby_f32` against
numpy, and — in child interpreters, on tiny seeded checkpoints and the CPU stand-ins — the cross-fade of `upscale_scenes_chunks`
against its composition restated by hand, and the program.  Every comparison is exact."""
import contextlib
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
import cpu_ops_seam  # noqa: E402
import scene_ref  # noqa: E402
import yuv_ref  # noqa: E402

PIXELS = 1000
LENGTHS, H, W = [12, 14], 16, 24                                                # the fixture: a cut at 12 in 26 frames
SCENE = ((24.0, 0.30), 4, 8)                                                    # min_len 4, max_len 8: cuts at 8 (forced), 12, 20 (forced)
CLIPS = [(0, 10), (8, 12), (12, 22), (20, 26)]                                  # what runs with overlap = 2


# ---- SceneCutter.forced -------------------------------------------------------------------------------------------------------------
def _flat(frames, bin_=10):
    hist = np.zeros((frames, 64), dtype=np.int32)
    hist[:, bin_] = PIXELS
    return np.zeros(frames, dtype=np.int64), hist


def _cut_at(sad, hist, t, bin_, mad=50):
    sad[t] = mad * PIXELS
    hist[t:] = 0
    hist[t:, bin_] = PIXELS


def _cuts_and_forced(sad, hist, pixels=PIXELS, **kw):
    """(cuts, forced) of the whole form, which must leave the plain result as it is and equal the streamed form for every split."""
    from uav import video_io
    cuts, forced = video_io.scene_cuts(sad, hist, pixels, forced=True, **kw)
    assert cuts == video_io.scene_cuts(sad, hist, pixels, **kw) == scene_ref.cuts(sad, hist, pixels, **kw)
    assert [c for c in cuts if c in forced] == forced
    for piece in (1, 3, 5, 48):
        cutter = video_io.SceneCutter(pixels, **kw)
        for i in range(0, len(sad), piece):
            cutter.push(sad[i:i + piece], hist[i:i + piece])
        cutter.finish()
        assert (cutter.cuts, cutter.forced) == (cuts, forced), (piece, kw)
    return cuts, forced


def test_without_candidates_every_cut_is_forced():
    sad, hist = _flat(40)
    assert _cuts_and_forced(sad, hist, max_len=8) == ([8, 16, 24, 32], [8, 16, 24, 32])
    assert _cuts_and_forced(sad, hist, max_len=12) == ([12, 24], [12, 24])
    assert _cuts_and_forced(sad, hist, max_len=0) == ([], [])


def test_a_candidate_at_start_plus_max_len_counts_as_detected():
    sad, hist = _flat(40)
    _cut_at(sad, hist, 8, 40)                                                   # exactly where max_len = 8 would split
    assert _cuts_and_forced(sad, hist, max_len=8) == ([8, 16, 24, 32], [16, 24, 32])
    _cut_at(sad, hist, 20, 20)                                                  # inside a forced scene: counted from the forced cut at 16
    assert _cuts_and_forced(sad, hist, max_len=8, min_len=4) == ([8, 16, 20, 28, 36], [16, 28, 36])
    sad, hist = _flat(26)
    _cut_at(sad, hist, 12, 40)                                                  # the shape of the composition fixture
    assert _cuts_and_forced(sad, hist, max_len=8, min_len=4) == ([8, 12, 20], [8, 20])


def test_forced_is_the_same_for_every_way_of_cutting_random_statistics():
    rng = np.random.default_rng(77)
    some = 0
    for _ in range(100):
        frames, pixels = int(rng.integers(1, 81)), 100
        hist = np.zeros((frames, 64), dtype=np.int32)
        row = rng.multinomial(pixels, np.ones(64) / 64)
        for t in range(frames):
            if rng.random() < 0.2:
                row = rng.multinomial(pixels, rng.dirichlet(np.ones(64) * 0.05))
            hist[t] = row
        sad = rng.integers(0, 60 * pixels, frames).astype(np.int64)
        min_len = int(rng.integers(1, 9))
        kw = dict(threshold=(float(rng.integers(0, 50)), float(rng.random()) * 0.8), min_len=min_len, max_len=min_len + int(rng.integers(0, 12)))
        cuts, forced = _cuts_and_forced(sad, hist, pixels, **kw)
        mad, hd = scene_ref.measures(sad, hist, pixels)
        assert all(not (mad[t] >= kw["threshold"][0] and hd[t] >= kw["threshold"][1]) for t in forced)     # never a candidate
        some += bool(forced) and len(forced) < len(cuts)
    assert some > 10                                                            # both kinds do occur together


# ---- the stand-in -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (3, 189), (4, 3, 8, 8)])
def test_stand_in_equals_numpy(shape):
    g = torch.Generator().manual_seed(sum(shape))
    a, b = (torch.rand(shape, generator=g) * 2.6 - 1.3 for _ in range(2))
    a.reshape(-1)[0], b.reshape(-1)[0] = -0.0, 0.0
    k = shape[0]
    wa = torch.tensor([(k - j) / (k + 1) for j in range(k)], dtype=torch.float32)
    wb = torch.tensor([(j + 1) / (k + 1) for j in range(k)], dtype=torch.float32)
    col = (k,) + (1,) * (len(shape) - 1)
    want = wa.numpy().reshape(col) * a.numpy() + wb.numpy().reshape(col) * b.numpy()
    assert want.dtype == np.float32
    assert np.array_equal(cpu_ops_seam.frame_axpby_f32(a, b, wa, wb).numpy().view(np.uint32), want.view(np.uint32))
    ta, tb = a.clone(), b.clone()                                               # in place, over either input
    assert cpu_ops_seam.frame_axpby_f32(ta, b, wa, wb, out=ta) is ta and cpu_ops_seam.frame_axpby_f32(a, tb, wa, wb, out=tb) is tb
    assert np.array_equal(ta.numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(tb.numpy().view(np.uint32), want.view(np.uint32))


# ---- upscale_scenes_chunks and the program, in child interpreters -----------------------------------------------------------------
def _in_child(check, tmp_path):
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), check, str(tmp_path)],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, f"{check} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"


def test_forced_splits_are_cross_faded_and_detected_cuts_stay_hard(tmp_path):
    """26 frames of 16x24 with a cut at 12, min_len 4, max_len 8, overlap 2: the chunks equal `upscale_clip` on [0,10), [8,12),
    [12,22), [20,26) with one generator, cross-faded at 8 and 20 by hand — as fp32 frames and as planes of two formats —, whatever
    the pieces; overlap = 0 is the call without the keyword; overlap > min_len raises."""
    _in_child("_check_composition", tmp_path)


def test_program_cross_fades_and_reports_it(tmp_path):
    _in_child("_check_program", tmp_path)


def test_bad_overlap_ends_the_program_with_one_line(tmp_path):
    _in_child("_check_errors", tmp_path)


class _StandIns:
    def __enter__(self):
        import cpu_ops
        import cpu_ops_fmt
        import cpu_ops_io
        import cpu_ops_scene
        self._mods = (cpu_ops, cpu_ops_io, cpu_ops_fmt, cpu_ops_scene, cpu_ops_seam)
        for m in self._mods:
            m.install()

    def __exit__(self, *exc):
        for m in reversed(self._mods):
            m.restore()


def _weights(k):
    wa = torch.tensor([(k - j) / (k + 1) for j in range(k)], dtype=torch.float32).view(k, 1, 1, 1)
    wb = torch.tensor([(j + 1) / (k + 1) for j in range(k)], dtype=torch.float32).view(k, 1, 1, 1)
    return wa, wb


def _composition(pipe, clip, generator, **kw):
    """The 26 expected frames, restated by hand from `video_io.upscale_clip` on CLIPS in order with one generator; also frame 0
    of the third clip, the one after the detected cut."""
    from uav import video_io
    one, two, three, four = (video_io.upscale_clip(pipe, clip[:, :, a:b].contiguous(), generator=generator, **kw) for a, b in CLIPS)
    assert [len(c) for c in (one, two, three, four)] == [10, 4, 10, 6]
    wa, wb = _weights(2)
    frames = torch.cat([one[:8], wa * one[8:10] + wb * two[:2], two[2:4], three[:8], wa * three[8:10] + wb * four[:2], four[2:]])
    assert frames.shape[0] == 26 and frames.dtype == torch.float32
    return frames, three[0]


def _check_composition(tmp_path, monkeypatch):
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(str(tmp_path))
    clip = torch.from_numpy(scene_ref.clip_of(scene_ref.scenes_u8(LENGTHS, H, W))).unsqueeze(0)
    assert scene_ref.assert_fixture(clip[0].numpy(), LENGTHS) == [12]
    with _StandIns():
        pipe, _ = cli.load_pipeline(base, device="cpu")
        kw = dict(prompt="best quality", negative_prompt="blur", steps=1, guidance_scale=6, noise_level=120)

        def gen():
            return torch.Generator().manual_seed(10)

        def pieces(n):
            return (clip[:, :, i:i + n] for i in range(0, clip.shape[2], n))
        want, after_cut = _composition(pipe, clip, gen(), **kw)
        alone = video_io.upscale_clip(pipe, clip[:, :, 12:22].contiguous(), generator=gen(), **kw)
        assert not torch.equal(alone[0], after_cut)                             # (the generator does carry on from scene to scene)
        for n in (26, 5):                                                       # one piece, and pieces of 5 frames
            chunks = video_io.upscale_scenes_chunks(pipe, pieces(n), scene=SCENE, overlap=2, generator=gen(), **kw)
            assert chunks.scenes == [] and chunks.seams == []
            got = list(chunks)
            assert chunks.scenes == [(0, 8), (8, 12), (12, 20), (20, 26)] and chunks.seams == [8, 20] and chunks.frames == 26
            assert all(1 <= c.shape[0] <= 3 for c in got) and sum(c.shape[0] for c in got) == 26
            got = torch.cat(got)
            assert torch.equal(got, want), f"pieces of {n}: frames {sorted(set((got != want).nonzero()[:, 0].tolist()))} differ"
            assert torch.equal(got[12], after_cut)                              # the detected cut stays hard
        assert not torch.equal(want[8], video_io.upscale_clip(pipe, clip[:, :, 8:12].contiguous(), generator=gen(), **kw)[0])
        for fmt in ("420", "444p10"):
            coefs = video_io.yuv_coefficients("bt601", True, depth=video_io.out_format(fmt).depth)
            chunks = video_io.upscale_scenes_chunks(pipe, pieces(5), scene=SCENE, overlap=2, generator=gen(), coefs=coefs, fmt=fmt, **kw)
            got = list(chunks)
            assert chunks.seams == [8, 20] and all(1 <= c[0].shape[0] <= 3 for c in got)
            planes = [torch.cat(p) for p in zip(*got)]
            assert all(torch.equal(p, q) for p, q in zip(planes, video_io.postprocess_planes(want, coefs, fmt))), fmt
        # overlap = 0 is the call without the keyword
        plain = list(video_io.upscale_scenes_chunks(pipe, pieces(5), scene=SCENE, generator=gen(), **kw))
        zero = video_io.upscale_scenes_chunks(pipe, pieces(5), scene=SCENE, overlap=0, generator=gen(), **kw)
        got = list(zero)
        assert zero.seams == [] and len(got) == len(plain) and all(torch.equal(g, p) for g, p in zip(got, plain))
        assert not torch.equal(torch.cat(plain)[8:10], want[8:10])                  # ... and the cross-fade does change the result
        for bad in (5, -1, 1.0, "2"):
            with pytest.raises(ValueError):
                video_io.upscale_scenes_chunks(pipe, pieces(5), scene=SCENE, overlap=bad, generator=gen(), **kw)
        assert video_io.upscale_scenes_chunks(pipe, pieces(5), scene=SCENE, overlap=4, generator=gen(), **kw).seams == []


def _y4m_of(rgb, fps="24"):
    from uav import video_io
    out = io.BytesIO()
    with video_io.Y4MWriter(out, rgb.shape[2], rgb.shape[1], fps, True) as writer:
        writer.write(*yuv_ref.encode(rgb, "bt601", True))
    return out.getvalue()


def _common(base):
    return ["--use_video_vae", "-s", "1", "--pretrained", base, "--device", "cpu"]


def _check_program(tmp_path, monkeypatch):
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, video_io
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    open("in.y4m", "wb").write(_y4m_of(scene_ref.scenes_u8(LENGTHS, H, W)))
    scenes = ["--scenes", "auto", "--scene-min", "4", "--scene-max", "8"]
    out = io.StringIO()
    with _StandIns(), contextlib.redirect_stdout(out):
        clip = video_io.preprocess_planes(video_io.read_y4m("in.y4m"), "cpu", "auto")
        assert scene_ref.assert_fixture(clip[0].numpy(), LENGTHS) == [12]
        assert cli.main(["-i", "in.y4m", "-o", "fade"] + scenes + ["--scene-overlap", "2"] + _common(base)) == 0
        assert cli.main(["-i", "in.y4m", "-o", "hard"] + scenes + _common(base)) == 0
        assert cli.main(["-i", "in.y4m", "-o", "zero"] + scenes + ["--scene-overlap", "0"] + _common(base)) == 0
        assert cli.main(["-i", "in.y4m", "-o", "rgb", "--dump-rgb", "rgb.npy"] + scenes + ["--scene-overlap", "2"] + _common(base)) == 0
        assert cli.main(["-i", "in.y4m", "-o", "nomax", "--scenes", "auto", "--scene-min", "4", "--scene-overlap", "2"] + _common(base)) == 0
        pipe, _ = cli.load_pipeline(base, use_video_vae=True, device="cpu")
        want, _ = _composition(pipe, clip, torch.Generator().manual_seed(10), prompt="best quality, extremely detailed",
                               negative_prompt="blur, worst quality", steps=1, guidance_scale=6, noise_level=120)
        coefs = video_io.yuv_coefficients("bt601", True)
        planes = [p.numpy() for p in video_io.postprocess_planes(want, coefs)]
        rgb = video_io.postprocess_frames(want).numpy()
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
    assert len(lines) == 5, lines
    head = "[1/1] in: 26 frames 16x24 -> 64x96, 1 tile(s), "
    assert lines[0].startswith(head + "4 scene(s) (cuts at 8, 12, 20), 2-frame overlap at 2 split(s), "), lines[0]
    assert lines[3].startswith(head + "4 scene(s) (cuts at 8, 12, 20), 2-frame overlap at 2 split(s), "), lines[3]
    for line in (lines[1], lines[2]):                                           # no option, or 0: the line of a program without the option
        assert line.startswith(head + "4 scene(s) (cuts at 8, 12, 20), ") and "overlap" not in line, line
    assert lines[4].startswith(head + "2 scene(s) (cuts at 12), ") and "overlap" not in lines[4], lines[4]      # accepted, no effect
    name = "video/in_n120_g6_s1.y4m"                                            # file names do not change
    got = video_io.read_y4m(os.path.join("fade", name))
    assert got.y.shape == (26, 64, 96)
    assert all(np.array_equal(g, w) for g, w in zip((got.y, got.cb, got.cr), planes)), "the file != the composition"
    hard = open(os.path.join("hard", name), "rb").read()
    assert hard == open(os.path.join("zero", name), "rb").read() and hard != open(os.path.join("fade", name), "rb").read()
    assert np.array_equal(np.load("rgb.npy"), rgb)                              # --dump-rgb gets the blended frames
    assert open(os.path.join("rgb", name), "rb").read() == open(os.path.join("fade", name), "rb").read()


def _check_errors(tmp_path, monkeypatch):
    from uav import cli
    monkeypatch.chdir(tmp_path)
    np.save("clip.npy", scene_ref.scenes_u8([2], 16, 24))
    common = ["-i", "clip.npy", "--pretrained", "no_checkpoints_here", "--device", "cpu", "--scene-min", "8"]
    for value in ("x", "-1", "9", "1.5"):
        for scenes in (["--scenes", "auto"], ["--scenes", "off"], []):
            err = io.StringIO()
            with contextlib.redirect_stderr(err):
                assert cli.main(common + scenes + [f"--scene-overlap={value}"]) == 2, value
            lines = err.getvalue().strip().splitlines()
            assert len(lines) == 1 and lines[0].startswith("upscale.py: error: --scene-overlap: "), (value, err.getvalue())
    for extra in (["--scene-overlap", "8"], ["--scene-overlap", "3", "--scene-max", "0"], ["--scene-overlap", "0"]):
        err = io.StringIO()                                                     # good values get as far as the checkpoints
        with contextlib.redirect_stderr(err):
            assert cli.main(common + ["--scenes", "auto"] + extra) == 2
        assert "--pretrained" in err.getvalue() and "--scene-overlap" not in err.getvalue()


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    with pytest.MonkeyPatch.context() as mp:
        from pathlib import Path
        {"_check_composition": _check_composition, "_check_program": _check_program, "_check_errors": _check_errors}[sys.argv[1]](
            Path(sys.argv[2]), mp)
