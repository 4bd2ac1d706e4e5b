"""The engine's own upscaling program (uav/cli.py, `python upscale.py`) end to end on the CPU stand-ins, against the videos
the reference project's program wrote for the same jobs (tests/golden/cli_dropin_videos.npz, recorded by
tests/test_cli_dropin_cpu.py): same checkpoints directory, clips, options and seed, so the uint8 RGB frames the program
hands to its Y'CbCr stage must match the recording within that file's bound for CPU rounding noise between machines, and
the Y4M file must hold exactly the numpy encoder's planes of those frames.  Each case runs in a child interpreter."""
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


def _in_child(check, tmp_path):
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), check, str(tmp_path)],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, f"{check} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"


def test_tile_job_matches_the_recorded_reference_run(tmp_path):
    """`--perform_tile --tile_size 64 -s 2` on the 2-frame 68x160 clip: two tiles sharing one generator."""
    _in_child("_check_tile", tmp_path)


def test_video_vae_job_matches_the_recorded_reference_run_and_fps_defaults(tmp_path):
    """`--use_video_vae -s 1 -n 100 --save_suffix x` on the 3-frame 16x24 clip; then the frame rate written without --fps:
    24 for an .npy input, the file's own for a .y4m input."""
    _in_child("_check_video_vae", tmp_path)


def test_program_behaviour_on_bad_and_multiple_inputs(tmp_path):
    """An unsupported file ends the program with a non-zero status and one line on stderr; a directory with two inputs yields
    two outputs in sorted order."""
    _in_child("_check_behaviour", tmp_path)


# ---- bodies (child interpreter) -------------------------------------------------------------------------------------------
class _StandIns:
    def __enter__(self):
        import cpu_ops
        import cpu_ops_io
        cpu_ops.install()
        cpu_ops_io.install()

    def __exit__(self, *exc):
        import cpu_ops
        import cpu_ops_io
        cpu_ops_io.restore()
        cpu_ops.restore()


def _header_and_planes(path):
    from uav import video_io
    with open(path, "rb") as fh:
        header = fh.readline().decode("ascii").split()
    return header, video_io.read_y4m(path)


def _run_case(case, tmp_path, monkeypatch):
    """The recorded job `case` through the new program; returns (dumped RGB frames, output path)."""
    import yuv_ref
    from test_cli_dropin_cpu import CASES, _assert_near_recording, _clip_u8, _recorded, _write_pretrained
    from uav import cli
    _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    argv, clip_args = CASES[case]
    clip = _clip_u8(*clip_args)                                                 # (T,C,H,W) uint8
    os.makedirs("inputs", exist_ok=True)
    np.save("inputs/clip.npy", clip.permute(0, 2, 3, 1).contiguous().numpy())
    argv = [a for a in argv if a != "--no_llava"]
    assert argv[:2] == ["-i", "inputs/clip.mp4"]
    argv = ["-i", "inputs/clip.npy"] + argv[2:] + ["--pretrained", os.path.join(str(tmp_path), "pretrained_models", "upscale_a_video"),
                                                   "--device", "cpu", "--fps", "8", "--dump-rgb", "rgb.npy"]
    with _StandIns():
        assert cli.main(argv) == 0
    rec = _recorded(case)
    rgb = np.load("rgb.npy")
    assert rgb.dtype == np.uint8
    d = np.abs(rgb[:, ::rec["row_step"]].astype(np.int16) - rec["rows"].astype(np.int16))
    print(f"{case}: {(d > 1).mean():.5f} of the bytes off by more than 1 LSB, mean {d.mean():.3f}, max {d.max()}")
    _assert_near_recording(rgb, rec)
    assert rec["path"].endswith(".mp4")
    out = rec["path"][:-4] + ".y4m"
    assert os.listdir("results/video") == [os.path.basename(out)] and os.path.isfile(out)
    header, planes = _header_and_planes(out)
    t, h, w, _ = rgb.shape
    assert header == ["YUV4MPEG2", f"W{w}", f"H{h}", "F8:1", "Ip", "A1:1", "C420jpeg", "XCOLORRANGE=FULL"]
    y, cb, cr = yuv_ref.encode(rgb, "bt709" if h >= 720 else "bt601", True)
    assert np.array_equal(planes.y, y) and np.array_equal(planes.cb, cb) and np.array_equal(planes.cr, cr)
    assert len(planes.y) == t
    return rgb, out


def _check_tile(tmp_path, monkeypatch):
    rgb, _ = _run_case("tile", tmp_path, monkeypatch)
    assert rgb.shape == (2, 272, 640, 3) and rgb.std() > 5


def _check_video_vae(tmp_path, monkeypatch):
    from uav import cli, video_io
    rgb, _ = _run_case("video_vae", tmp_path, monkeypatch)
    assert rgb.shape == (3, 64, 96, 3)
    base = os.path.join(str(tmp_path), "pretrained_models", "upscale_a_video")
    common = ["--use_video_vae", "-s", "1", "--pretrained", base, "--device", "cpu"]
    # without --fps: an .npy input has no rate of its own -> 24 frames/s
    with _StandIns():
        assert cli.main(["-i", "inputs/clip.npy", "-o", "plain"] + common) == 0
    header, _ = _header_and_planes("plain/video/clip_n120_g6_s1.y4m")
    assert "F24:1" in header
    # ... and a .y4m input is written at its own rate (limited range in, limited range out)
    frames = np.load("inputs/clip.npy")
    rng = np.random.default_rng(0)
    y = rng.integers(16, 236, frames.shape[:3], dtype=np.uint8)
    cb = rng.integers(100, 156, (3, 8, 12), dtype=np.uint8)
    video_io.write_y4m("inputs/ntsc.y4m", y, cb, cb[::-1].copy(), "30000/1001", False)
    with _StandIns():
        assert cli.main(["-i", "inputs/ntsc.y4m", "-o", "plain"] + common) == 0
    header, planes = _header_and_planes("plain/video/ntsc_n120_g6_s1.y4m")
    assert "F30000:1001" in header and "C420mpeg2" in header and "XCOLORRANGE=LIMITED" in header
    assert planes.y.shape == (3, 64, 96) and planes.fps.numerator == 30000 and planes.full_range is False


def _check_behaviour(tmp_path, monkeypatch):
    import contextlib
    import io
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import cli
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    common = ["--use_video_vae", "-s", "1", "--pretrained", base, "--device", "cpu", "-o", "out"]
    err = io.StringIO()
    open("clip.mp4", "wb").write(b"\0\0\0 ftypisom")
    with _StandIns(), contextlib.redirect_stderr(err):
        status = cli.main(["-i", "clip.mp4"] + common)
    lines = err.getvalue().strip().splitlines()
    assert status != 0 and len(lines) == 1 and "clip.mp4" in lines[0] and "Traceback" not in err.getvalue(), err.getvalue()
    open("ten.y4m", "wb").write(b"YUV4MPEG2 W4 H4 F24:1 Ip C420p10\nFRAME\n" + bytes(48))
    err = io.StringIO()
    with _StandIns(), contextlib.redirect_stderr(err):
        status = cli.main(["-i", "ten.y4m"] + common)
    assert status != 0 and len(err.getvalue().strip().splitlines()) == 1 and "C420p10" in err.getvalue()
    err = io.StringIO()
    with _StandIns(), contextlib.redirect_stderr(err):
        status = cli.main(["-i", "nowhere.y4m"] + common)
    assert status != 0 and len(err.getvalue().strip().splitlines()) == 1
    # a directory with two inputs: one output each, visited in sorted order
    os.makedirs("many")
    clip = _clip_u8(2, 16, 24, 35).permute(0, 2, 3, 1).contiguous().numpy()
    np.save("many/b_second.npy", clip)
    np.save("many/a_first.npy", clip[:1])
    open("many/notes.txt", "w").write("not a video")
    out = io.StringIO()
    with _StandIns(), contextlib.redirect_stdout(out):
        assert cli.main(["-i", "many", "--save_image"] + common) == 0
    assert sorted(os.listdir("out/frame/b_second_n120_g6_s1")) == ["0000.png", "0001.png"]            # PIL is what read_frames needs too
    assert sorted(os.listdir("out/video")) == ["a_first_n120_g6_s1.y4m", "b_second_n120_g6_s1.y4m"]
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
    assert len(lines) == 2 and lines[0].startswith("[1/2] a_first: 1 frames 16x24 -> 64x96") and lines[1].startswith("[2/2] b_second: 2 frames")


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    with pytest.MonkeyPatch.context() as mp:
        from pathlib import Path
        {"_check_tile": _check_tile, "_check_video_vae": _check_video_vae, "_check_behaviour": _check_behaviour}[sys.argv[1]](Path(sys.argv[2]), mp)
