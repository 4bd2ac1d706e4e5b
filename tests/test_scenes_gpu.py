"""`--scenes auto` on the device: the scene-statistics kernel (csrc/scene_stats.hip, `uav_clip_scene_stats`) against the numpy
reference of tests/scene_ref.py — exactly, through the raw C ABI, inside 4 KiB guards, outputs pre-filled with garbage, with
16-byte and scalar loads —, its argument checks, and the upscaling program (uav/cli.py) end to end in one child process."""
import ctypes
import functools
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
import scene_ref  # noqa: E402
import yuv_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096
# a single frame (sad[0] = 0 only); widths of 1, odd and 4k+1; h*w % 4 != 0 (scalar loads, a short last thread); more than one
# block of 1024 pixels per frame
SHAPES = [(1, 1, 1), (2, 1, 1), (3, 2, 3), (2, 7, 9), (4, 16, 16), (3, 33, 65), (5, 64, 96), (2, 130, 258)]


class _Guarded:
    """`nbytes` of device memory, every byte 0xA5, with GUARD bytes in front and behind (and `shift` bytes of misalignment)."""

    def __init__(self, nbytes, dev, shift=0, fill=None):
        self.buf = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.lo, self.n = GUARD + shift, nbytes
        if fill is not None:
            self.buf[self.lo:self.lo + nbytes] = torch.from_numpy(np.ascontiguousarray(fill).reshape(-1).view(np.uint8)).to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def body(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.lo + self.n:] == 0xA5).all())


def _coefs():
    from uav import video_io
    return video_io.yuv_coefficients("bt601", True)


def _run(clip, dev, shift=0):
    """`clip` (3,T,h,w) fp32 numpy through the raw entry point -> (hist, sad) numpy; outputs start as garbage, guards checked."""
    from uav import _lib
    lib = _lib.load()
    _, t, h, w = clip.shape
    src = _Guarded(clip.size * 4, dev, shift, fill=clip)
    hist, sad = _Guarded(t * 64 * 4, dev), _Guarded(t * 8, dev)
    fwd = (ctypes.c_int32 * 10)(*_coefs().forward)
    assert lib.uav_clip_scene_stats(src.ptr, t, h, w, hist.ptr, sad.ptr, fwd, None) == 0
    torch.cuda.synchronize()
    assert src.intact() and hist.intact() and sad.intact()
    assert np.array_equal(src.body().view(np.float32), clip.reshape(-1))
    return hist.body().view(np.int32).reshape(t, 64), sad.body().view(np.int64)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """A seeded clip of the shape in [-1.3, 1.3] (the clamp matters) and its reference, computed once."""
    t, h, w = shape
    clip = (torch.rand(3, t, h, w, generator=torch.Generator().manual_seed(7 * t + 3 * h + w)) * 2.6 - 1.3).numpy()
    clip.reshape(-1)[:4] = [-1.0, 1.0, -1.3, 1.3][:clip.size]
    return clip, scene_ref.stats(clip)


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "one_float_in"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_reference_exactly(dev, shape, shift):
    """`shift` = 4: the clip's base is one float past a 16-byte boundary, so every load is scalar whatever h*w is."""
    clip, (want_hist, want_sad) = _case(shape)
    hist, sad = _run(clip, dev, shift)
    assert np.array_equal(hist, want_hist) and np.array_equal(sad, want_sad)
    assert sad[0] == 0 and hist.sum(axis=1).tolist() == [shape[1] * shape[2]] * shape[0]


def test_identical_frames_black_to_white_and_the_op(dev):
    from uav import ops
    t, h, w = 3, 20, 52
    still = np.repeat(_case((1, 33, 65))[0], 4, axis=1)                          # four identical frames
    hist, sad = _run(still, dev)
    assert sad.tolist() == [0, 0, 0, 0] and all(np.array_equal(hist[0], row) for row in hist)
    assert np.array_equal(hist, scene_ref.stats(still)[0])
    steps = np.full((3, t, h, w), -1.0, dtype=np.float32)
    steps[:, 1] = 1.0                                                           # black -> white -> black
    for shift in (0, 4):
        hist, sad = _run(steps, dev, shift)
        assert sad.tolist() == [0, 255 * h * w, 255 * h * w]
        assert [np.flatnonzero(row).tolist() for row in hist] == [[0], [63], [0]] and hist.max(axis=1).tolist() == [h * w] * 3
    # the tensor-level op: same integers, on the clip's device
    clip, (want_hist, want_sad) = _case((5, 64, 96))
    got_hist, got_sad = ops.clip_scene_stats(torch.from_numpy(clip).to(dev), _coefs())
    assert got_hist.device == got_sad.device == torch.from_numpy(clip).to(dev).device
    assert got_hist.dtype == torch.int32 and got_sad.dtype == torch.int64
    assert np.array_equal(got_hist.cpu().numpy(), want_hist) and np.array_equal(got_sad.cpu().numpy(), want_sad)
    view = torch.zeros(3 * 5 * 64 * 96 + 1, device=dev)                         # ... and a view one float into its storage
    view[1:] = torch.from_numpy(clip).reshape(-1).to(dev)
    got_hist, got_sad = ops.clip_scene_stats(view[1:].view(3, 5, 64, 96), _coefs())
    assert np.array_equal(got_hist.cpu().numpy(), want_hist) and np.array_equal(got_sad.cpu().numpy(), want_sad)


def test_bad_arguments_are_refused_with_nothing_written(dev):
    from uav import _lib, ops
    lib = _lib.load()
    fn = lib.uav_clip_scene_stats
    fwd = (ctypes.c_int32 * 10)(*_coefs().forward)
    clip = torch.zeros(3, 2, 4, 4, device=dev)
    hist = torch.full((2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    sad = torch.full((2,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    good = [clip.data_ptr(), 2, 4, 4, hist.data_ptr(), sad.data_ptr(), fwd, None]
    for hole in (0, 4, 5, 6):                                                   # null pointers
        args = list(good)
        args[hole] = None
        assert fn(*args) == -1                                                  # UAV_EINVAL
    for t, h, w in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (2, 0, 4), (2, 4, 0), (2, -4, 4), (2, 4, -4)):
        assert fn(clip.data_ptr(), t, h, w, hist.data_ptr(), sad.data_ptr(), fwd, None) == -3          # UAV_ESHAPE
    assert fn(clip.data_ptr(), 2, 2 ** 31 - 1, 2 ** 31 - 1, hist.data_ptr(), sad.data_ptr(), fwd, None) == -3      # 2^31 blocks and more
    torch.cuda.synchronize()
    assert bool((hist == 0x5A5A5A5A).all()) and bool((sad == 0x5A5A5A5A5A5A).all()) and bool((clip == 0).all())
    k = _coefs()
    assert tuple(ops.clip_scene_stats(clip, k)[0].shape) == (2, 64)
    for bad in (clip.cpu(), clip.half(), torch.zeros(3, 2, 4, 6, device=dev)[..., :4], torch.zeros(4, 2, 4, 4, device=dev),
                torch.zeros(3, 4, 4, device=dev), clip.double()):
        with pytest.raises(_lib.UavError):
            ops.clip_scene_stats(bad, k)


# ---- the program, in one child process -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _program(tmp):
    return subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), tmp], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def program(dev, tmp_path_factory):
    r = _program(str(tmp_path_factory.mktemp("scenes")))
    assert r.returncode == 0, f"exit status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-1500:])
    return r.stdout


def test_program_end_to_end_on_the_device(program):
    """uav/cli.py `-s 2 --scenes auto` on tiny seeded checkpoints and the two-scene 17-frame 64x96 fixture: exit status 0, 17
    frames written, 2 scenes reported, and the planes of the file equal `upscale_scenes_chunks` driven directly."""
    assert "two scenes: ok" in program


def test_program_writes_the_same_bytes_without_a_cut(program):
    """A 12-frame clip without a cut: `--scenes auto` writes the file `--scenes off` writes, byte for byte."""
    assert "same bytes: ok" in program


def _child(tmp):
    import contextlib
    import io
    import time
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, video_io
    start = time.time()
    dev = torch.device("cuda:0")
    base = _write_pretrained(tmp)
    os.chdir(tmp)

    def write_input(name, lengths):
        rgb = scene_ref.scenes_u8(lengths, 64, 96)
        video_io.write_y4m(name, *yuv_ref.encode(rgb, "bt601", True), "24", True)
        source = video_io.read_y4m(name)
        clip = video_io.preprocess_planes(source, dev, "auto")
        assert scene_ref.assert_fixture(clip[0].cpu().numpy(), lengths) == np.cumsum(lengths)[:-1].tolist()
        return clip

    clip = write_input("two.y4m", [9, 8])
    calm = write_input("calm.y4m", [12])
    common = ["-s", "2", "--pretrained", base, "--device", "cuda:0"]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main(["-i", "two.y4m", "-o", "auto", "--scenes", "auto"] + common) == 0
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("[")]
    assert len(lines) == 1 and "two: 17 frames 64x96 -> 256x384, 1 tile(s), 2 scene(s) (cuts at 9), " in lines[0], lines
    got = video_io.read_y4m("auto/video/two_n120_g6_s2.y4m")
    assert got.y.shape == (17, 256, 384) and got.y.std() > 5
    pipe, _ = cli.load_pipeline(base, device=dev)
    coefs = video_io.yuv_coefficients("bt601", True)
    chunks = video_io.upscale_scenes_chunks(pipe, iter([clip]), prompt="best quality, extremely detailed", negative_prompt="blur, worst quality",
                                            steps=2, guidance_scale=6, noise_level=120, generator=torch.Generator(device=dev).manual_seed(10),
                                            coefs=coefs)
    want = [torch.cat(p).cpu().numpy() for p in zip(*chunks)]
    assert chunks.scenes == [(0, 9), (9, 17)]
    assert all(np.array_equal(g, w) for g, w in zip((got.y, got.cb, got.cr), want)), "the file != upscale_scenes_chunks driven directly"
    print(f"two scenes: ok at {time.time() - start:.1f} s", flush=True)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["-i", "calm.y4m", "-o", "auto", "--scenes", "auto"] + common) == 0
        assert cli.main(["-i", "calm.y4m", "-o", "off"] + common) == 0
    off = open("off/video/calm_n120_g6_s2.y4m", "rb").read()
    assert off.count(b"FRAME\n") >= 12 and off == open("auto/video/calm_n120_g6_s2.y4m", "rb").read(), "auto != off without a cut"
    del calm
    print(f"same bytes: ok at {time.time() - start:.1f} s", flush=True)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    _child(sys.argv[1])
