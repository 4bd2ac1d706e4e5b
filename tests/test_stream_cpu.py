"""The 4x frames streamed to the Y4M writer in 3-frame decode chunks, on the CPU stand-ins: `VideoUpscalePipeline.denoise` +
`decode_chunks`, `tiling.upscale_tiled_chunks`, `video_io.upscale_clip_chunks` and `Y4MWriter` each give the bits of the
whole-clip function they split (`pipeline(...)`, `upscale_tiled`, `upscale_clip`, `write_y4m`), and the program
(uav/cli.py) writes byte for byte the file that the whole-clip path — `upscale_clip` -> `postprocess_planes` -> `write_y4m`
called by hand — writes, while it never holds more than one chunk.  (Those two functions are themselves compositions of
the chunked pieces now, so the by-hand file of checks 5 and 7 shares code with the program; what is independent are checks
1 - 3 against `pipeline(...)` and `upscale_tiled`, the recorded runs of tests/test_upscale_cli_cpu.py, and the restated
whole-clip path of tests/test_stream_gpu.py.)  Checkpoints: the tiny seeded ones of
tests/test_cli_dropin_cpu.py.  Everything that loads them runs in a child interpreter, as there."""
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

KW = dict(num_inference_steps=2, guidance_scale=6, noise_level=120, negative_prompt="n")


def _in_child(check, tmp_path):
    r = subprocess.run([sys.executable, "-X", "faulthandler", os.path.abspath(__file__), check, str(tmp_path)],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, f"{check} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    print(r.stdout[-2000:])


# ---- 4. the writer (no checkpoints: in this process) ------------------------------------------------------------------
def _planes(t, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (t, h, w), dtype=np.uint8), rng.integers(0, 256, (t, (h + 1) // 2, (w + 1) // 2), dtype=np.uint8),
            rng.integers(0, 256, (t, (h + 1) // 2, (w + 1) // 2), dtype=np.uint8))


class _Pipe:
    """A binary sink that can only be written to, like a pipe: no seek, no tell."""

    def __init__(self):
        self.data = bytearray()

    def write(self, b):
        self.data += b
        return len(b)

    def flush(self):
        pass


@pytest.mark.parametrize("as_tensor", [False, True])
def test_writer_chunks_give_the_bytes_of_one_write_y4m_call(tmp_path, as_tensor):
    from uav import video_io
    y, cb, cr = _planes(7, 6, 10, seed=1)
    conv = torch.from_numpy if as_tensor else (lambda p: p)
    whole = tmp_path / "whole.y4m"
    video_io.write_y4m(whole, conv(y), conv(cb), conv(cr), "30000/1001", False)
    expected = whole.read_bytes()
    assert os.listdir(tmp_path) == ["whole.y4m"]                              # no `.part` left behind
    header = video_io.y4m_header(10, 6, "30000/1001", False)
    frame = len(b"FRAME\n") + 6 * 10 + 2 * 3 * 5
    assert len(expected) == len(header) + 7 * frame

    path = tmp_path / "chunks.y4m"
    with video_io.Y4MWriter(path, 10, 6, "30000/1001", False) as out:
        assert not path.exists()                                              # the name appears on a clean exit only
        for k, (a, b) in enumerate(((0, 3), (3, 6), (6, 7))):
            out.write(conv(y[a:b]), conv(cb[a:b]), conv(cr[a:b]))
            if k == 0:
                assert os.path.getsize(str(path) + ".part") == len(header) + 3 * frame         # header + 3 frames after the first write
        assert out.frames == 7
    assert path.read_bytes() == expected and not os.path.exists(str(path) + ".part")

    pipe = _Pipe()                                                            # a stream without seek / tell
    with video_io.Y4MWriter(pipe, 10, 6, "30000/1001", False) as out:
        for a, b in ((0, 3), (3, 6), (6, 7)):
            out.write(conv(y[a:b]), conv(cb[a:b]), conv(cr[a:b]))
    assert bytes(pipe.data) == expected
    mem = io.BytesIO()
    with video_io.Y4MWriter(mem, 10, 6, "30000/1001", False) as out:
        out.write(conv(y), conv(cb), conv(cr))
    assert mem.getvalue() == expected and not mem.closed                      # the caller's stream stays the caller's


def test_writer_refuses_wrong_planes_and_leaves_no_file_on_failure(tmp_path):
    from uav import video_io
    y, cb, cr = _planes(2, 6, 10, seed=2)
    with video_io.Y4MWriter(io.BytesIO(), 10, 6, 24, True) as out:
        for bad in ((y[:, :4], cb, cr), (y, cb[:, :2], cr), (y, cb, cr[:1]), (y[0], cb[0], cr[0]),
                    (y.astype(np.int16), cb, cr), (y, cb.astype(np.float32), cr.astype(np.float32)),
                    (torch.from_numpy(y).float(), torch.from_numpy(cb), torch.from_numpy(cr))):
            with pytest.raises(ValueError):
                out.write(*bad)
        assert out.frames == 0
    path = tmp_path / "broken.y4m"
    with pytest.raises(RuntimeError, match="half-way"):
        with video_io.Y4MWriter(path, 10, 6, 24, True) as out:
            out.write(y, cb, cr)
            raise RuntimeError("half-way")
    assert os.listdir(tmp_path) == []                                         # neither the file nor its `.part`


def test_read_y4m_accepts_an_open_stream(tmp_path):
    from uav import video_io
    y, cb, cr = _planes(2, 6, 10, seed=3)
    path = tmp_path / "in.y4m"
    video_io.write_y4m(path, y, cb, cr, 25, True)
    a, b = video_io.read_y4m(path), video_io.read_y4m(io.BytesIO(path.read_bytes()))
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])) and a[3:] == b[3:]
    with pytest.raises(ValueError, match="not a YUV4MPEG2 file"):
        video_io.read_y4m(io.BytesIO(b"RIFF"))


# ---- 2 (second half). a process group of size 2 -----------------------------------------------------------------------
def _dist_worker(rank, world, port, q):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "upscale-a-video_amd"))
    torch.set_num_threads(2)
    import torch.distributed as dist
    from models_video.pipeline_upscale_a_video import Denoised, VideoUpscalePipeline
    from uav import dist as D
    from uav import tiling
    D.init("gloo")
    got = []
    try:
        next(tiling.upscale_tiled_chunks(object(), "p", torch.zeros(1, 3, 2, 68, 160), None, torch.Generator(), tile_size=64))
    except ValueError as e:
        got.append("tiled: " + str(e))
    pipe = VideoUpscalePipeline()
    pipe.shard_windows = True
    try:
        next(pipe.decode_chunks(Denoised(torch.zeros(1, 4, 4, 8, 8), torch.zeros(1, 3, 4, 8, 8))))
    except ValueError as e:
        got.append("decode: " + str(e))
    dist.barrier()
    q.put((rank, got))


def test_chunk_generators_refuse_a_process_group():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30500 + os.getpid() % 1000
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    for rank, got in res:
        assert len(got) == 2 and got[0].startswith("tiled: ") and got[1].startswith("decode: "), (rank, got)


# ---- children ------------------------------------------------------------------------------------------------------------
def test_decode_chunks_of_denoise_equal_the_pipeline_call(tmp_path):
    """1: T = 2, 3, 7 (chunks 3+3+1) and 11 (two windows), with and without propagation steps: same bits, starts 0, 3, 6, ...,
    and the generator is left in the same state."""
    _in_child("_check_pipeline", tmp_path)


def test_tiled_chunks_and_clip_chunks_equal_the_whole_clip_functions(tmp_path):
    """2, 3: `upscale_tiled_chunks` assembled == `upscale_tiled` (68x160, tile 64, T = 2 and 5); `upscale_clip_chunks`
    concatenated == `upscale_clip` and its planes == `postprocess_planes` of that, untiled and tiled."""
    _in_child("_check_tiled_and_clip", tmp_path)


def test_program_writes_the_bytes_of_the_whole_clip_path(tmp_path):
    """5, 6: the two recorded jobs of tests/test_upscale_cli_cpu.py and a 7-frame untiled job: file and --dump-rgb array equal
    the by-hand whole-clip path; PNG names run across the chunks; decode and write alternate, one chunk at a time."""
    _in_child("_check_program", tmp_path)


def test_program_through_real_pipes(tmp_path):
    """7: bytes in through `-i -`, bytes out through `--y4m-out -`, in a child process of its own."""
    _in_child("_check_pipes", tmp_path)


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


def _gen(seed=10):
    return torch.Generator(device="cpu").manual_seed(seed)


def _check_pipeline(tmp_path, monkeypatch):
    import golden_cases as GC
    import synth
    from models_video.propagation_module import Propagation
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli
    base = _write_pretrained(str(tmp_path))
    with _StandIns():
        pipe, _ = cli.load_pipeline(base, device="cpu")
        pipe.propagator = Propagation(4, learnable=False)
        for t in (2, 3, 7, 11):
            clip = synth.synth_clip(1, t, 16, 24, seed=40 + t)
            flows = list(GC.prop_inputs(t, 16, 24, seed=300 + t)[1:])                  # forward, backward: (1,2,T-1,h,w)
            for prop in ([], [1]):
                kw = dict(KW, image=clip, flows_bi=flows if prop else None, propagation_steps=prop)
                g1, g2 = _gen(), _gen()
                whole, lat = pipe("p", generator=g1, return_dict=False, **kw)
                den = pipe.denoise("p", generator=g2, **kw)
                chunks = list(pipe.decode_chunks(den))
                assert [s for s, _ in chunks] == list(range(0, t, 3))
                assert [f.shape[2] for _, f in chunks] == [min(3, t - s) for s in range(0, t, 3)]
                assert all(f.dtype == torch.float32 and f.shape[:2] == (1, 3) and float(f.abs().max()) <= 1.0 for _, f in chunks)
                assert torch.equal(torch.cat([f for _, f in chunks], 2), whole) and whole.std() > 0.05
                assert torch.equal(den.latents.float(), lat) and den.image_dec.dtype == torch.float32 and den.w_lr == 1
                assert torch.equal(g1.get_state(), g2.get_state())
                assert torch.equal(pipe("p", generator=_gen(), **kw).images, whole)             # return_dict=True keeps its bits
                print(f"T = {t}, propagation {prop}: {len(chunks)} chunk(s) ok", flush=True)
        without = pipe("p", image=clip, generator=_gen(), **KW).images
        assert not torch.equal(without, whole)                                                   # the propagation step did run


def _assemble(chunks, t, h, w):
    out = torch.full((1, 3, t, 4 * h, 4 * w), float("nan"))
    starts = []
    for start, n, pieces in chunks:
        starts.append((start, n))
        for (y0, y1, x0, x1), crop in pieces:
            assert crop.shape[1] == n and y0 % 4 == 0 and x0 % 4 == 0
            out[0, :, start:start + n, y0:y1, x0:x1] = crop
    assert starts == [(s, min(3, t - s)) for s in range(0, t, 3)]
    return out


def _check_tiled_and_clip(tmp_path, monkeypatch):
    import synth
    from test_cli_dropin_cpu import _write_pretrained
    from uav import cli, tiling, video_io
    base = _write_pretrained(str(tmp_path))
    opts = dict(prompt="p", negative_prompt="n", steps=2, guidance_scale=6, noise_level=120)
    coefs = video_io.yuv_coefficients("bt601", True)
    with _StandIns():
        pipe, _ = cli.load_pipeline(base, device="cpu")
        for t in (2, 5):
            clip = synth.synth_clip(1, t, 68, 160, seed=33)
            g1, g2 = _gen(), _gen()
            whole = tiling.upscale_tiled(pipe, "p", clip, None, g1, tile_size=64, **KW)
            mine = _assemble(tiling.upscale_tiled_chunks(pipe, "p", clip, None, g2, tile_size=64, **KW), t, 68, 160)
            assert torch.equal(mine, whole) and torch.equal(g1.get_state(), g2.get_state())
            print(f"tiled T = {t} ok", flush=True)
        for name, clip, extra in (("untiled", synth.synth_clip(1, 7, 16, 24, seed=7), {}),
                                  ("tiled", clip, dict(perform_tile=True, tile_size=64))):
            whole = video_io.upscale_clip(pipe, clip, generator=_gen(), **opts, **extra)
            frames = list(video_io.upscale_clip_chunks(pipe, clip, generator=_gen(), **opts, **extra))
            assert [len(f) for f in frames] == [min(3, clip.shape[2] - s) for s in range(0, clip.shape[2], 3)]
            assert torch.equal(torch.cat(frames), whole) and whole.dtype == torch.float32
            if name == "tiled":
                assert torch.equal(whole, mine.squeeze(0).permute(1, 0, 2, 3))
            planes = list(video_io.upscale_clip_chunks(pipe, clip, generator=_gen(), coefs=coefs, **opts, **extra))
            for got, ref in zip((torch.cat(p) for p in zip(*planes)), video_io.postprocess_planes(whole, coefs)):
                assert got.dtype == torch.uint8 and torch.equal(got, ref)
            print(f"upscale_clip_chunks {name} ok", flush=True)
        with pytest.raises(ValueError, match="color_fix"):
            next(video_io.upscale_clip_chunks(pipe, clip, generator=_gen(), color_fix="Sepia", **opts))


def _by_hand(pipe, source, argv_opts, out_path, fps):
    """The whole-clip path of the program before it streamed: upscale_clip -> postprocess_planes -> write_y4m."""
    from uav import video_io
    clip = video_io.preprocess_frames(torch.from_numpy(source).permute(0, 3, 1, 2).contiguous())
    output = video_io.upscale_clip(pipe, clip, generator=_gen(), **argv_opts)
    coefs = video_io.yuv_coefficients(video_io.auto_matrix(output.shape[-2]), True)
    video_io.write_y4m(out_path, *video_io.postprocess_planes(output, coefs), fps, True)
    return video_io.postprocess_frames(output).cpu().numpy()


def _check_program(tmp_path, monkeypatch):
    from test_cli_dropin_cpu import CASES, _clip_u8, _write_pretrained
    from models_video.pipeline_upscale_a_video import VideoUpscalePipeline
    from uav import cli, video_io
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    events = []
    real_decode, real_write = VideoUpscalePipeline.decode_chunks, video_io.Y4MWriter.write

    def decode_chunks(self, denoised):
        for start, frames in real_decode(self, denoised):
            events.append(("decode", start))
            yield start, frames

    def write(self, y, cb, cr):
        events.append(("write", self.frames))
        return real_write(self, y, cb, cr)
    monkeypatch.setattr(VideoUpscalePipeline, "decode_chunks", decode_chunks)
    monkeypatch.setattr(video_io.Y4MWriter, "write", write)

    jobs = {"tile": (_clip_u8(*CASES["tile"][1]), ["--perform_tile", "--tile_size", "64", "-s", "2", "--a_prompt", "p", "--n_prompt", "n"],
                     dict(prompt="p", negative_prompt="n", steps=2, guidance_scale=6, noise_level=120, perform_tile=True, tile_size=64), False,
                     "clip_n120_g6_s2"),
            "video_vae": (_clip_u8(*CASES["video_vae"][1]), ["--use_video_vae", "-s", "1", "-g", "6", "-n", "100", "--save_suffix", "x"],
                          dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=1, guidance_scale=6,
                               noise_level=100), True, "clip_n100_g6_s1_x"),
            "seven": (_clip_u8(7, 16, 24, 36), ["-s", "2"],
                      dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2, guidance_scale=6,
                           noise_level=120), False, "clip_n120_g6_s2")}
    for name, (clip, argv, opts, video_vae, save_name) in jobs.items():
        source = clip.permute(0, 2, 3, 1).contiguous().numpy()
        os.makedirs(name, exist_ok=True)
        np.save(f"{name}/clip.npy", source)
        common = ["-i", f"{name}/clip.npy", "--pretrained", base, "--device", "cpu", "--fps", "8"] + argv
        t = len(source)
        with _StandIns():
            del events[:]
            assert cli.main(common + ["-o", f"{name}/planes"]) == 0                              # chunks -> planes -> writer
            tiles = 2 if name == "tile" else 1
            expect = [e for s in range(0, t, 3) for e in [("decode", s)] * tiles + [("write", s)]]
            assert events == expect, (name, events)                                              # 6: one chunk ahead of the writer at most
            assert cli.main(common + ["-o", f"{name}/frames", "--dump-rgb", f"{name}/rgb.npy"] + (["--save_image"] if have_pil else [])) == 0
            pipe, _ = cli.load_pipeline(base, use_video_vae=video_vae, device="cpu")
            monkeypatch.setattr(VideoUpscalePipeline, "decode_chunks", real_decode)
            rgb = _by_hand(pipe, source, opts, f"{name}/hand.y4m", 8)
            monkeypatch.setattr(VideoUpscalePipeline, "decode_chunks", decode_chunks)
        hand = open(f"{name}/hand.y4m", "rb").read()
        for run in ("planes", "frames"):
            assert os.listdir(f"{name}/{run}/video") == [save_name + ".y4m"]
            assert open(f"{name}/{run}/video/{save_name}.y4m", "rb").read() == hand, f"{name}/{run}: file != whole-clip path"
        assert np.array_equal(np.load(f"{name}/rgb.npy"), rgb) and rgb.shape == (t, 4 * source.shape[1], 4 * source.shape[2], 3)
        if have_pil:
            from PIL import Image
            folder = f"{name}/frames/frame/{save_name}"
            assert sorted(os.listdir(folder)) == [f"{i:04d}.png" for i in range(t)]
            assert all(np.array_equal(np.asarray(Image.open(f"{folder}/{i:04d}.png")), rgb[i]) for i in range(t))
        print(f"{name}: {t} frames, {len(hand)} bytes ok", flush=True)
    if not have_pil:
        print("PIL is not installed: the --save_image names were not checked")


def _program(argv):
    """`python upscale.py ...` on the CPU stand-ins (what a child of the pipe test runs)."""
    from uav import cli
    with _StandIns():
        return cli.main(argv)


def _check_pipes(tmp_path, monkeypatch):
    import yuv_ref
    from test_cli_dropin_cpu import _clip_u8, _write_pretrained
    from uav import video_io
    base = _write_pretrained(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    rgb = _clip_u8(4, 16, 24, 37).permute(0, 2, 3, 1).contiguous().numpy()
    video_io.write_y4m("in.y4m", *yuv_ref.encode(rgb, "bt601", False), "30000/1001", False)
    stream = open("in.y4m", "rb").read()
    common = ["--use_video_vae", "-s", "1", "--pretrained", base, "--device", "cpu"]
    prog = [sys.executable, os.path.abspath(__file__), "_program"]
    r = subprocess.run(prog + ["-i", "in.y4m", "-o", "file_run"] + common, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    expected = open("file_run/video/in_n120_g6_s1.y4m", "rb").read()
    assert r.stdout.decode().startswith("[1/1] in: 4 frames 16x24 -> 64x96, 1 tile(s)")
    r = subprocess.run(prog + ["-i", "-", "--y4m-out", "-", "-o", "never"] + common, input=stream, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert r.stdout == expected, "standard output is not exactly the stream of the file run"
    assert expected.startswith(b"YUV4MPEG2 W96 H64 F30000:1001 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\nFRAME\n")
    assert "[1/1] stdin: 4 frames 16x24 -> 64x96" in r.stderr.decode() and not os.path.exists("never")
    # -i - alone: the video is called `stdin`; --y4m-out FILE alone
    r = subprocess.run(prog + ["-i", "-", "-o", "named"] + common, input=stream, capture_output=True, timeout=900)
    assert r.returncode == 0 and open("named/video/stdin_n120_g6_s1.y4m", "rb").read() == expected
    r = subprocess.run(prog + ["-i", "in.y4m", "--y4m-out", "direct.y4m", "-o", "never"] + common, capture_output=True, timeout=900)
    assert r.returncode == 0 and open("direct.y4m", "rb").read() == expected and not os.path.exists("never")
    assert r.stdout.decode().startswith("[1/1] in:")
    # two inputs with --y4m-out: exit status 2, one line on standard error, nothing on standard output
    os.makedirs("many")
    for n in ("a.y4m", "b.y4m"):
        open(os.path.join("many", n), "wb").write(stream)
    r = subprocess.run(prog + ["-i", "many", "--y4m-out", "-"] + common, capture_output=True, timeout=900)
    assert r.returncode == 2 and r.stdout == b"" and len(r.stderr.decode().strip().splitlines()) == 1 and b"--y4m-out" in r.stderr


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
    torch.set_num_threads(min(16, os.cpu_count() or 1))                         # as tests/conftest.py
    if sys.argv[1] == "_program":
        sys.exit(_program(sys.argv[2:]))
    with pytest.MonkeyPatch.context() as mp:
        from pathlib import Path
        {"_check_pipeline": _check_pipeline, "_check_tiled_and_clip": _check_tiled_and_clip, "_check_program": _check_program,
         "_check_pipes": _check_pipes}[sys.argv[1]](Path(sys.argv[2]), mp)
