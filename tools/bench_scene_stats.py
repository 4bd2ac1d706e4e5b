"""Same-process timing of the scene-statistics kernel of `--scenes auto` (csrc/scene_stats.hip, `uav_clip_scene_stats`) against the
8-bit 4:2:0 encoder `uav_clip_to_yuv420_u8` on a (T,3,h,w) tensor of the same size, in the style of tools/bench_out_format.py.
  clips (3,8,320,320), (3,48,480,856), (3,48,720,1280) fp32; both kernels read 12 B per pixel and frame; the encoder also writes
  1.5 B, the statistics (64*4 + 8) B per frame and block of 1024 pixels at most, as atomics.
Per kernel and shape: ROUNDS rounds, interleaved between the two kernels, of 20 warm launches between two HIP events; the launches
rotate over NBUF input tensors (at 720p 4 x 531 MB, more than the 256 MiB Infinity Cache; the 320x320 clip, 9.8 MB, stays in cache
as it does in the program).  The statistics' launch includes the launcher's two memsets.  One JSON line per kernel and shape: median
and min of the rounds' mean launch time in us, GB/s of the bytes read at the median, and that figure as a fraction of the yardstick's.
With --end-to-end: the tests' tiny seeded checkpoints and a 24-frame 64x96 clip without a cut are written to a temporary directory
and the program runs on it with `--scenes off` and with `--scenes auto`, each twice, each in a fresh process: wall time, the program's
own seconds per video, and whether the two files are the same bytes.
usage: python tools/bench_scene_stats.py [--out FILE] [--end-to-end [--steps N]]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "upscale-a-video_amd"))
from uav import ops, video_io  # noqa: E402

LAUNCHES, ROUNDS, NBUF = 20, 7, 4
SHAPES = [(8, 320, 320), (48, 480, 856), (48, 720, 1280)]


def time_round(fn, bufs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(LAUNCHES):
        fn(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES                                 # us per launch


def calm_clip(path, frames=24, h=64, w=96):
    """A clip without a cut as a full-range 4:2:0 .y4m file: a sine pattern drifting one pixel per frame."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rgb = np.stack([np.stack([m + 28 * np.sin(2 * np.pi * (x + i) / 13 + 0.9 * c) * np.cos(2 * np.pi * y / 19.5)
                              for c, m in enumerate((70, 90, 60))]) for i in range(frames)])
    frames_u8 = torch.from_numpy(np.clip(np.rint(rgb), 0, 255).astype(np.uint8)).to("cuda:0")     # (T,3,h,w)
    clip = video_io.preprocess_frames(frames_u8)
    planes = video_io.postprocess_planes(clip[0].permute(1, 0, 2, 3), video_io.yuv_coefficients("bt601", True))
    video_io.write_y4m(path, *planes, 24, True)


def end_to_end(steps):
    """Wall time of `upscale.py` on the clip per mode, a fresh process each (checkpoint loading and warm-up included in both)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    from test_cli_dropin_cpu import _write_pretrained
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        pretrained = _write_pretrained(tmp)
        clip = os.path.join(tmp, "calm.y4m")
        calm_clip(clip)
        for mode in ("off", "auto", "off", "auto"):
            start = time.time()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "upscale.py"), "-i", clip, "-o", os.path.join(tmp, mode), "-s", str(steps),
                                "--pretrained", pretrained, "--scenes", mode], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("[1/1]")][0]
            assert ("1 scene(s)" in line) == (mode == "auto"), line
            out.setdefault(mode, []).append(dict(wall_s=round(time.time() - start, 2), video_s=float(line.split(" s -> ")[0].split()[-1])))
        name = f"calm_n120_g6_s{steps}.y4m"
        same = open(os.path.join(tmp, "off", "video", name), "rb").read() == open(os.path.join(tmp, "auto", "video", name), "rb").read()
    return out, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--end-to-end", dest="end_to_end", action="store_true")
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    coefs = video_io.yuv_coefficients("bt601", True)
    lines = []
    for t, h, w in SHAPES:
        clips = [torch.rand(3, t, h, w, generator=g, device=dev) * 2.0 - 1.0 for _ in range(NBUF)]
        cases = [("uav_clip_to_yuv420_u8", lambda c: ops.clip_to_yuv420_u8(c.view(t, 3, h, w), coefs)),       # the same bytes as frames
                 ("uav_clip_scene_stats", lambda c: ops.clip_scene_stats(c, coefs))]
        for _, fn in cases:                                                     # warm-up: code objects, allocator
            for c in clips:
                fn(c)
        torch.cuda.synchronize()
        times = [[] for _ in cases]
        for _ in range(ROUNDS):
            for k, (_, fn) in enumerate(cases):
                times[k].append(time_round(fn, clips))
        yard = None
        for (kernel, _), ts in zip(cases, times):
            med, best, nbytes = statistics.median(ts), min(ts), 12.0 * t * h * w
            gbps = nbytes / med / 1e3
            yard = yard or gbps
            lines.append(json.dumps(dict(kernel=kernel, shape=[3, t, h, w], launches_per_round=LAUNCHES, rounds=ROUNDS, input_buffers=NBUF,
                                         us_median=round(med, 2), us_min=round(best, 2), read_bytes_per_pixel=12.0,
                                         read_gbps_at_median=round(gbps, 1), gbps_vs_yardstick=round(gbps / yard, 3),
                                         spread_min_vs_median=round(1 - best / med, 3), device=torch.cuda.get_device_name(0))))
        del clips, cases
        torch.cuda.empty_cache()
    if args.end_to_end:
        runs, same = end_to_end(args.steps)
        for mode, r in runs.items():
            lines.append(json.dumps(dict(end_to_end="upscale.py", clip="24 frames 64x96, no cut", steps=args.steps, scenes=mode, runs=r,
                                         same_bytes_as_off=same)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
