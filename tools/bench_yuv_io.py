"""Same-process timing of the frame I/O kernels around the pipeline call (csrc/yuv_io.hip K13): the Y'CbCr pair of the Y4M
front end against the RGB pair it stands beside.
  out side, frames (8,3,1280,1280):  uav_clip_to_yuv420_u8 (12 B read + 1.5 B written per pixel)  vs  uav_clip_to_frames_u8 (12 + 3)
  in side,  clip   (8,3,320,320):    uav_yuv420_to_clip_f32 (1.5 B read + 12 B written)           vs  uav_frames_to_clip_f32 from uint8 (3 + 12)
Per kernel: ROUNDS rounds, interleaved between the kernels, of 20 warm launches between two HIP events; the launches rotate over
NBUF input tensors (4 x 157 MB on the out side, more than the 256 MiB Infinity Cache) so that every launch reads from HBM.  One JSON
line per kernel: median and min of the rounds' mean launch time in us, and GB/s of the algorithmic bytes at the median.
usage: python tools/bench_yuv_io.py [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "upscale-a-video_amd"))
from uav import ops, video_io  # noqa: E402

LAUNCHES, ROUNDS, NBUF = 20, 7, 4


def time_round(fn, bufs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(LAUNCHES):
        fn(bufs[i % len(bufs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES                                 # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    coefs = video_io.yuv_coefficients("bt709", True)
    g = torch.Generator().manual_seed(0)
    t, h, w = 8, 1280, 1280
    frames = [(torch.randn(t, 3, h, w, generator=g) * 0.8).to(dev) for _ in range(NBUF)]
    th, hh, ww = 8, 320, 320
    planes = [tuple(torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in ((th, hh, ww), (th, hh // 2, ww // 2), (th, hh // 2, ww // 2)))
              for _ in range(NBUF)]
    rgb = [torch.randint(0, 256, (th, 3, hh, ww), generator=g, dtype=torch.uint8).to(dev) for _ in range(NBUF)]
    cases = [
        ("uav_clip_to_yuv420_u8", (t, 3, h, w), lambda f: ops.clip_to_yuv420_u8(f, coefs), frames, 13.5 * t * h * w),
        ("uav_clip_to_frames_u8", (t, 3, h, w), ops.clip_to_frames_u8, frames, 15.0 * t * h * w),
        ("uav_yuv420_to_clip_f32", (th, 3, hh, ww), lambda p: ops.yuv420_to_clip_f32(*p, coefs), planes, 13.5 * th * hh * ww),
        ("uav_frames_to_clip_f32", (th, 3, hh, ww), ops.frames_to_clip_f32, rgb, 15.0 * th * hh * ww),
    ]
    for _, _, fn, bufs, _ in cases:                                             # warm-up: code objects, allocator
        for b in bufs:
            fn(b)
    torch.cuda.synchronize()
    times = {name: [] for name, *_ in cases}
    for _ in range(ROUNDS):
        for name, _, fn, bufs, _ in cases:
            times[name].append(time_round(fn, bufs))
    lines = []
    for name, shape, _, _, nbytes in cases:
        med, best = statistics.median(times[name]), min(times[name])
        lines.append(json.dumps(dict(kernel=name, shape=list(shape), launches_per_round=LAUNCHES, rounds=ROUNDS, input_buffers=NBUF,
                                     us_median=round(med, 2), us_min=round(best, 2), algorithmic_bytes=int(nbytes),
                                     gbps_at_median=round(nbytes / med / 1e3, 1), device=torch.cuda.get_device_name(0))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
