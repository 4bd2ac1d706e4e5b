"""Measurements of the streamed output path (profiles/stream_*.txt keeps the record).

  python tools/bench_stream.py kernel [--frames 3|8]
      ROUNDS x (window kernel on a decoder-layout chunk (1,3,T,1280,1280) | the copy that makes the same pixels (T,3,H,W)
      contiguous | uav_clip_to_yuv420_u8 on the copy), alternating, after a warm-up; meant to run under
      `rocprofv3 --kernel-trace --stats`, which gives the device-side duration of the three kernels.  The launches rotate over
      NBUF source tensors so that the 66 MB (T = 3) / 157 MB (T = 8) sources do not sit in the 256 MiB Infinity Cache.
  python tools/bench_stream.py e2e
      T = 16, 320x320, 30 steps on the full-width random-weight pipeline of bench.py: the whole-clip path (pipeline(...) ->
      permute + contiguous -> postprocess_planes -> write_y4m) and the chunked path (upscale_clip_chunks -> Y4MWriter), one
      warm-up each, then alternately twice each; host clock around a device synchronise; the files must be identical."""
import argparse
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "upscale-a-video_amd")]
from uav import ops, video_io  # noqa: E402

ROUNDS, NBUF = 240, 4


def kernel(frames):
    dev = torch.device("cuda:0")
    coefs = video_io.yuv_coefficients("bt709", True)
    g = torch.Generator().manual_seed(0)
    h = w = 1280
    chunks = [(torch.randn(1, 3, frames, h, w, generator=g) * 0.8).to(dev) for _ in range(NBUF)]
    y = torch.empty((frames, h, w), dtype=torch.uint8, device=dev)
    cb, cr = (torch.empty((frames, h // 2, w // 2), dtype=torch.uint8, device=dev) for _ in range(2))
    for i in range(ROUNDS + 8):                                                # 8 warm-up rounds
        src = chunks[i % NBUF]
        ops.clip_window_to_yuv420_u8(src[0], y, cb, cr, coefs)
        packed = src[0].permute(1, 0, 2, 3).contiguous()
        ops.clip_to_yuv420_u8(packed, coefs)
    torch.cuda.synchronize()
    print(json.dumps(dict(mode="kernel", frames=frames, rounds=ROUNDS, warmup_rounds=8, source_buffers=NBUF,
                          pixels=frames * h * w, bytes_window_or_sibling=13.5 * frames * h * w, bytes_copy=24.0 * frames * h * w)))


def e2e():
    import bench
    dev = torch.device("cuda:0")
    pipe = bench.build_pipeline(dev, 320, 320, text_encoder="standin")
    g = torch.Generator().manual_seed(3)
    clip = (torch.rand(1, 3, 16, 320, 320, generator=g) * 2 - 1).to(dev)
    coefs = video_io.yuv_coefficients("bt709", True)
    opts = dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=30, guidance_scale=6, noise_level=120)

    def whole():
        sink = io.BytesIO()
        out = pipe(opts["prompt"], image=clip, generator=torch.Generator(device=dev).manual_seed(10), num_inference_steps=30, guidance_scale=6,
                   noise_level=120, negative_prompt=opts["negative_prompt"]).images
        out = out.squeeze(0).permute(1, 0, 2, 3).contiguous()
        video_io.write_y4m(sink, *video_io.postprocess_planes(out, coefs), 24, True)
        return sink.getvalue()

    def chunked():
        sink = io.BytesIO()
        with video_io.Y4MWriter(sink, 1280, 1280, 24, True) as out:
            for planes in video_io.upscale_clip_chunks(pipe, clip, coefs=coefs, generator=torch.Generator(device=dev).manual_seed(10), **opts):
                out.write(*planes)
        return sink.getvalue()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, data
    ref = timed(whole)[1]
    assert timed(chunked)[1] == ref, "the chunked path's stream differs from the whole-clip path's"
    times = {"whole": [], "chunked": []}
    for _ in range(2):
        for name, fn in (("whole", whole), ("chunked", chunked)):
            torch.cuda.reset_peak_memory_stats()
            s, data = timed(fn)
            assert data == ref
            times[name].append(round(s, 4))
            times.setdefault(name + "_peak_bytes", []).append(torch.cuda.max_memory_allocated())
    print(json.dumps(dict(mode="e2e", frames=16, size=[320, 320], steps=30, seconds=times, overlap_mode_of_call=pipe.last_overlap_mode,
                          stream_bytes=len(ref), device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "e2e"])
    ap.add_argument("--frames", type=int, default=3)
    a = ap.parse_args()
    kernel(a.frames) if a.mode == "kernel" else e2e()
