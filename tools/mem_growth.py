"""Peak of device memory of one upscaling run at T = 12 and T = 36 (64x96 input, 2 steps, tiny seeded checkpoints):
   python tools/mem_growth.py ROOT hand|stream OUT.json
ROOT: a built checkout of this repository, whose modules are the ones imported (`git worktree add ../parent 4e1f3e2`, build it, and
pass that path to measure the last commit whose program held the whole clip).  `hand`: upscale_clip -> postprocess_planes ->
write_y4m (every commit since the Y4M front end); `stream`: upscale_clip_chunks -> Y4MWriter.  One warm-up run at T = 12 first;
prints and writes one JSON record (peaks, growth, growth in fp32 copies of the 24 added output frames, sha256 of the streams)."""
import io, json, os, sys, tempfile
root, mode, out_path = os.path.abspath(sys.argv[1]), sys.argv[2], sys.argv[3]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "oracle"), root, os.path.join(root, "upscale-a-video_amd")]
import torch
torch.set_num_threads(16)
import synth
from test_cli_dropin_cpu import _write_pretrained
from uav import cli, video_io
assert os.path.abspath(video_io.__file__).startswith(root), video_io.__file__
dev = torch.device("cuda:0")
tmp = tempfile.mkdtemp()
base = _write_pretrained(tmp)
pipe, _ = cli.load_pipeline(base, device=dev)
opts = dict(prompt="best quality, extremely detailed", negative_prompt="blur, worst quality", steps=2, guidance_scale=6, noise_level=120)
coefs = video_io.yuv_coefficients("bt601", True)

def run(t):
    clip = synth.synth_clip(1, t, 64, 96, seed=60).to(dev)
    gen = torch.Generator(device=dev).manual_seed(10)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    sink = io.BytesIO()
    if mode == "hand":
        output = video_io.upscale_clip(pipe, clip, generator=gen, **opts)
        y, cb, cr = video_io.postprocess_planes(output, coefs)
        path = os.path.join(tmp, "o.y4m")
        video_io.write_y4m(path, y, cb, cr, 24, True)
        data = open(path, "rb").read()
    else:
        with video_io.Y4MWriter(sink, 384, 256, 24, True) as out:
            for planes in video_io.upscale_clip_chunks(pipe, clip, coefs=coefs, generator=gen, **opts):
                out.write(*planes)
        data = sink.getvalue()
    torch.cuda.synchronize()
    import hashlib
    return torch.cuda.max_memory_allocated(), hashlib.sha256(data).hexdigest()

run(12)
(p12, h12), (p36, h36) = run(12), run(36)
B = 24 * 3 * 256 * 384 * 4
res = dict(root=root, mode=mode, peak_t12=p12, peak_t36=p36, growth=p36 - p12, growth_in_B=(p36 - p12) / B, B=B, sha_t12=h12, sha_t36=h36)
print(json.dumps(res))
json.dump(res, open(out_path, "w"))
