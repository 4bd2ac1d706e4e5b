"""CFG-shared UNet head, extended by the text-free front of the first cross-attention block: `down_blocks[1].resnets[0]` (256 -> 512
at the second level) sees no text, so with `cfg_shared_input` it runs once at B = 1 and its rows (with their GroupNorm statistics
partials) are duplicated in front of the block's first transformer.  Full-width model: the result must not change by a bit, and the
256 -> 512 3x3 conv must be launched exactly once, at half the rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 8


@pytest.fixture(scope="module")
def unet(dev):
    from uav import configs, init_weights
    from models_video.unet_video import UNetVideoModel
    model = UNetVideoModel.from_config(dict(configs.UNET_VIDEO)).half().to(dev).eval()
    return init_weights.random_init_(model, seed=1234)


def inputs(dev, h, w):
    gd = torch.Generator(device=dev).manual_seed(5)
    lat = torch.randn(1, 4, T, h, w, generator=gd, device=dev).half().repeat(2, 1, 1, 1, 1)
    low = torch.randn(1, 3, T, h, w, generator=gd, device=dev).half().repeat(2, 1, 1, 1, 1)
    ehs = torch.randn(2, 77, 1024, generator=gd, device=dev).half()           # the entries differ in the text only
    return lat, low, ehs, torch.tensor([120])


@pytest.mark.parametrize("h,w", [(32, 32), (48, 32)])
def test_shared_front_is_bit_identical(unet, dev, h, w):
    lat, low, ehs, cl = inputs(dev, h, w)
    with torch.no_grad():
        a = unet(lat, 925, low, encoder_hidden_states=ehs, class_labels=cl, cfg_shared_input=False).sample
        b = unet(lat, 925, low, encoder_hidden_states=ehs, class_labels=cl, cfg_shared_input=True).sample
    assert bool(torch.isfinite(a).all()) and not torch.equal(a[0], a[1])
    assert torch.equal(a, b)


def test_front_conv_is_launched_once_at_half_the_rows(unet, dev):
    from uav import ops
    h = w = 32
    lat, low, ehs, cl = inputs(dev, h, w)
    full_rows = 2 * T * (h // 2) * (w // 2)
    key = "conv_gemm cin=256 n=512 k=1x3x3 M=%d"

    def launches(shared):
        ops.PROFILER.detail = True
        ops.PROFILER.start(only={"conv_gemm"})
        try:
            with torch.no_grad():
                unet(lat, 925, low, encoder_hidden_states=ehs, class_labels=cl, cfg_shared_input=shared)
            torch.cuda.synchronize()
        finally:
            ops.PROFILER.stop()
            ops.PROFILER.detail = False
        s = ops.PROFILER.summary()
        return tuple(s.get(key % m, {}).get("launches", 0) for m in (full_rows // 2, full_rows))

    assert launches(False) == (0, 1)          # the duplicated reference order: one launch at the full rows
    assert launches(True) == (1, 0)
