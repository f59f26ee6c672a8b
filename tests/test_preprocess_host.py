"""Video preprocessing, host side (vaura_amd/preprocess.py): the integer restatement ``reference_u8`` against torch's own uint8
path, the tap tables, the segment rule and the configuration reader.  No GPU.

What the expectation is.  torchvision is not installed, so the reference's transform objects cannot run; for tensors
``torchvision.transforms.v2.Resize`` is ``torch.nn.functional.interpolate(mode="bilinear", antialias=True)``, which is computed here,
live, on seeded noise.  Criteria (both sides on the same input):
  A  max |ours_u8 - torch_u8| <= 1 level                       (closeness to the reference's integer path)
  B  max |ours_u8 - exact| <= max |torch_u8 - exact|           (no worse than it; exact = torch's float64 path)
and, because ``reference_u8`` reaches 0 differing pixels on every geometry below, A is tightened to ``torch.equal``.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from vaura_amd import _lib as L
from vaura_amd.preprocess import VideoPreprocessor, crop_offset, resized_size, segment_starts, tap_table

GEOMETRIES = [(360, 640), (144, 176), (640, 360), (239, 427), (480, 854), (1080, 1920), (256, 340), (224, 224)]

# configs/generate_vgg.yaml:53-65, as data
VGG_TRANSFORMS = [
    {"target": "torchvision.transforms.v2.Resize", "params": {"size": 256, "antialias": True}},
    {"target": "torchvision.transforms.v2.CenterCrop", "params": {"size": [224, 224]}},
    {"target": "models.data.transforms.video_transforms.ToFloat32DType"},
    {"target": "torchvision.transforms.v2.Normalize", "params": {"mean": [0.5, 0.5, 0.5], "std": [0.5, 0.5, 0.5]}},
]


def noise_video(T, H, W, seed):
    return torch.randint(0, 256, (T, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def torch_paths(video, resize=256, crop=(224, 224)):
    """torch's uint8 path and its float64 path of Resize(resize, antialias) -> CenterCrop(crop) on (T, 3, H, W): (T, 3, h, w) each."""
    H, W = video.shape[-2:]
    oh, ow = resized_size(H, W, resize)
    top, left = crop_offset(oh, crop[0]), crop_offset(ow, crop[1])
    u8 = Fn.interpolate(video, size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
    ex = Fn.interpolate(video.double(), size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
    cut = lambda t: t[..., top:top + crop[0], left:left + crop[1]]  # noqa: E731
    return cut(u8), cut(ex)


def as_segments(x, F=16):
    """(T, 3, h, w) with T == F -> (1, 1, 3, F, h, w)"""
    return x.view(1, 1, F, *x.shape[1:]).permute(0, 1, 3, 2, 4, 5)


def check_a_b(ours, t_u8, exact, what):
    d = (ours.int() - t_u8.int()).abs()
    share = float((d > 0).float().mean())
    ours_err = float((ours.double() - exact).abs().max())
    torch_err = float((t_u8.double() - exact).abs().max())
    print(f"{what}: max |ours - torch_u8| {int(d.max())}, differing pixels {100 * share:.3f} %, max |ours - exact| {ours_err:.4f}, "
          f"max |torch_u8 - exact| {torch_err:.4f}")
    assert int(d.max()) <= 1, what                               # A
    assert ours_err <= torch_err, what                           # B
    return share


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_reference_u8_against_torch(H, W, channels_last):
    T = 2
    video = noise_video(T, H, W, seed=H * 7 + W)
    pre = VideoPreprocessor(segment_size_vframes=T, channels_last=channels_last)
    ours = pre.reference_u8(video.permute(0, 2, 3, 1).contiguous() if channels_last else video)
    assert ours.dtype == torch.uint8 and tuple(ours.shape) == (1, 1, 3, T, 224, 224)
    t_u8, exact = torch_paths(video)
    share = check_a_b(ours, as_segments(t_u8, T), as_segments(exact, T), f"{H}x{W} channels_last={channels_last}")
    assert share == 0.0 and torch.equal(ours, as_segments(t_u8, T))     # A, tightened: the restatement is torch's integer path
    if (H, W) == (256, 340):                                            # no resize happens: the crop of the input itself
        assert torch.equal(ours, as_segments(video[..., 16:240, 58:282], T))


def test_scale_normalize_is_the_fp32_formula_in_order():
    pre = VideoPreprocessor(mean=(0.4, 0.5, 0.45), std=(0.2, 0.5, 0.25))
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 1, 1, 16, 16).expand(1, 1, 3, 1, 16, 16).contiguous()
    got = pre.scale_normalize(u8)
    for c in range(3):
        want = ((u8[0, 0, c].float() / 255) - torch.tensor(pre.mean[c])) / torch.tensor(pre.std[c])
        assert torch.equal(got[0, 0, c], want)
        assert torch.equal(pre.lut[c], want.reshape(-1))                # the table the kernel reads


@pytest.mark.parametrize("H,W", GEOMETRIES + [(2160, 3840), (100, 3000)])
def test_tap_tables(H, W):
    oh, ow = resized_size(H, W, 256)
    for in_size, out_size, crop in ((W, ow, 224), (H, oh, 224)):
        lo = crop_offset(out_size, crop)
        t = tap_table(in_size, out_size, lo, crop)
        w, wf = t["weights"].astype(np.int64), t["weights_f64"]
        assert w.shape == (crop, t["taps"]) and t["taps"] <= 32
        # float64 taps sum to 1.0; the int16 taps are each rounded on their own (as torch's are), so a row is within taps / 2 of 2^prec
        assert np.allclose(wf.sum(1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(w.sum(1) - (1 << t["prec"])).max() <= t["taps"] / 2
        assert (w >= 0).all() and w.max() < (1 << 15)
        # start + length (the last tap that may be non-zero) and start + taps (what the kernel reads) stay inside the source
        assert (t["start"] >= 0).all() and (t["start"] + t["length"] <= in_size).all() and (t["start"] + t["taps"] <= in_size).all()
        assert (t["length"] >= 1).all() and (t["length"] <= t["taps"]).all()
        assert not w[np.arange(t["taps"])[None, :] >= t["length"][:, None]].any()
        assert (np.diff(t["start"]) >= 0).all()                         # what the kernel's tiling of source rows relies on


def test_tap_bound_and_crop_refusals():
    pre = VideoPreprocessor()
    assert pre.geometry(1080, 1920).h["taps"] == 11 and pre.geometry(1080, 1920).v["taps"] == 11
    with pytest.raises(L.VauraHipError, match="taps"):
        pre.geometry(4352, 4352)                                        # scale 17: 37 taps
    with pytest.raises(L.VauraHipError, match="larger than the resized image"):
        VideoPreprocessor(resize=128).geometry(360, 640)
    with pytest.raises(L.VauraHipError, match="3 are needed"):
        pre.reference_u8(torch.zeros(16, 4, 64, 64, dtype=torch.uint8))


@pytest.mark.parametrize("T,F,step,want_first", [(64, 16, 1.0, [0, 16, 32, 48]), (70, 16, 1.0, [3, 19, 35, 51]),
                                                 (64, 16, 0.5, [0, 8, 16, 24, 32, 40, 48]), (16, 16, 1.0, [0])])
def test_segment_rule(T, F, step, want_first):
    """video_transforms.py:146-156 (count, stride) and :205-236 (the run of segments is centred: 70 frames start at frame 3)."""
    S, first, stride = segment_starts(T, F, step)
    assert [first + s * stride for s in range(S)] == want_first
    assert S == (T - F) // stride + 1 and first + (S - 1) * stride + F <= T
    # through reference_u8: frame t is the constant image t, no resize (256 x 256 source), so every output pixel names its source frame
    video = torch.arange(T, dtype=torch.uint8).view(T, 1, 1, 1).expand(T, 3, 256, 256).contiguous()
    out = VideoPreprocessor(segment_size_vframes=F, step_size_seg=step).reference_u8(video)
    assert tuple(out.shape) == (1, S, 3, F, 224, 224)
    want = torch.tensor(want_first).view(S, 1) + torch.arange(F).view(1, F)
    assert torch.equal(out[0, :, 0, :, 0, 0].long(), want) and torch.equal(out[0, :, 2, :, 223, 223].long(), want)


def test_segment_rule_against_the_reference_class(golden):
    """tests/golden/preproc_segments.npz: the frame indices the reference's own GenerateMultipleSegments picked (make_golden_preproc.py)."""
    g = golden("preproc_segments.npz")
    n = 0
    while f"case{n}_frames" in g.files:
        T, F, step = g[f"case{n}_T_F_step"]
        S, first, stride = segment_starts(int(T), int(F), float(step))
        ours = np.array([[first + s * stride + f for f in range(int(F))] for s in range(S)], np.int32)
        assert np.array_equal(ours, g[f"case{n}_frames"]), (T, F, step)
        n += 1
    assert n >= 4


def test_segment_refusals():
    with pytest.raises(L.VauraHipError, match="shorter than one segment"):
        segment_starts(15, 16, 1.0)
    with pytest.raises(L.VauraHipError, match="shorter than one segment"):
        VideoPreprocessor().reference_u8(torch.zeros(15, 3, 64, 64, dtype=torch.uint8))
    with pytest.raises(L.VauraHipError, match="at most 4"):
        segment_starts(64, 16, 1.0, n_segments=5)
    assert segment_starts(64, 16, 1.0, n_segments=2) == (2, 16, 16)     # fewer segments than fit: still centred


def test_from_transforms_config():
    pre = VideoPreprocessor.from_transforms_config(VGG_TRANSFORMS, step_size_seg=0.5)
    assert (pre.resize, pre.crop, pre.mean, pre.std, pre.step_size_seg) == (256, (224, 224), (0.5,) * 3, (0.5,) * 3, 0.5)
    other = [dict(VGG_TRANSFORMS[0]), VGG_TRANSFORMS[1], {"target": "torchvision.transforms.v2.ToDtype", "params": {"dtype": "torch.float32", "scale": True}},
             VGG_TRANSFORMS[3]]
    assert VideoPreprocessor.from_transforms_config(other).resize == 256

    def bad(i, entry, match):
        cfg = list(VGG_TRANSFORMS)
        cfg[i] = entry
        with pytest.raises(L.VauraHipError, match=match):
            VideoPreprocessor.from_transforms_config(cfg)
    bad(0, {"target": "torchvision.transforms.v2.Resize", "params": {"size": 256, "antialias": False}}, "antialias")
    bad(0, {"target": "torchvision.transforms.v2.Resize", "params": {"size": 256}}, "antialias")
    bad(0, {"target": "torchvision.transforms.v2.Resize", "params": {"size": 256, "antialias": True, "interpolation": "bicubic"}}, "bicubic")
    bad(1, {"target": "torchvision.transforms.v2.RandomCrop", "params": {"size": [224, 224]}}, "RandomCrop")
    bad(2, {"target": "torchvision.transforms.v2.ToDtype", "params": {"dtype": "torch.float32"}}, "scale")
    with pytest.raises(L.VauraHipError, match="in that order"):
        VideoPreprocessor.from_transforms_config(VGG_TRANSFORMS[:3])


def test_float_input_is_refused():
    pre = VideoPreprocessor()
    for call in (pre.reference_u8, pre):
        with pytest.raises(L.VauraHipError, match="transformed already"):
            call(torch.zeros(16, 3, 64, 64, dtype=torch.float32))


def test_mixed_geometry_list_on_the_host():
    a, b = noise_video(16, 144, 176, 1), noise_video(16, 239, 427, 2)
    pre = VideoPreprocessor()
    out = pre.reference_u8([a, b])
    assert tuple(out.shape) == (2, 1, 3, 16, 224, 224)
    assert torch.equal(out[0:1], pre.reference_u8(a)) and torch.equal(out[1:2], pre.reference_u8(b))
