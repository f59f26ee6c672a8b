"""Video preprocessing from 4:2:0 decoder surfaces on the GPU: vaura_video_preprocess_yuv420 (csrc/preproc.hip) through
VideoPreprocessor(input_format="nv12" / "i420").  Everything is equality, no tolerance: the kernel applies the host's integer colour
formula and then the tables of the RGB kernel, so its output is bit for bit (a) the RGB kernel's on the frames yuv420_to_rgb_u8
converts on the host and (b) scale_normalize(reference_u8(yuv)), the CPU restatement."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_preprocess_host import VGG_TRANSFORMS  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.preprocess import VideoPreprocessor, yuv420_to_rgb_u8, yuv_coefficients  # noqa: E402
from yuv_cases import CONTENTS, GEOMETRIES, noise_planes, pack  # noqa: E402

DEV = "cuda:0"
T = 2
LAYOUTS = ("nv12", "i420")


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_kernel_equals_rgb_kernel_and_reference_u8(H, W, content):
    y, u, v = CONTENTS[content](T, H, W, seed=H * 7 + W)
    rgb = yuv420_to_rgb_u8(y, u, v)
    pre_rgb = VideoPreprocessor(segment_size_vframes=T)
    via_rgb = pre_rgb(rgb.to(DEV))                                       # the parent's kernel on the converted frames
    for layout in LAYOUTS:
        pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
        surf = pack(y, u, v, layout)
        got = pre(surf.to(DEV))
        assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (1, 1, 3, T, 224, 224)
        bad = int((got != via_rgb).sum())
        print(f"{H}x{W} {content} {layout}: {bad} of {got.numel()} values differ from the RGB kernel's")
        assert torch.equal(got, via_rgb), (layout, bad)
        assert torch.equal(got.cpu(), pre.scale_normalize(pre.reference_u8(surf))), layout


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", [(144, 176), (480, 854)])
def test_padded_surface_on_the_device_unaligned_base(H, W, layout):
    """A decoder surface with P = W + 24, the chroma plane from row H + 8 and random bytes everywhere outside the planes, in a view
    that starts at an odd address: equal to the tight call, and to itself with other padding bytes."""
    y, u, v = noise_planes(T, H, W, seed=H + W)
    pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
    tight = pre(pack(y, u, v, layout).to(DEV))
    outs = []
    for fill in (1, 2):
        surf = pack(y, u, v, layout, pad=True, fill_seed=fill)
        buf = torch.randint(0, 256, (surf.numel() + 5,), dtype=torch.uint8, generator=torch.Generator().manual_seed(fill)).to(DEV)
        view = buf[1:1 + surf.numel()].view(surf.shape)
        view.copy_(surf)
        assert view.data_ptr() % 2 == 1 and view.shape[-1] == W + 24
        outs.append(pre(view, size=(H, W), chroma_row=H + 8))
        assert torch.equal(outs[-1], tight), fill
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(pre(surf, size=(H, W), chroma_row=H + 8), tight)  # the padded surface from the host, copied as it is


@pytest.mark.parametrize("color_matrix,color_range", [("bt709", "limited"), ("bt601", "full"), ("bt709", "full")])
def test_matrix_and_range_variants(color_matrix, color_range):
    H, W = 288, 352
    y, u, v = noise_planes(T, H, W, seed=17)
    pre_rgb = VideoPreprocessor(segment_size_vframes=T)
    want = pre_rgb.scale_normalize(pre_rgb.reference_u8(yuv420_to_rgb_u8(y, u, v, color_matrix, color_range)))
    base = pre_rgb.scale_normalize(pre_rgb.reference_u8(yuv420_to_rgb_u8(y, u, v)))
    assert not torch.equal(want, base)
    for layout in LAYOUTS:
        pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout, color_matrix=color_matrix, color_range=color_range)
        assert torch.equal(pre(pack(y, u, v, layout).to(DEV)).cpu(), want), layout


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mixed_input_list(layout):
    """Two geometries, host (pinned and not pinned) and device clips in one list: the output keeps the list's order and every clip's
    bits are those of its own call."""
    shapes = [(144, 176), (144, 176), (288, 352), (288, 352), (144, 176)]
    clips = [pack(*noise_planes(T, H, W, seed=30 + i), layout) for i, (H, W) in enumerate(shapes)]
    placed = [clips[0], clips[1].to(DEV), clips[2].pin_memory(), clips[3], clips[4].to(DEV)]
    pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
    out = pre(placed)
    assert tuple(out.shape) == (5, 1, 3, T, 224, 224)
    assert torch.equal(out.cpu(), pre.scale_normalize(pre.reference_u8(clips)))
    for i, c in enumerate(clips):
        assert torch.equal(out[i:i + 1], pre(c.to(DEV))), i
    assert torch.equal(pre(torch.stack(clips[:2]).to(DEV)), out[:2])     # (B, T, R, P)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_views_with_a_frame_stride(layout):
    """Every other frame of a clip (frames at twice the surface size: read in place) and a batch without its first frames (no
    single frame stride: copied once) give the bits of the contiguous clips."""
    H, W = 144, 176
    big = torch.stack([pack(*noise_planes(2 * T + 1, H, W, seed=50 + i), layout) for i in range(2)]).to(DEV)   # (2, 5, R, P)
    pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
    for view in (big[:, ::2][:, :T], big[:, 1:1 + T], big[0, ::2][:T]):
        assert not view.is_contiguous()
        assert torch.equal(pre(view), pre(view.contiguous()))
        assert torch.equal(pre(view).cpu(), pre.scale_normalize(pre.reference_u8(view.cpu())))


def test_frames_from_video_through_the_extractor():
    """VAURAModel.frames_from_video(nv12, input_format="nv12") -> MotionFormer.forward, as tests/test_gpu_preprocess.py does for RGB:
    frames and features equal those of the converted RGB clip; one cached preprocessor per configuration."""
    from vaura_amd.model import VAURAModel
    cfg = synth.tiny_sampler(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAURAModel(
            feature_extractor_config={"target": "vaura_amd.feature_extractor.MotionFormer", "params": {"extract_features": True}},
            audio_encoder_config={"target": "vaura_amd.codec.DacModelWrapper", "params": {"model_sr": 44100, "synthetic": True}},
            sampler_config={"target": "vaura_amd.sampler.Transformer", "params": cfg.yaml_params()},
            visual_bridge_config={"target": "torch.nn.Identity"},
            pattern_provider_config={"target": "vaura_amd.patterns.DelayedPatternProvider", "params": {"n_q": 9}},
            flatten_vis_feats=True, freeze_feature_extractor=True)
    m.visual_feature_extractor.load_state_dict(synth.avclip_state_dict(seed=0), strict=True)
    m = m.to(DEV)
    H, W = 360, 640
    y, u, v = CONTENTS["legal"](32, H, W, seed=11)
    nv12 = pack(y, u, v, "nv12")[None]                                   # (1, 32, 540, 640) -> 2 segments
    frames = m.frames_from_video(nv12, video_transforms=VGG_TRANSFORMS, input_format="nv12")
    assert tuple(frames.shape) == (1, 2, 3, 16, 224, 224) and len(m._video_preprocessors) == 1
    frames_rgb = m.frames_from_video(yuv420_to_rgb_u8(y, u, v)[None], video_transforms=VGG_TRANSFORMS)
    assert torch.equal(frames, frames_rgb) and len(m._video_preprocessors) == 2
    feats = m.visual_feature_extractor(frames)[0].clone()
    feats_rgb = m.visual_feature_extractor(frames_rgb)[0].clone()
    assert torch.equal(feats, feats_rgb)
    # the same configuration again: the cached preprocessor; another matrix, layout or a padded surface: its own entry / the same bits
    m.frames_from_video(nv12, video_transforms=VGG_TRANSFORMS, input_format="nv12")
    assert len(m._video_preprocessors) == 2
    other = m.frames_from_video(nv12, video_transforms=VGG_TRANSFORMS, input_format="nv12", color_matrix="bt709")
    assert len(m._video_preprocessors) == 3 and not torch.equal(other, frames)
    padded = pack(y, u, v, "i420", pad=True, fill_seed=3)
    via_i420 = m.frames_from_video(padded, video_transforms=VGG_TRANSFORMS, input_format="i420", size=(H, W), chroma_row=H + 8)
    assert len(m._video_preprocessors) == 4 and torch.equal(via_i420, frames)


def _call(video, out, tabs, **over):
    a = dict(video_bytes=0 if video is None else video.numel(), layout=0, pitch=64, chroma_offset=64 * 64, frame_stride=96 * 64, n_clips=1, T=16, H=64, W=64,
             resize=32, crop_h=24, crop_w=24, F=16, S=1, seg_start=0, seg_stride=16, h_taps=5, h_prec=15, v_taps=5, v_prec=15, x0=0,
             span=64, tile_rows=8, tile_src_rows=32)
    a.update(over)
    h_rel, h_w, v_start, v_w, lut = tabs
    return L.lib().vaura_video_preprocess_yuv420(
        L.ptr(video) if video is not None else None, a["video_bytes"], a["layout"], a["pitch"], a["chroma_offset"], a["frame_stride"],
        a["n_clips"], a["T"], a["H"], a["W"], *a.get("color", yuv_coefficients()), a["resize"], a["crop_h"], a["crop_w"], a["F"], a["S"],
        a["seg_start"], a["seg_stride"], L.ptr(h_rel), L.ptr(h_w), a["h_taps"], a["h_prec"], L.ptr(v_start), L.ptr(v_w), a["v_taps"],
        a["v_prec"], a["x0"], a["span"], a["tile_rows"], a["tile_src_rows"], L.ptr(lut), L.ptr(out), L.current_stream(torch.device(DEV)))


def test_status_codes_of_refused_surfaces():
    video = torch.zeros(16, 96, 64, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1, 3, 16, 24, 24), float("nan"), device=DEV)
    tabs = (torch.zeros(24, dtype=torch.int32, device=DEV), torch.zeros(24 * 33, dtype=torch.int16, device=DEV),
            torch.zeros(24, dtype=torch.int32, device=DEV), torch.zeros(24 * 33, dtype=torch.int16, device=DEV),
            torch.zeros(768, device=DEV))
    SHAPE, ARG = -2, -1
    assert _call(video, out, tabs, H=63) == SHAPE                        # odd H
    assert _call(video, out, tabs, W=63, span=63) == SHAPE               # odd W
    assert _call(video, out, tabs, pitch=63) == ARG                      # pitch < W
    assert _call(video, out, tabs, video_bytes=video.numel() - 1) == ARG  # the last plane byte lies behind the buffer
    assert _call(video, out, tabs, layout=1, pitch=65, chroma_offset=64 * 65, frame_stride=96 * 65, T=16, video_bytes=16 * 96 * 65) == ARG
    assert _call(video, out, tabs, chroma_offset=64 * 64 - 1) == ARG     # the chroma plane starts inside the luma plane
    assert _call(video, out, tabs, frame_stride=96 * 64 - 1) == ARG      # frames overlap
    assert _call(video, out, tabs, layout=2) == ARG
    assert _call(video, out, tabs, color=(16, 1 << 21, 0, 0, 0, 0)) == ARG
    assert _call(video, out, tabs, crop_w=22) == SHAPE                   # and what vaura_video_preprocess refuses
    assert _call(video, out, tabs, T=15) == SHAPE
    assert _call(video, out, tabs, h_taps=33) == SHAPE
    assert _call(video, out, tabs, span=65) == ARG
    assert _call(None, out, tabs) == ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                  # nothing was launched
    for layout in (0, 1):
        out.fill_(float("nan"))
        assert _call(video, out, tabs, layout=layout) == 0               # the same call, accepted (the buffer ends with the last byte)
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())                                  # zero taps, zero table
