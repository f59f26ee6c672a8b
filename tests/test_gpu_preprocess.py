"""Video preprocessing on the GPU: vaura_video_preprocess (csrc/preproc.hip) through VideoPreprocessor against its CPU restatement
``reference_u8`` (bit for bit: integer arithmetic, then a table of fp32 values) and against torch's own uint8 and float64 paths
(criteria A and B of tests/test_preprocess_host.py, computed live on the same seeded input).  Every figure is printed; with
VAURA_PREPROCESS_PARITY_OUT=<file> they are also written there (profiles/preprocess_parity.txt is such a file)."""
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_preprocess_host import GEOMETRIES, VGG_TRANSFORMS, as_segments, check_a_b, noise_video, torch_paths  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.preprocess import VideoPreprocessor  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def parity_lines():
    lines = []
    yield lines
    path = os.environ.get("VAURA_PREPROCESS_PARITY_OUT")
    if lines and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("# video preprocessing on the device against torch's CPU paths (tests/test_gpu_preprocess.py; seeded uniform noise)\n"
                     "# A: max |kernel_u8 - torch_u8| (levels); C: share of pixels where they differ; B: max distance to torch's float64 path\n")
            fh.write("\n".join(lines) + "\n")


def levels(pre, out):
    """The uint8 levels behind a device output: the inverse of the fp32 table, checked to be exact."""
    lut = pre.lut.to(out.device)
    x = out.movedim(2, -1)                                             # (..., 3)
    idx = torch.stack([torch.bucketize(x[..., c].contiguous(), lut[c].contiguous()) for c in range(3)], dim=-1).clamp_(0, 255)
    back = torch.stack([lut[c][idx[..., c]] for c in range(3)], dim=-1)
    assert torch.equal(back, x), "an output value is not an entry of the level table"
    return idx.movedim(-1, 2).to(torch.uint8).cpu()


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_kernel_equals_reference_u8_and_meets_a_b_against_torch(H, W, channels_last, parity_lines):
    T = 2
    video = noise_video(T, H, W, seed=H * 7 + W)
    pre = VideoPreprocessor(segment_size_vframes=T, channels_last=channels_last)
    src = video.permute(0, 2, 3, 1).contiguous() if channels_last else video
    got = pre(src.to(DEV))
    assert got.dtype == torch.float32 and got.device.type == "cuda" and tuple(got.shape) == (1, 1, 3, T, 224, 224)
    ref_u8 = pre.reference_u8(src)
    assert torch.equal(got.cpu(), pre.scale_normalize(ref_u8))          # no tolerance
    # A and B against torch directly, on the levels the kernel produced
    ours = levels(pre, got)
    t_u8, exact = torch_paths(video)
    what = f"{H}x{W} {'NHWC' if channels_last else 'NCHW'}"
    share = check_a_b(ours, as_segments(t_u8, T), as_segments(exact, T), what)
    assert torch.equal(ours, as_segments(t_u8, T))                      # A, tightened (see test_preprocess_host.py)
    d = (ours.double() - as_segments(exact, T)).abs().max()
    dt = (t_u8.double() - exact).abs().max()
    parity_lines.append(f"{what:>16}: A max diff {int((ours.int() - as_segments(t_u8, T).int()).abs().max())} level, C differing pixels "
                        f"{100 * share:.4f} %, B max |kernel - exact| {float(d):.4f} <= max |torch_u8 - exact| {float(dt):.4f}")


def test_host_input_segments_and_two_calls():
    """Host (pinned or not) uint8 input, T not a multiple of 16 (the run of segments is centred), B = 1; two calls give the same bits."""
    video = noise_video(70, 144, 176, seed=5)
    pre = VideoPreprocessor()
    a = pre(video)                                                       # host tensor, (T, C, H, W)
    b = pre(video[None].pin_memory())
    assert tuple(a.shape) == (1, 4, 3, 16, 224, 224) and torch.equal(a, b)
    assert torch.equal(a.cpu(), pre.scale_normalize(pre.reference_u8(video)))
    half = VideoPreprocessor(step_size_seg=0.5)
    c = half(video.to(DEV))
    assert tuple(c.shape) == (1, 7, 3, 16, 224, 224)
    assert torch.equal(c.cpu(), half.scale_normalize(half.reference_u8(video)))
    assert torch.equal(c[:, 1, :, :8], c[:, 0, :, 8:])                   # overlapping segments share frames


def test_mixed_geometry_list_other_normalisation():
    clips = [noise_video(16, 144, 176, 1), noise_video(16, 239, 427, 2), noise_video(16, 239, 427, 3), noise_video(16, 640, 360, 4)]
    pre = VideoPreprocessor(mean=(0.4, 0.5, 0.45), std=(0.2, 0.5, 0.25))
    out = pre([c.to(DEV) if i % 2 else c for i, c in enumerate(clips)])  # device and host clips mixed
    assert tuple(out.shape) == (4, 1, 3, 16, 224, 224)
    assert torch.equal(out.cpu(), pre.scale_normalize(pre.reference_u8(clips)))
    for i, c in enumerate(clips):
        assert torch.equal(out[i:i + 1], pre(c))


def test_unaligned_source_view():
    """A view whose first byte is not 4-byte aligned (odd width, odd offset): the aligned-word loads must select the right bytes."""
    big = noise_video(17, 239, 427, seed=9).to(DEV)
    view = big[1:]                                                       # offset 3 * 239 * 427 bytes: odd
    assert view.data_ptr() % 4 != 0
    pre = VideoPreprocessor()
    assert torch.equal(pre(view).cpu(), pre.scale_normalize(pre.reference_u8(view.cpu())))


def test_frames_from_video_through_the_extractor(parity_lines):
    """VAURAModel.frames_from_video -> MotionFormer.forward (synthetic extractor weights, seed 0, as tests/test_gpu_avclip.py): the
    features equal those of reference_u8's output through the same extractor; the distance to the features of torch's own uint8
    path is printed and recorded (not gated: it measures level differences, not this kernel)."""
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
    video = noise_video(32, 360, 640, seed=11)[None]                     # (1, 32, 3, 360, 640) -> 2 segments
    frames = m.frames_from_video(video, video_transforms=VGG_TRANSFORMS)
    assert frames is not None and tuple(frames.shape) == (1, 2, 3, 16, 224, 224)
    assert m.frames_from_video(video, video_transforms=VGG_TRANSFORMS).data_ptr() != 0 and len(m._video_preprocessors) == 1
    pre = VideoPreprocessor.from_transforms_config(VGG_TRANSFORMS)
    feats, _ = m.visual_feature_extractor(frames)
    feats = feats.clone()
    ref_frames = pre.scale_normalize(pre.reference_u8(video)).to(DEV)
    feats_ref, _ = m.visual_feature_extractor(ref_frames)
    assert torch.equal(feats, feats_ref.clone())
    t_u8, _ = torch_paths(video[0])
    t_frames = pre.scale_normalize(t_u8.view(1, 2, 16, 3, 224, 224).permute(0, 1, 3, 2, 4, 5)).to(DEV)
    feats_t, _ = m.visual_feature_extractor(t_frames)
    rel = float(((feats - feats_t) ** 2).mean().sqrt() / (feats_t ** 2).mean().sqrt())
    print(f"features from the kernel's frames vs from torch's uint8 path: relative RMS distance {rel:.3e}")
    parity_lines.append(f"extractor features (360x640, 2 segments), kernel frames vs torch uint8-path frames: relative RMS {rel:.3e}")


def _call(video, out, tabs, **over):
    a = dict(channels_last=0, n_clips=1, T=16, C=3, H=64, W=64, resize=32, crop_h=24, crop_w=24, F=16, S=1, seg_start=0, seg_stride=16,
             h_taps=5, h_prec=15, v_taps=5, v_prec=15, x0=0, span=64, tile_rows=8, tile_src_rows=32)
    a.update(over)
    h_rel, h_w, v_start, v_w, lut = tabs
    return L.lib().vaura_video_preprocess(
        L.ptr(video), a["channels_last"], a["n_clips"], a["T"], a["C"], a["H"], a["W"], a["resize"], a["crop_h"], a["crop_w"], a["F"], a["S"],
        a["seg_start"], a["seg_stride"], L.ptr(h_rel), L.ptr(h_w), a["h_taps"], a["h_prec"], L.ptr(v_start), L.ptr(v_w), a["v_taps"],
        a["v_prec"], a["x0"], a["span"], a["tile_rows"], a["tile_src_rows"], L.ptr(lut), L.ptr(out), L.current_stream(torch.device(DEV)))


def test_status_codes_of_refused_shapes():
    video = torch.zeros(16, 3, 64, 64, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1, 3, 16, 24, 24), 7.0, device=DEV)
    tabs = (torch.zeros(24, dtype=torch.int32, device=DEV), torch.zeros(24 * 33, dtype=torch.int16, device=DEV),
            torch.zeros(24, dtype=torch.int32, device=DEV), torch.zeros(24 * 33, dtype=torch.int16, device=DEV),
            torch.zeros(768, device=DEV))
    SHAPE, ARG = -2, -1
    assert _call(video, out, tabs, C=4) == SHAPE
    assert _call(video, out, tabs, C=1) == SHAPE
    assert _call(video, out, tabs, crop_h=33) == SHAPE                   # the resized image is 32 x 32
    assert _call(video, out, tabs, crop_w=36) == SHAPE
    assert _call(video, out, tabs, H=64, W=128, crop_w=68) == SHAPE      # resized 32 x 64
    assert _call(video, out, tabs, crop_w=22) == SHAPE                   # not a multiple of 4
    assert _call(video, out, tabs, T=15) == SHAPE                        # T < F
    assert _call(video, out, tabs, S=2) == SHAPE                         # second segment outside the clip
    assert _call(video, out, tabs, h_taps=33) == SHAPE
    assert _call(video, out, tabs, v_taps=33) == SHAPE
    assert _call(video, out, tabs, span=65) == ARG
    assert _call(None, out, tabs) == ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # nothing was launched
    assert _call(video, out, tabs) == 0                                  # the same call, accepted
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())                                      # zero taps, zero table
    with pytest.raises(L.VauraHipError, match="shorter than one segment"):
        VideoPreprocessor()(torch.zeros(15, 3, 64, 64, dtype=torch.uint8, device=DEV))
