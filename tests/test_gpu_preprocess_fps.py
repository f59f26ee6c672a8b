"""Video at its own frame rate on the GPU: vaura_video_preprocess_frames / vaura_video_preprocess_yuv420_frames (csrc/preproc.hip)
through VideoPreprocessor(src_fps=..) / pts, VideoFrameStream and VAURAModel.open_video_stream.

Everything is torch.equal against the slow route: select the frames on the host with fps_plan's table, then call what exists.  The
table launch runs the arithmetic of the existing launch on the frame the table names, so what can go wrong is bookkeeping — a wrong
frame, a segment cut from the source instead of the converted sequence, a carried frame lost between two pushes.  Every frame of the
seeded noise inputs differs from every other, so a wrong frame cannot compare equal.

Shapes: 144 x 176 and 224 x 224 frames (tests/test_gpu_preprocess_yuv.py's smallest), segments of 16, and the frame counts of
tests/preprocess_fps_reference.py: 2 full segments at 24, 60 and 12.5 fps, 2 segments out of 33 frames at 30 and 30000/1001 fps."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_fps_reference as R  # noqa: E402
from test_preprocess_host import noise_video  # noqa: E402
from vaura_amd import _lib as L  # noqa: E402
from vaura_amd import synth  # noqa: E402
from vaura_amd.preprocess import VideoPreprocessor, fps_plan  # noqa: E402
from yuv_cases import PAD_ROWS, noise_planes, pack  # noqa: E402

DEV = "cuda:0"
H, W = 144, 176
LAYOUTS = ("nchw", "nhwc", "nv12", "i420")
RATE_IDS = [c[0] for c in R.GPU_CASES]


def make_clip(layout, n, h, w, seed):
    """(n, ..) uint8 frames in `layout`, the preprocessor keywords and the call keywords (I420: one padded surface)."""
    if layout in ("nchw", "nhwc"):
        v = noise_video(n, h, w, seed)
        return (v.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else v), dict(channels_last=layout == "nhwc"), {}
    planes = noise_planes(n, h, w, seed)
    if layout == "nv12":
        return pack(*planes, "nv12"), dict(input_format="nv12"), {}
    return pack(*planes, "i420", pad=True, fill_seed=seed), dict(input_format="i420"), dict(size=(h, w), chroma_row=h + PAD_ROWS)


def select(v, table, dim=1):
    return v.index_select(dim, torch.from_numpy(np.asarray(table).astype(np.int64)).to(v.device))


@pytest.fixture()
def calls(monkeypatch):
    """Counts the calls of the four preprocessing entry points on the library handle."""
    lib, n = L.lib(), {}
    for name in ("vaura_video_preprocess", "vaura_video_preprocess_yuv420", "vaura_video_preprocess_frames", "vaura_video_preprocess_yuv420_frames"):
        real = getattr(lib, name)
        n[name] = 0

        def counted(*a, _real=real, _name=name):
            n[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return n


# ---------------------------------------------------------------------------------------------------------------- 1. one pass
@pytest.mark.parametrize("name,n,rate", R.GPU_CASES, ids=RATE_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_pass_equals_the_host_selection(layout, name, n, rate, calls):
    a, pkw, ckw = make_clip(layout, n, H, W, seed=n)
    b = make_clip(layout, n, H, W, seed=n + 100)[0]
    video = torch.stack([a, b])                                          # B = 2
    table = fps_plan(n, rate).table
    plain, fps = VideoPreprocessor(**pkw), VideoPreprocessor(src_fps=rate, **pkw)
    want = plain(select(video, table).to(DEV), **ckw)                    # the existing launch on the frames selected beforehand
    assert tuple(want.shape) == (2, 2, 3, 16, 224, 224)
    table_entry = "vaura_video_preprocess_frames" if layout in ("nchw", "nhwc") else "vaura_video_preprocess_yuv420_frames"
    assert calls[table_entry] == 0
    got = fps(video.to(DEV), **ckw)                                      # from the device
    assert calls[table_entry] == 1 and torch.equal(got, want)
    assert torch.equal(fps(video, **ckw), want)                          # from the host: only the named frames are copied
    assert torch.equal(plain(video.to(DEV), src_fps=rate, **ckw), want)  # the rate as a keyword of the call
    assert calls[table_entry] == 3
    assert torch.equal(got.cpu(), fps.scale_normalize(fps.reference_u8(video, **ckw)))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_list_of_two_geometries_and_per_clip_timestamps(layout):
    a, pkw, ckw = make_clip(layout, 39, H, W, seed=1)
    b = make_clip(layout, 39, 224, 224, seed=2)[0]
    if layout == "i420":                                                 # size= describes one surface geometry per call
        b = make_clip(layout, 39, H, W, seed=2)[0]
    plain = VideoPreprocessor(**pkw)
    table = fps_plan(39, 30).table
    want = torch.cat([plain(select(a, table, 0).to(DEV), **ckw), plain(select(b, table, 0).to(DEV), **ckw)])
    fps = VideoPreprocessor(src_fps=30, **pkw)
    assert torch.equal(fps([a.to(DEV), b], **ckw), want)                 # a device clip and a host clip
    assert torch.equal(fps([a, b.to(DEV)], **ckw), want)
    # per-clip pts: two different tables in one call (both give 33 frames -> 2 segments)
    tb = Fraction(1, 90000)
    pa, pb = R.jittered_pts(39, Fraction(30), seed=3), R.jittered_pts(39, Fraction(30), seed=4)
    ta, tb_ = fps_plan(pts=pa, time_base=tb).table, fps_plan(pts=pb, time_base=tb).table
    assert ta.tolist() != tb_.tolist() and len(ta) >= 32 and len(tb_) >= 32
    one = VideoPreprocessor(n_segments=2, **pkw)
    want = torch.cat([one(select(a, ta, 0).to(DEV), **ckw), one(select(b, tb_, 0).to(DEV), **ckw)])
    assert torch.equal(one([a.to(DEV), b.to(DEV)], pts=[pa, pb], time_base=tb, **ckw), want)
    assert torch.equal(one([a, b], pts=[pa, pb], time_base=tb, **ckw), want)
    if a.shape == b.shape:                                               # the same as one batch: one launch, two tables
        assert torch.equal(one(torch.stack([a, b]).to(DEV), pts=[pa, pb], time_base=tb, **ckw), want)


@pytest.mark.parametrize("n,kw,S", [(20, dict(n_segments=1), 1), (39, dict(step_size_seg=0.5), 3)], ids=["one_of_17", "half_step"])
def test_the_segment_rule_acts_on_the_converted_sequence(n, kw, S):
    video = noise_video(n, H, W, seed=n)[None]
    table = fps_plan(n, 30).table
    plain = VideoPreprocessor(**kw)
    want = plain(select(video, table).to(DEV))
    assert tuple(want.shape) == (1, S, 3, 16, 224, 224)
    for src in (video, video.to(DEV)):
        assert torch.equal(VideoPreprocessor(src_fps=30, **kw)(src), want)
    if n == 20:                                                          # T = 20 would centre one segment at frame 2; T' = 17 starts at 0
        assert not torch.equal(plain(video.to(DEV)), want)


@pytest.mark.parametrize("layout", ["nchw", "nv12"])
def test_at_25_fps_the_existing_launch_runs(layout, calls):
    v, pkw, ckw = make_clip(layout, 32, H, W, seed=7)
    video = v[None].to(DEV)
    want = VideoPreprocessor(**pkw)(video, **ckw)
    old = "vaura_video_preprocess" if layout == "nchw" else "vaura_video_preprocess_yuv420"
    assert calls[old] == 1
    for pre, kw in ((VideoPreprocessor(src_fps=None, **pkw), {}), (VideoPreprocessor(src_fps=25, **pkw), {}),
                    (VideoPreprocessor(src_fps=(50, 2), **pkw), {}), (VideoPreprocessor(**pkw), dict(src_fps=25.0))):
        assert torch.equal(pre(video, **ckw, **kw), want)
    assert calls[old] == 5 and calls["vaura_video_preprocess_frames"] == 0 and calls["vaura_video_preprocess_yuv420_frames"] == 0
    # timestamps at exactly 25 fps select every frame once: the table launch, the same bits
    got = VideoPreprocessor(**pkw)(video, pts=list(range(0, 32 * 40, 40)), time_base=(1, 1000), **ckw)
    assert torch.equal(got, want) and calls["vaura_video_preprocess_frames"] + calls["vaura_video_preprocess_yuv420_frames"] == 1


# ---------------------------------------------------------------------------------------------------------------- 2. the op
def _raw(pre, v, out, dmap, carry, uses):
    """vaura_video_preprocess_frames with a device map as given (the host wrapper would refuse a bad one first)."""
    b, T, C, h, w = v.shape
    g = pre.geometry(h, w)
    tile_rows, tile_src = g.tiles(False)
    h_rel, h_w, v_start, v_w = g.device_tables(v.device)
    lut = pre.lut.to(v.device)
    rc = L.lib().vaura_video_preprocess_frames(
        L.ptr(v), 0, b, T, C, h, w, pre.resize, pre.crop[0], pre.crop[1], pre.segment_size_vframes, out.shape[1], L.ptr(h_rel), L.ptr(h_w),
        g.h["taps"], g.h["prec"], L.ptr(v_start), L.ptr(v_w), g.v["taps"], g.v["prec"], g.x0, g.span, tile_rows, tile_src, L.ptr(lut),
        L.ptr(out), L.ptr(dmap), L.ptr(carry), int(uses), L.current_stream(v.device))
    torch.cuda.synchronize()
    return rc


def test_map_values_keep_carry_and_clamp():
    T, F = 5, 4
    pre = VideoPreprocessor(segment_size_vframes=F)
    big = torch.stack([noise_video(T + 8, H, W, seed=11), noise_video(T + 8, H, W, seed=12)]).to(DEV)     # (2, 13, 3, H, W)
    v = big[:, 4:4 + T].contiguous()
    carry = noise_video(2, H, W, seed=13).to(DEV)                        # one frame per clip
    per_frame = lambda frames: pre(frames.repeat_interleave(F, dim=1))[:, :, :, :1]  # noqa: E731  (b, n, 3, 1, h, w): every frame on its own
    want_v, want_c = per_frame(v), per_frame(carry[:, None])
    # -1 keeps the bytes that were there (NaN), -2 reads the clip's carried frame, e >= 0 frame e of the clip
    fmap = np.array([[3, -1, -2, 0], [-2, 4, -1, -1]], np.int32)
    out = torch.full((2, 1, 3, F, 224, 224), float("nan"), device=DEV)
    pre._launch(v, out, torch.device(DEV), fmap=fmap, carry=carry)
    for b in range(2):
        for f in range(F):
            e, got = int(fmap[b, f]), out[b, 0, :, f]
            if e == -1:
                assert bool(torch.isnan(got).all()), (b, f)
            else:
                assert torch.equal(got, (want_c[b, 0] if e == -2 else want_v[b, e])[:, 0]), (b, f)
    # without a carry buffer -2 is refused by the host, and so is every index outside [-2, T)
    for bad in (np.array([[0, 0, 0, -2]] * 2, np.int32), np.array([[0, 0, 0, T]] * 2, np.int32), np.array([[0, 0, -3, 0]] * 2, np.int32)):
        with pytest.raises(L.VauraHipError):
            pre._launch(v, out, torch.device(DEV), fmap=bad)
    # the kernel itself clamps: T + 3 and T read frame T - 1, -4 and -3 frame 0 of the clip.  The clip is the middle of a longer
    # one (4 frames on either side), so an unclamped read would stay inside the allocation and show as another frame's pixels.
    one = big[:1, 4:4 + T]
    assert one.is_contiguous() and one.data_ptr() == big.data_ptr() + 4 * 3 * H * W
    dmap = torch.tensor([[T + 3, -4, T, -3]], dtype=torch.int32, device=DEV)
    out1 = torch.full((1, 1, 3, F, 224, 224), float("nan"), device=DEV)
    assert _raw(pre, one, out1, dmap, None, 0) == 0
    for f, e in enumerate((T - 1, 0, T - 1, 0)):
        assert torch.equal(out1[0, 0, :, f], want_v[0, e][:, 0]), f
    # a -2 that reaches the kernel without a carry buffer leaves the frame as it is; with carry_used the call is refused
    out1.fill_(float("nan"))
    dmap2 = torch.tensor([[-2, 1, -2, -1]], dtype=torch.int32, device=DEV)
    assert _raw(pre, one, out1, dmap2, None, 1) == -1 and bool(torch.isnan(out1).all())
    assert _raw(pre, one, out1, dmap2, None, 0) == 0
    assert bool(torch.isnan(out1[0, 0, :, [0, 2, 3]]).all()) and torch.equal(out1[0, 0, :, 1], want_v[0, 1][:, 0])


# ---------------------------------------------------------------------------------------------------------------- 3. the stream
def run_stream(pre, video, split, ckw, pts=None, **skw):
    vs = pre.open_stream(video.shape[0], size=ckw.get("size"), chroma_row=ckw.get("chroma_row"), **skw)
    segs, n = [], video.shape[1]
    for lo in range(0, n, split):
        hi = min(lo + split, n)
        segs += vs.push(video[:, lo:hi], None if pts is None else pts[lo:hi])
    segs += vs.close()
    return segs, vs


@pytest.mark.parametrize("timing", ["constant", "jittered"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stream_equals_one_pass_for_every_split(layout, timing):
    n = 50
    a, pkw, ckw = make_clip(layout, n, H, W, seed=21)
    video = torch.stack([a, make_clip(layout, n, H, W, seed=22)[0]])
    if timing == "constant":
        pts, skw, plan = None, dict(src_fps=30), fps_plan(n, 30)                         # 42 ticks: 2 segments, 10 ticks dropped
    else:
        pts = R.jittered_pts(n, Fraction(30), seed=5)
        skw, plan = dict(time_base=(1, 90000)), fps_plan(pts=pts, time_base=(1, 90000))
    S = plan.n_out // 16
    assert S == 2
    pre = VideoPreprocessor(**pkw)
    want = pre(select(video, plan.table[:S * 16]).to(DEV), **ckw)
    for split, src in ((1, video.to(DEV)), (7, video), (n, video.to(DEV))):
        segs, vs = run_stream(pre, src, split, ckw, pts, **skw)
        assert len(segs) == S == vs.segments and vs.dropped_ticks == plan.n_out - 16 * S
        assert all(tuple(s.shape) == (2, 1, 3, 16, 224, 224) for s in segs)
        assert torch.equal(torch.cat(segs, dim=1), want), split


def test_stream_slow_source_close_and_state_size():
    """12.5 fps: every frame is shown twice, so most ticks come from the carried frame; 24 fps pushed one frame at a time.  The
    device state is one segment and one frame per clip however long the video is."""
    pre = VideoPreprocessor()
    for rate, n in ((Fraction(25, 2), 52), (24, 95)):                    # 104 ticks -> 6 segments + 8; 99 ticks -> 6 segments + 3
        video = noise_video(n, H, W, seed=n)[None].to(DEV)
        plan = fps_plan(n, rate)
        want = pre(select(video, plan.table[:96]))
        vs = pre.open_stream(1, src_fps=rate)
        segs, sizes = [], {}
        for i in range(n):
            segs += vs.push(video[0, i:i + 1])                           # (n, C, H, W) with B == 1
            sizes.setdefault(vs.segments, (tuple(vs._pending.shape), tuple(vs._carry.shape), vs._pending.data_ptr() != 0))
        assert vs.push(video[:, :0]) == []
        segs += vs.close()
        assert len(segs) == 6 and vs.dropped_ticks == plan.n_out - 96 and torch.equal(torch.cat(segs, dim=1), want)
        assert sizes[2] == sizes[5] == ((1, 1, 3, 16, 224, 224), (1, 3, H, W), True)
        assert vs._pending is None and vs._carry is None
        assert len({s.data_ptr() for s in segs}) == 6                    # a returned segment is never written again
    # an end that the stream only learns at close(): the last frame is held for 10 more ticks, which completes a segment
    pts = list(range(0, 10 * 40, 40))                                    # 10 frames at 25 fps
    video = noise_video(10, H, W, seed=3)[None].to(DEV)
    vs = pre.open_stream(1, time_base=(1, 1000))
    assert vs.push(video, pts) == []
    segs = vs.close(end=16 * 40)
    assert len(segs) == 1 and vs.dropped_ticks == 0
    assert torch.equal(segs[0], pre(select(video, list(range(10)) + [9] * 6)))


# ---------------------------------------------------------------------------------------------------------------- 4. end to end
def test_live_session_fed_through_a_video_stream(tiny_sampler_sd):
    """30 fps frames -> open_video_stream -> LiveSession.push(frames=), over 5 segments: the blocks are those of a session fed the
    segments of the frames selected on the host beforehand (the tiny model of tests/test_gpu_live.py)."""
    import test_gpu_per_clip_sampling as G
    model = G._model(tiny_sampler_sd)
    fx = model.visual_feature_extractor
    fx.extract_features = True
    fx.load_state_dict(synth.avclip_state_dict(seed=0), strict=True)
    fx.to(DEV)
    B, n = 2, 96                                                         # 96 frames at 30 fps = 80 ticks = 5 segments
    video = torch.stack([noise_video(n, H, W, seed=31), noise_video(n, H, W, seed=32)])
    plan = fps_plan(n, 30)
    assert plan.n_out == 80
    want_segs = model.frames_from_video(select(video, plan.table).to(DEV))
    assert tuple(want_segs.shape) == (B, 5, 3, 16, 224, 224)
    assert torch.equal(model.frames_from_video(video, src_fps=30), want_segs)
    kw = dict(use_sampling=False, cfg_scale=1.0)
    ref = model.open_live(B, block_frames=16, **kw)
    want = []
    for s in range(5):
        want += ref.push(frames=want_segs[:, s:s + 1].contiguous())
    want += ref.close()
    session = model.open_live(B, block_frames=16, **kw)
    vs = model.open_video_stream(B, src_fps=30)
    blocks, pushed = [], 0
    for lo in range(0, n, 10):                                           # a decoder's blocks of 10 frames, from the host
        for seg in vs.push(video[:, lo:lo + 10]):
            blocks += session.push(frames=seg)
            pushed += 1
    for seg in vs.close():
        blocks += session.push(frames=seg)
        pushed += 1
    blocks += session.close()
    assert pushed == 5 and vs.dropped_ticks == 0 and len(blocks) == len(want) > 1
    for x, y in zip(blocks, want):
        assert x["start_frame"] == y["start_frame"] and x["frames"] == y["frames"]
        assert torch.equal(x["sampled_indices"], y["sampled_indices"]) and torch.equal(x["audio"], y["audio"])
    with pytest.raises(L.VauraHipError, match="src_fps"):
        model.open_video_stream(B)
