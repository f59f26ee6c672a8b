"""Video at its own frame rate, host side (no GPU): ``fps_plan`` / ``FpsClock`` (vaura_amd/preprocess.py) against the literal queue of
tests/preprocess_fps_reference.py and against known answers, every refusal, the CPU restatement with a rate, and the argument checks
of the two C entry points (refused before any launch, so they run without a device)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import preprocess_fps_reference as R
from test_preprocess_host import noise_video
from vaura_amd import _lib as L
from vaura_amd.preprocess import FpsClock, VideoFrameStream, VideoPreprocessor, as_rate, fps_plan
from yuv_cases import noise_planes, pack


def test_as_rate():
    assert as_rate(30) == 30 and as_rate(Fraction(25, 2)) == Fraction(25, 2) and as_rate((30000, 1001)) == Fraction(30000, 1001)
    assert as_rate(29.97) == Fraction(2997, 100) and as_rate(12.5) == Fraction(25, 2)
    for bad in (0, -25, (0, 1), (-1, 2), 0.0, "30", None, True, (30, 0), float("nan")):
        with pytest.raises(L.VauraHipError):
            as_rate(bad)


@pytest.mark.parametrize("name", list(R.RATES))
def test_plan_equals_the_queue_at_constant_rates(name):
    rate = R.RATES[name]
    for n in range(1, 81):
        first, want = R.simulate_constant(n, rate)
        p = fps_plan(n, rate)
        assert p.first_tick == first == 0 and p.n_out == len(want) and p.table.dtype == np.int32, (name, n)
        assert p.table.tolist() == want, (name, n)


@pytest.mark.parametrize("seed", range(6))
def test_plan_equals_the_queue_on_timestamps(seed):
    for n in (1, 2, 3, 17, 64):
        for fps in (Fraction(30), Fraction(60), Fraction(24000, 1001)):
            pts, tb = R.jittered_pts(n, fps, seed), Fraction(1, 90000)
            for end in (None, pts[-1] + 1, pts[-1] + 9000):
                first, want = R.simulate_pts(pts, tb, end)
                p = fps_plan(pts=pts, time_base=tb, end=end)
                assert (p.first_tick, p.table.tolist()) == (first, want), (n, fps, end)
        pts, tb = R.variable_pts(n, seed), Fraction(1, 1000)
        first, want = R.simulate_pts(pts, tb)
        p = fps_plan(pts=np.array(pts), time_base=(1, 1000))
        assert (p.first_tick, p.table.tolist(), p.n_out) == (first, want, len(want)), n
        assert first == R.round_half_away(pts[0] * tb * 25)              # a video that does not start at 0 keeps its first tick


def test_known_answers():
    for n, rate, n_out, begins in R.KNOWN:
        p = fps_plan(n, rate)
        assert p.n_out == n_out and p.table[:len(begins)].tolist() == begins, (n, rate)
    t = fps_plan(39, 30).table.tolist()
    assert sorted(set(range(39)) - set(t)) == R.DROPPED_39_AT_30 and t == sorted(t) and len(set(t)) == 33
    assert fps_plan(39, (30000, 1001)).table.tolist() == t
    t24 = fps_plan(31, 24).table.tolist()
    assert set(t24) == set(range(31)) and [i for i in range(31) if t24.count(i) == 2] == [11]
    assert 0 not in fps_plan(77, 60).table.tolist()                       # frames 0 and 1 both round to tick 0: 1 replaces 0
    assert fps_plan(16, Fraction(25, 2)).table.tolist() == [i // 2 for i in range(32)]
    assert fps_plan(0, 30).n_out == 0 and fps_plan(1, 1000).n_out == 0     # N_out = max(r_end - r_0, 0)


def clock_in_pushes(make, frames, split, end=None):
    """The clock over `frames` (a count or a pts list) in pushes of `split` -> (ticks in order, the checks of the decision rule)."""
    c, got = make(), []
    n = frames if isinstance(frames, int) else len(frames)
    for lo in range(0, n, split):
        hi = min(lo + split, n)
        new = c.push(hi - lo if isinstance(frames, int) else frames[lo:hi])
        # decided only once a frame with a larger r has arrived: every decided tick lies below the r of the newest frame and
        # never shows that frame (a later one may still replace it)
        assert all(tick < c.next_tick and src <= c.n - 2 for tick, src in new)
        got += new
    assert c.push(0 if isinstance(frames, int) else []) == []
    got += c.close(end)
    return got, c


@pytest.mark.parametrize("split", [1, 7, 10 ** 6])
def test_clock_concatenates_to_the_plan(split):
    for name, rate in R.RATES.items():
        for n in (1, 2, 20, 39, 77):
            p = fps_plan(n, rate)
            got, c = clock_in_pushes(lambda: FpsClock(rate), n, split)
            assert [t for t, _ in got] == list(range(p.first_tick, p.first_tick + p.n_out)), (name, n)
            assert [s for _, s in got] == p.table.tolist(), (name, n)
    for seed in range(3):
        for pts, tb, end in ((R.jittered_pts(50, Fraction(30), seed), Fraction(1, 90000), None),
                             (R.variable_pts(50, seed), Fraction(1, 1000), None),
                             (R.variable_pts(50, seed), Fraction(1, 1000), R.variable_pts(50, seed)[-1] + 333)):
            p = fps_plan(pts=pts, time_base=tb, end=end)
            got, c = clock_in_pushes(lambda: FpsClock(time_base=tb), pts, split, end)
            assert [t for t, _ in got] == list(range(p.first_tick, p.first_tick + p.n_out)) and c.first_tick == p.first_tick
            assert [s for _, s in got] == p.table.tolist()


def test_no_tick_is_decided_early():
    c = FpsClock(30)
    assert c.push(1) == []                                               # frame 0 alone decides nothing
    assert c.push(1) == [(0, 0)]                                         # r_1 = 1 > 0
    assert c.push(2) == [(1, 1), (2, 2)]                                 # r_2 = 2, r_3 = 3 (2.5 rounds away from zero)
    assert c.push(1) == []                                               # r_4 = 3: frame 3 is dropped, tick 3 still open
    assert c.push(1) == [(3, 4)]
    assert c.close() == [(4, 5)]                                         # r_end = rnd(6 * 25 / 30) = 5
    slow = FpsClock(Fraction(25, 2))
    assert slow.push(1) == [] and slow.push(1) == [(0, 0), (1, 0)] and slow.close() == [(2, 1), (3, 1)]


def test_refusals_of_the_plan_and_the_clock():
    bad = [dict(), dict(n_frames=10), dict(src_fps=30), dict(n_frames=10, src_fps=30, pts=[0, 1], time_base=1), dict(pts=[0, 1]),
           dict(time_base=(1, 1000)), dict(n_frames=10, src_fps=30, time_base=(1, 1000)), dict(n_frames=10, src_fps=0),
           dict(n_frames=-1, src_fps=30), dict(n_frames=10, src_fps=30, end=4), dict(n_frames=10, src_fps=30, dst_fps=0),
           dict(pts=[0, 40, 40], time_base=(1, 1000)), dict(pts=[0, 40, 39], time_base=(1, 1000)), dict(pts=[0.0, 40.0], time_base=(1, 1000)),
           dict(pts=[0, 40], time_base=(1, 1000), end=40), dict(pts=[0, 40], time_base=0)]
    for kw in bad:
        with pytest.raises(L.VauraHipError):
            fps_plan(**kw)
    for kw in (dict(), dict(src_fps=30, time_base=(1, 1000)), dict(src_fps=-1)):
        with pytest.raises(L.VauraHipError):
            FpsClock(**kw)
    c = FpsClock(time_base=(1, 1000))
    c.push([0, 40])
    for frames in ([40], [30, 50], 3, [41.5]):
        with pytest.raises(L.VauraHipError):
            c.push(frames)
    with pytest.raises(L.VauraHipError, match="behind"):
        c.close(end=40)
    assert c.close(end=80) == [(1, 1)]                                  # a refused close leaves the clock open
    k = FpsClock(30)
    with pytest.raises(L.VauraHipError):
        k.push([0, 1])
    with pytest.raises(L.VauraHipError):
        k.push(-1)
    k.push(3)
    with pytest.raises(L.VauraHipError, match="pts"):
        k.close(end=7)
    k = FpsClock(30)
    k.close()
    for call in (lambda: k.push(1), k.close):
        with pytest.raises(L.VauraHipError):
            call()


@pytest.mark.parametrize("rate,n,kw", [(30, 39, {}), ((30000, 1001), 39, {}), (24, 31, {}), (60, 77, {}), (Fraction(25, 2), 16, {}),
                                       (30, 20, dict(n_segments=1)), (30, 39, dict(step_size_seg=0.5))])
def test_reference_u8_with_a_rate_is_reference_u8_of_the_selected_frames(rate, n, kw):
    video = noise_video(n, 36, 48, seed=n)
    table = torch.from_numpy(fps_plan(n, rate).table.astype(np.int64))
    plain = VideoPreprocessor(resize=32, crop=(24, 24), **kw)
    want = plain.reference_u8(video[table])
    assert want.shape[1] == (3 if "step_size_seg" in kw else (1 if kw else 2))
    assert torch.equal(VideoPreprocessor(resize=32, crop=(24, 24), src_fps=rate, **kw).reference_u8(video), want)
    assert torch.equal(plain.reference_u8(video, src_fps=rate), want)
    assert torch.equal(plain.reference_u8(video[None], src_fps=[rate]), want)
    # the segment rule acts on the selected sequence: cutting first and selecting afterwards is something else
    if n == 39 and not kw:
        assert not torch.equal(plain.reference_u8(video[:32]), want)


def test_reference_u8_with_pts_rates_per_clip_and_yuv():
    a, b = noise_video(39, 36, 48, seed=1), noise_video(31, 40, 40, seed=2)
    pre = VideoPreprocessor(resize=32, crop=(24, 24))
    sel = lambda v, p: v[torch.from_numpy(p.table.astype(np.int64))]  # noqa: E731
    want = torch.cat([pre.reference_u8(sel(a, fps_plan(39, 30))), pre.reference_u8(sel(b, fps_plan(31, 24)))])
    assert torch.equal(pre.reference_u8([a, b], src_fps=[30, 24]), want)
    pa, pb = R.jittered_pts(39, Fraction(30), 3), R.variable_pts(31, 4, Fraction(1, 90000))
    pb = [p * 40 for p in pb]                                            # gaps of 5 .. 120 ticks of 1/90000 s are too short: stretch them
    plans = [fps_plan(pts=pa, time_base=(1, 90000)), fps_plan(pts=pb, time_base=(1, 90000))]
    assert plans[0].table.tolist() != plans[1].table.tolist()
    n = min(p.n_out for p in plans) // 16
    one = VideoPreprocessor(resize=32, crop=(24, 24), n_segments=n)
    want = torch.cat([one.reference_u8(sel(a, plans[0])), one.reference_u8(sel(b, plans[1]))])
    assert torch.equal(one.reference_u8([a, b], pts=[pa, pb], time_base=(1, 90000)), want)
    same = torch.stack([a, a])                                           # one pts list serves every clip of a batch
    assert torch.equal(one.reference_u8(same, pts=pa, time_base=(1, 90000))[1], one.reference_u8(sel(a, plans[0]))[0])
    yuv = VideoPreprocessor(resize=32, crop=(24, 24), input_format="nv12")
    surf = pack(*noise_planes(39, 36, 48, seed=5), "nv12")
    assert torch.equal(yuv.reference_u8(surf, src_fps=30), yuv.reference_u8(sel(surf, fps_plan(39, 30))))


def test_refusals_of_the_preprocessor_and_the_stream():
    video = noise_video(39, 36, 48, seed=1)
    pre = VideoPreprocessor(resize=32, crop=(24, 24))
    ref = pre.reference_u8
    for kw in (dict(src_fps=0), dict(src_fps=30, pts=list(range(39)), time_base=(1, 30)), dict(pts=list(range(39))),
               dict(time_base=(1, 30)), dict(end=40), dict(pts=list(range(38)), time_base=(1, 30)), dict(src_fps=[30, 30]),
               dict(pts=[list(range(39))] * 2, time_base=(1, 30)), dict(pts=[0] * 39, time_base=(1, 30))):
        with pytest.raises(L.VauraHipError):
            ref(video, **kw)
    with pytest.raises(L.VauraHipError, match="shorter than one segment"):
        ref(video[:18], src_fps=30)                                      # 18 frames at 30 fps are 15 at 25
    with pytest.raises(L.VauraHipError, match="same number of segments"):
        ref([video, video[:20]], src_fps=30)
    with pytest.raises(L.VauraHipError):
        VideoPreprocessor(src_fps=-30)
    with pytest.raises(L.VauraHipError):
        VideoPreprocessor(dst_fps=0)
    for kw in (dict(step_size_seg=0.5), dict(n_segments=2)):
        with pytest.raises(L.VauraHipError, match="back-to-back"):
            VideoPreprocessor(**kw).open_stream(1, src_fps=30)
    with pytest.raises(L.VauraHipError, match="one clock"):
        VideoFrameStream(pre, 2, src_fps=[30, 24])
    with pytest.raises(L.VauraHipError):
        VideoFrameStream(pre, 2, src_fps=30, time_base=(1, 1000))
    with pytest.raises(L.VauraHipError, match="4:2:0"):
        pre.open_stream(1, src_fps=30, size=(36, 48))
    vs = pre.open_stream(2, src_fps=30)
    for frames, pts in ((video.float()[None], None), (video, None), (video[None], None), (torch.stack([video, video]), [0] * 39)):
        with pytest.raises(L.VauraHipError):
            vs.push(frames, pts)
    ts = pre.open_stream(1, time_base=(1, 1000))
    with pytest.raises(L.VauraHipError, match="one pts per frame"):
        ts.push(video)
    with pytest.raises(L.VauraHipError, match="one pts per frame"):
        ts.push(video, list(range(38)))
    assert ts.push(video[:0], []) == [] and ts.close() == [] and ts.dropped_ticks == 0     # nothing pushed: no device is touched
    with pytest.raises(L.VauraHipError, match="after close"):
        ts.push(video[:0], [])


def _tables():
    z = lambda n, dt: torch.zeros(n, dtype=dt)  # noqa: E731
    return z(24, torch.int32), z(24 * 33, torch.int16), z(24, torch.int32), z(24 * 33, torch.int16), z(768, torch.float32)


def _rgb(video, out, tabs, fmap, carry=None, **over):
    a = dict(channels_last=0, n_clips=1, T=4, C=3, H=64, W=64, resize=32, crop_h=24, crop_w=24, F=16, S=1, h_taps=5, h_prec=15, v_taps=5,
             v_prec=15, x0=0, span=64, tile_rows=8, tile_src_rows=32, carry_used=0)
    a.update(over)
    h_rel, h_w, v_start, v_w, lut = tabs
    return L.lib().vaura_video_preprocess_frames(
        L.ptr(video), a["channels_last"], a["n_clips"], a["T"], a["C"], a["H"], a["W"], a["resize"], a["crop_h"], a["crop_w"], a["F"], a["S"],
        L.ptr(h_rel), L.ptr(h_w), a["h_taps"], a["h_prec"], L.ptr(v_start), L.ptr(v_w), a["v_taps"], a["v_prec"], a["x0"], a["span"],
        a["tile_rows"], a["tile_src_rows"], L.ptr(lut), L.ptr(out), L.ptr(fmap), L.ptr(carry), a["carry_used"], 0)


def _yuv(video, out, tabs, fmap, carry=None, **over):
    a = dict(video_bytes=0 if video is None else video.numel(), layout=0, pitch=64, chroma_offset=64 * 64, frame_stride=96 * 64, n_clips=1, T=4,
             H=64, W=64, color=(16, 19077, 26149, -6419, -13320, 33050), resize=32, crop_h=24, crop_w=24, F=16, S=1, h_taps=5, h_prec=15,
             v_taps=5, v_prec=15, x0=0, span=64, tile_rows=8, tile_src_rows=32, carry_used=0)
    a.update(over)
    h_rel, h_w, v_start, v_w, lut = tabs
    return L.lib().vaura_video_preprocess_yuv420_frames(
        L.ptr(video), a["video_bytes"], a["layout"], a["pitch"], a["chroma_offset"], a["frame_stride"], a["n_clips"], a["T"], a["H"], a["W"],
        *a["color"], a["resize"], a["crop_h"], a["crop_w"], a["F"], a["S"], L.ptr(h_rel), L.ptr(h_w), a["h_taps"], a["h_prec"],
        L.ptr(v_start), L.ptr(v_w), a["v_taps"], a["v_prec"], a["x0"], a["span"], a["tile_rows"], a["tile_src_rows"], L.ptr(lut), L.ptr(out),
        L.ptr(fmap), L.ptr(carry), a["carry_used"], 0)


def test_c_entry_points_are_exported_and_refuse_before_any_launch():
    """Host memory stands in for device memory: every call below is refused by the argument checks, which come before any launch
    (tests/test_gpu_preprocess_fps.py runs the accepted call)."""
    assert "vaura_video_preprocess_frames" in L.SIGNATURES and "vaura_video_preprocess_yuv420_frames" in L.SIGNATURES
    lib = L.lib()
    assert lib.vaura_video_preprocess_frames and lib.vaura_video_preprocess_yuv420_frames
    SHAPE, ARG = -2, -1
    tabs = _tables()
    out = torch.full((1, 1, 3, 16, 24, 24), 7.0)
    fmap = torch.zeros(16, dtype=torch.int32)
    rgb, yuv = torch.zeros(4, 3, 64, 64, dtype=torch.uint8), torch.zeros(4, 96, 64, dtype=torch.uint8)
    for call, video in ((_rgb, rgb), (_yuv, yuv)):
        assert call(video, out, tabs, None) == ARG                       # no map
        assert call(video, out, tabs, fmap.view(torch.uint8)[1:5]) == ARG   # a misaligned map
        assert call(video, out, tabs, fmap, carry_used=1) == ARG         # the host says the map names the carried frame; there is none
        assert call(None, out, tabs, fmap) == ARG
        assert call(video, None, tabs, fmap) == ARG
        assert call(video, out, tabs, fmap, T=0) == ARG
        assert call(video, out, tabs, fmap, S=0) == SHAPE
        assert call(video, out, tabs, fmap, S=70000) == SHAPE
        assert call(video, out, tabs, fmap, n_clips=4096) == SHAPE       # more than 65535 output frames
        assert call(video, out, tabs, fmap, crop_w=22) == SHAPE          # and what the sibling's check refuses
        assert call(video, out, tabs, fmap, crop_h=33) == SHAPE
        assert call(video, out, tabs, fmap, h_taps=33) == SHAPE
        assert call(video, out, tabs, fmap, span=65) == ARG
        assert call(video, out, tabs, fmap, tile_src_rows=4) == ARG
    assert _rgb(rgb, out, tabs, fmap, C=4) == SHAPE
    assert _yuv(yuv, out, tabs, fmap, H=63) == SHAPE
    assert _yuv(yuv, out, tabs, fmap, layout=2) == ARG
    assert _yuv(yuv, out, tabs, fmap, pitch=63) == ARG
    assert _yuv(yuv, out, tabs, fmap, video_bytes=yuv.numel() - 1) == ARG
    assert _yuv(yuv, out, tabs, fmap, frame_stride=96 * 64 - 1) == ARG
    assert _yuv(yuv, out, tabs, fmap, color=(16, 1 << 21, 0, 0, 0, 0)) == ARG
    assert bool((out == 7.0).all())


def test_host_refusals_of_a_frame_map():
    pre = VideoPreprocessor(resize=32, crop=(24, 24))
    ok = np.zeros((1, 16), np.int32)
    assert pre._check_map(ok, 1, 4, 1, None) is False
    carry = torch.zeros(1, 3, 64, 64, dtype=torch.uint8)
    assert pre._check_map(np.full((1, 16), -2, np.int32), 1, 4, 1, carry) is True
    for fmap in (np.full((1, 16), 4, np.int32), np.full((1, 16), -3, np.int32), np.zeros((1, 15), np.int32), np.zeros((1, 16), np.int64),
                 np.full((1, 16), -2, np.int32)):
        with pytest.raises(L.VauraHipError):
            pre._check_map(fmap, 1, 4, 1, None)
