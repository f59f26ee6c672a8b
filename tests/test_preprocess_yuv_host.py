"""Video preprocessing from 4:2:0 decoder surfaces, host side (vaura_amd/preprocess.py): the integer colour formula against a float64
evaluation of the same real coefficients, the two layouts, padded surfaces and every refusal.  No GPU.

What the expectation is.  The reference does not pin the colour step: its loader gets RGB from torchvision / PyAV (swscale), neither
of which is installed.  The formula is the project's: BT.601 / BT.709, limited or full range, coefficients rounded to 2^-14, chroma
replicated.  Its bound against the real-valued formula is rounding (0.5) plus coefficient quantisation, at most 2^-15 per coefficient
over |Y - y_off| <= 239 and |C - 128| <= 128 twice: 0.5 + 495 * 2^-15 = 0.5151 levels, on the level BEFORE the clamp."""
import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd.preprocess import (VideoPreprocessor, yuv420_planes, yuv420_to_rgb_u8, yuv_coefficients, yuv_coefficients_f64)
from yuv_cases import CONTENTS, GEOMETRIES, noise_planes, pack

BOUND = 0.5 + 495 * 2.0 ** -15


def test_bt601_limited_integers_and_grey():
    assert yuv_coefficients() == (16, 19077, 26149, -6419, -13320, 33050)
    assert yuv_coefficients("bt601", "limited") == yuv_coefficients()
    assert yuv_coefficients("bt709", "full")[:2] == (0, 1 << 14)
    grey = torch.full((1, 2, 2), 128, dtype=torch.uint8)[:, :1, :1]
    for Y, want in ((16, 0), (235, 255), (0, 0), (255, 255), (126, 128)):
        rgb = yuv420_to_rgb_u8(torch.full((1, 2, 2), Y, dtype=torch.uint8), grey, grey)
        assert tuple(rgb.shape) == (1, 3, 2, 2) and bool((rgb == want).all()), (Y, want)


@pytest.mark.parametrize("color_range", ["limited", "full"])
@pytest.mark.parametrize("color_matrix", ["bt601", "bt709"])
def test_all_triples_against_float64(color_matrix, color_range):
    """All 2^24 (Y, U, V): |acc >> 14 - exact| <= 0.5151 for the three channels; the accumulators stay within +-9.0e6."""
    y_off, cy, crv, cgu, cgv, cbu = yuv_coefficients(color_matrix, color_range)
    _, (fy, frv, fgu, fgv, fbu) = yuv_coefficients_f64(color_matrix, color_range)
    u = (torch.arange(256, dtype=torch.int32) - 128).view(1, 256, 1)
    v = (torch.arange(256, dtype=torch.int32) - 128).view(1, 1, 256)
    worst, acc_max = 0.0, 0
    for y0 in range(0, 256, 32):
        y = (torch.arange(y0, y0 + 32, dtype=torch.int32) - y_off).view(32, 1, 1)
        for (iu, iv), (fu, fv) in (((0, crv), (0.0, frv)), ((cgu, cgv), (fgu, fgv)), ((cbu, 0), (fbu, 0.0))):
            acc = cy * y + iu * u + iv * v + (1 << 13)
            exact = fy * y.double() + fu * u.double() + fv * v.double()
            worst = max(worst, float(((acc >> 14).double() - exact).abs().max()))
            acc_max = max(acc_max, int(acc.abs().max()))
    print(f"{color_matrix} {color_range}: max |unclamped level - float64| {worst:.5f} (bound {BOUND:.5f}), max |acc| {acc_max:.3e}")
    assert worst <= BOUND
    assert acc_max <= 9.0e6


def test_the_geometries_are_what_they_are_chosen_for():
    g = {hw: VideoPreprocessor().geometry(*hw) for hw in GEOMETRIES}
    first_row = lambda x: int(x.v["start"].min())  # noqa: E731
    assert g[(144, 176)].span % 2 == 1
    assert g[(360, 640)].x0 % 2 == 0 and first_row(g[(360, 640)]) % 2 == 0
    assert (g[(480, 854)].x0, first_row(g[(480, 854)])) == (217, 29)
    assert (g[(224, 224)].x0, first_row(g[(224, 224)])) == (13, 13)
    assert (g[(288, 352)].x0, first_row(g[(288, 352)])) == (49, 17)
    assert g[(256, 340)].h["taps"] == 1 and g[(256, 340)].v["taps"] == 1
    assert g[(1080, 1920)].h["taps"] == 11 and g[(1080, 1920)].x0 == 487


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_reference_u8_of_yuv_is_reference_u8_of_the_converted_rgb(layout):
    T, H, W = 2, 144, 176
    for name, make in CONTENTS.items():
        y, u, v = make(T, H, W, seed=3)
        surf = pack(y, u, v, layout)
        assert tuple(surf.shape) == (T, 3 * H // 2, W)
        py, pu, pv = yuv420_planes(surf, layout)
        assert torch.equal(py, y) and torch.equal(pu, u) and torch.equal(pv, v)
        rgb = yuv420_to_rgb_u8(y, u, v)
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (T, 3, H, W)
        pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
        want = VideoPreprocessor(segment_size_vframes=T).reference_u8(rgb)
        assert torch.equal(pre.reference_u8(surf), want), name
        assert torch.equal(pre.reference_u8(surf[None]), want) and torch.equal(pre.reference_u8([surf, surf])[1:], want)


def test_legal_content_is_in_gamut_and_noise_is_not():
    """What the contents are for: the legal clip never reaches a clamp by more than rounding, the noise and corner clips mostly do."""
    y_off, cy, crv, cgu, cgv, cbu = yuv_coefficients()

    def out_of_gamut(y, u, v):
        yy = (y.int() - y_off) * cy + (1 << 13)
        uu, vv = ((c.int() - 128).repeat_interleave(2, -2).repeat_interleave(2, -1) for c in (u, v))
        lv = torch.stack([yy + crv * vv, yy + cgu * uu + cgv * vv, yy + cbu * uu]) >> 14
        return float(((lv < -2) | (lv > 257)).float().mean()), bool((lv < 0).any()), bool((lv > 255).any())
    assert out_of_gamut(*CONTENTS["legal"](2, 64, 64, 1))[0] == 0.0
    for name in ("noise", "corners"):
        share, below, above = out_of_gamut(*CONTENTS[name](2, 64, 64, 1))
        assert share > 0.2 and below and above, name


def test_nv12_and_i420_of_the_same_planes_are_equal():
    T, H, W = 2, 144, 176
    y, u, v = noise_planes(T, H, W, seed=4)
    a = VideoPreprocessor(segment_size_vframes=T, input_format="nv12").reference_u8(pack(y, u, v, "nv12"))
    b = VideoPreprocessor(segment_size_vframes=T, input_format="i420").reference_u8(pack(y, u, v, "i420"))
    assert torch.equal(a, b)
    # and the matrix / range reach the result
    c = VideoPreprocessor(segment_size_vframes=T, input_format="nv12", color_matrix="bt709", color_range="full")
    want = VideoPreprocessor(segment_size_vframes=T).reference_u8(yuv420_to_rgb_u8(y, u, v, "bt709", "full"))
    assert torch.equal(c.reference_u8(pack(y, u, v, "nv12")), want) and not torch.equal(want, a)


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_padded_surface_equals_the_tight_one(layout):
    T, H, W = 2, 144, 176
    y, u, v = noise_planes(T, H, W, seed=5)
    pre = VideoPreprocessor(segment_size_vframes=T, input_format=layout)
    tight = pre.reference_u8(pack(y, u, v, layout))
    for fill in (1, 2):
        surf = pack(y, u, v, layout, pad=True, fill_seed=fill)
        assert surf.shape[-1] == W + 24 and surf.shape[-2] > H + 8 + H // 2
        assert torch.equal(pre.reference_u8(surf, size=(H, W), chroma_row=H + 8), tight)
    # chroma_row defaults to H
    surf = torch.cat([pack(y, u, v, layout), torch.full((T, 5, W), 77, dtype=torch.uint8)], dim=1)
    assert torch.equal(pre.reference_u8(surf, size=(H, W)), tight)


def test_refusals():
    def bad(match, call, *a, **kw):
        with pytest.raises(L.VauraHipError, match=match):
            call(*a, **kw)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)  # noqa: E731
    nv12, i420 = (VideoPreprocessor(segment_size_vframes=2, input_format=f) for f in ("nv12", "i420"))
    for pre in (nv12, i420):
        for call in (pre.reference_u8, pre):                            # the device call refuses before any device work
            bad("H = 75", call, u8(2, 3 * 75 + 75 // 2 + 1, 100), size=(75, 100))            # odd H
            bad("W = 101", call, u8(2, 150, 101))                                             # tight, odd W
            bad("no multiple of 3", call, u8(2, 100, 100))                                    # tight frames need R = 3H/2
            bad("P = 90", call, u8(2, 150, 90), size=(100, 100))                              # pitch below W
            bad("R = 149", call, u8(2, 149, 100), size=(100, 100))                            # rows do not hold the chroma plane
            bad("R = 150", call, u8(2, 150, 100), size=(100, 100), chroma_row=101)
            bad("chroma_row = 99", call, u8(2, 160, 100), size=(100, 100), chroma_row=99)     # inside the luma plane
            bad("chroma_row needs size", call, u8(2, 150, 100), chroma_row=100)
            bad("contiguous", call, u8(2, 150, 200)[..., ::2])
            bad("contiguous", call, u8(2, 300, 100)[:, ::2])
            bad("float32", call, torch.zeros(2, 150, 100))
            bad("int16", call, torch.zeros(2, 150, 100, dtype=torch.int16))                   # 10-bit surfaces: refused by dtype
            bad(r"\(T, R, P\)", call, [u8(1, 2, 150, 100)])
            bad(r"\(B, T, R, P\)", call, u8(2, 3, 150, 100)[0, 0])
            bad("shorter than one segment", call, u8(1, 150, 100))
    bad("P = 101", i420.reference_u8, u8(2, 150, 101), size=(100, 100))                       # i420: odd pitch
    bad("P = 101", i420, u8(2, 150, 101), size=(100, 100))
    assert tuple(nv12.reference_u8(u8(2, 390, 257), size=(256, 256), chroma_row=260).shape) == (1, 1, 3, 2, 224, 224)   # nv12 may
    bad("channels_last", VideoPreprocessor, channels_last=True, input_format="nv12")
    bad("channels_last", VideoPreprocessor, channels_last=True, input_format="i420")
    bad("'yuv444'", VideoPreprocessor, input_format="yuv444")
    bad("'bt2020'", VideoPreprocessor, color_matrix="bt2020")
    bad("'studio'", VideoPreprocessor, color_range="studio")
    bad("'bt2020'", yuv_coefficients, "bt2020")
    bad("input_format is 'rgb'", VideoPreprocessor(), u8(16, 3, 64, 64), size=(64, 64))
