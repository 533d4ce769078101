"""The ROI pooler restatement (tests/roi_pooler_ref64.py) against the pinned oracle form and against hand-computed answers, and the config
surface of the Faster-RCNN head's pooler (MODEL.ROI_BOX_HEAD.POOLER_TYPE / POOLER_SAMPLING_RATIO / NUM_CONV).  No GPU."""
import pytest
import torch

from oracle import utv2_oracle as O
from tests import roi_pooler_ref64 as R64


def _ramp(H=8, W=8):
    """one channel, feat[y, x] = W * y + x: the maximum of a window is its last pixel, and the value names the pixel"""
    return torch.arange(H * W, dtype=torch.float32).view(1, H, W)


def test_aligned_adaptive_equals_the_pinned_oracle_form():
    """(aligned, ratio 0) is what oracle.roi_align states: forward and autograd gradient to fp32 rounding (the oracle computes the box
    in Python floats and the sample positions in fp32, the restatement everything in the features' dtype)"""
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(6, 13, 17, generator=g)
    xy = torch.rand(9, 2, generator=g) * torch.tensor([60.0, 44.0]) - 6.0
    wh = torch.exp(torch.rand(9, 2, generator=g) * 3.5 + 0.5)
    rois = torch.cat([xy, xy + wh], 1)
    rois[0] = torch.tensor([-30.0, -20.0, 120.0, 90.0])     # larger than the map: grid 3 x 4, samples skipped outside
    rois[1] = torch.tensor([10.0, 8.0, 10.0, 30.0])         # zero width: no samples
    dy = torch.randn(9, 6, 7, 7, generator=g)
    for dt, tol in ((torch.float32, 1e-5), (torch.float64, 1e-5)):   # sample positions up to 2^5 carry fp32 roundings of 2^-19
        a = feat.clone().requires_grad_(True)
        b = feat.clone().to(dt).requires_grad_(True)
        ya = O.roi_align(a, rois, 0.25, 7)
        yb = R64.roi_align(b, rois, 0.25, 7, aligned=True, sampling_ratio=0)
        assert yb.dtype == dt
        scale = float(ya.detach().abs().max())
        assert float((ya.detach().double() - yb.detach().double()).abs().max()) <= tol * scale
        ya.backward(dy)
        yb.backward(dy.to(dt))
        assert float((a.grad.double() - b.grad.double()).abs().max()) <= tol * float(a.grad.abs().max())
    assert float(ya[1].abs().max()) == 0 and float(ya[0].abs().max()) > 0


def test_roi_pool_rounds_half_away_from_zero():
    f = _ramp()
    # scaled corners (0.5, 1.5, 2.5, 3.5) -> (1, 2, 3, 4): rows 2..4, columns 1..3 (half-to-even would give columns 0..2)
    y, a = R64.roi_pool(f, torch.tensor([[0.5, 1.5, 2.5, 3.5]]), 1.0, 1, return_argmax=True)
    assert float(y) == 35.0 and int(a) == 4 * 8 + 3
    # (-0.5, -1.5, 1.5, 0.5) -> (-1, -2, 2, 1): 4 x 4 box, rows -2..1 and columns -1..2 clipped to rows 0..1, columns 0..2
    y, a = R64.roi_pool(f, torch.tensor([[-0.5, -1.5, 1.5, 0.5]]), 1.0, 1, return_argmax=True)
    assert float(y) == 10.0 and int(a) == 1 * 8 + 2
    # the same through a scale: 2 * 0.25 = 0.5 -> 1, 10 * 0.25 = 2.5 -> 3
    y = R64.roi_pool(f, torch.tensor([[2.0, 2.0, 10.0, 10.0]]), 0.25, 1)
    assert float(y) == 3 * 8 + 3


def test_roi_pool_clipped_box_has_empty_bins():
    f = _ramp()
    # columns 5..11 of an 8-wide map, rows 0..6, P = 7: bins of one pixel; bin columns 3..6 lie outside
    y, a = R64.roi_pool(f, torch.tensor([[5.0, 0.0, 11.0, 6.0]]), 1.0, 7, return_argmax=True)
    exp = torch.zeros(7, 7)
    arg = torch.full((7, 7), -1, dtype=torch.long)
    for ph in range(7):
        for pw in range(3):
            exp[ph, pw] = 8 * ph + 5 + pw
            arg[ph, pw] = 8 * ph + 5 + pw
    assert torch.equal(y[0, 0], exp) and torch.equal(a[0, 0], arg)
    # wholly outside: every bin empty
    y, a = R64.roi_pool(f, torch.tensor([[20.0, 20.0, 30.0, 30.0]]), 1.0, 7, return_argmax=True)
    assert float(y.abs().max()) == 0 and bool((a == -1).all())


def test_roi_pool_constant_patch_takes_the_first_pixel():
    f = torch.full((1, 8, 8), 2.0)
    y, a = R64.roi_pool(f, torch.tensor([[1.0, 1.0, 4.0, 4.0]]), 1.0, 2, return_argmax=True)   # 4 x 4 box, bins of 2 x 2 pixels
    assert torch.equal(y[0, 0], torch.full((2, 2), 2.0))
    assert a[0, 0].tolist() == [[1 * 8 + 1, 1 * 8 + 3], [3 * 8 + 1, 3 * 8 + 3]]


def test_roi_pool_narrow_box_overlapping_bins_share_an_argmax():
    """3 pixels wide at P = 7: bin = float(3 / 7), column windows [0,1) [0,1) [0,2) [1,2) [1,3) [2,3) [2,3) from column 2; the middle
    column holds the row's maximum, so it is the argmax of bins 2, 3 and 4 and collects three gradients"""
    col = torch.tensor([0.0, 0.0, 1.0, 5.0, 2.0, 0.0, 0.0, 0.0])
    f = (10.0 * torch.arange(8.0)[:, None] + col[None, :]).view(1, 8, 8).double().requires_grad_(True)
    y, a = R64.roi_pool(f, torch.tensor([[2.0, 0.0, 4.0, 6.0]]), 1.0, 7, return_argmax=True)
    cols = [2, 2, 3, 3, 3, 4, 4]
    for ph in range(7):
        assert a[0, 0, ph].tolist() == [8 * ph + c for c in cols]
        assert y[0, 0, ph].tolist() == [10.0 * ph + float(col[c]) for c in cols]
    y.sum().backward()
    exp = torch.zeros(8, 8, dtype=torch.float64)
    exp[:7, 2], exp[:7, 3], exp[:7, 4] = 2.0, 3.0, 2.0
    assert torch.equal(f.grad[0], exp)


def test_roi_align_not_aligned_floors_a_zero_width_box_at_one_pixel():
    f = torch.arange(8.0).view(1, 1, 8).expand(1, 8, 8).contiguous()      # feat[y, x] = x
    roi = torch.tensor([[3.0, 1.0, 3.0, 5.0]])
    # width 0 -> 1: bins of half a pixel, one sample each at x = 3.25 and 3.75; height 4: two samples per bin, all inside
    y = R64.roi_align(f, roi, 1.0, 2, aligned=False, sampling_ratio=0)
    assert torch.equal(y[0, 0], torch.tensor([[3.25, 3.75], [3.25, 3.75]]))
    # a fixed ratio of 2: samples at 3.125, 3.375 | 3.625, 3.875 - the same means on a linear ramp
    y = R64.roi_align(f, roi, 1.0, 2, aligned=False, sampling_ratio=2)
    assert torch.equal(y[0, 0], torch.tensor([[3.25, 3.75], [3.25, 3.75]]))
    # aligned, adaptive: width 0 gives a grid of 0 samples
    y = R64.roi_align(f, roi, 1.0, 2, aligned=True, sampling_ratio=0)
    assert float(y.abs().max()) == 0
    # aligned with a fixed ratio samples the zero-width box on the line x = 2.5
    y = R64.roi_align(f, roi, 1.0, 2, aligned=True, sampling_ratio=2)
    assert torch.equal(y[0, 0], torch.full((2, 2), 2.5))


def test_roi_pooler_assigns_levels_and_skips_invalid_slots():
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(2, 3, h, w, generator=g) for h, w in ((24, 32), (12, 16), (6, 8), (3, 4))]
    rois = torch.tensor([[10.0, 10.0, 40.0, 30.0], [-20.0, -20.0, 140.0, 110.0], [-60.0, -60.0, 200.0, 170.0], [-200.0, -150.0, 330.0, 250.0]])
    assert R64.assign_levels(rois).tolist() == [0, 1, 2, 3]
    batch = torch.tensor([0, 1, 0, 1])
    valid = torch.tensor([1, 1, 0, 1])
    y, a = R64.roi_pooler(feats, rois, batch, 5, "ROIPool", roi_valid=valid, return_argmax=True)
    assert float(y[2].abs().max()) == 0 and bool((a[2] == -1).all())
    assert torch.equal(y[1], R64.roi_pool(feats[1][1], rois[1:2], 1 / 8, 5)[0])
    y = R64.roi_pooler(feats, rois, batch, 5, "ROIAlign", 2, roi_valid=valid)
    assert torch.equal(y[3], R64.roi_align(feats[3][1], rois[3:4], 1 / 32, 5, False, 2)[0])


def _cfg(opts):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", "cpu"] + list(opts))


@pytest.mark.parametrize("opts,expect", [
    (["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIPool"], ("ROIPool", 0)),
    (["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlign"], ("ROIAlign", 0)),
    (["MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2], ("ROIAlignV2", 2)),
    (["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlign", "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2], ("ROIAlign", 2)),
    ([], ("ROIAlignV2", 0)),
])
def test_build_model_accepts_the_pooler_types(opts, expect):
    from ubteacher.modeling import build_model
    torch.manual_seed(0)
    model = build_model(_cfg(opts))
    assert (model.roi_heads.pooler_type, model.roi_heads.sampling_ratio) == expect


@pytest.mark.parametrize("opts,key", [
    (["MODEL.ROI_BOX_HEAD.POOLER_TYPE", "ROIAlignRotated"], "MODEL.ROI_BOX_HEAD.POOLER_TYPE"),
    (["MODEL.ROI_BOX_HEAD.NUM_CONV", 1], "MODEL.ROI_BOX_HEAD.NUM_CONV"),
])
def test_build_model_names_the_unbuilt_box_head_key(opts, key):
    from ubteacher.modeling import build_model
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        build_model(_cfg(opts))
