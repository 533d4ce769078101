"""The HIP ROI pooler in every built mode (POOLER_TYPE "ROIAlignV2" / "ROIAlign" with POOLER_SAMPLING_RATIO 0 or fixed, "ROIPool") against
the fp64 restatement tests/roi_pooler_ref64.py: forward, both backward forms, 16-bit I/O of both library builds, the two forward
kernels against each other, and whole Faster-RCNN steps against the oracle with its `roi_align` swapped for the restatement.
Bounds are those of the default mode's tests in tests/test_rcnn_kernels_gpu.py and tests/test_backbone_variants_gpu.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import utv2_oracle as O
from tests import roi_pooler_ref64 as R64
from tests.utv2_testutil import FixedLoader, cpu_state, make_batch, rcnn_tune

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24, 32), (12, 16), (6, 8), (3, 4))          # the four levels of a 96 x 128 image
SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
N, P_SLOTS = 2, 16
ALIGN_MODES = [("ROIAlignV2", 0), ("ROIAlignV2", 2), ("ROIAlign", 0), ("ROIAlign", 1), ("ROIAlign", 2)]
NEW_ALIGN_MODES = ALIGN_MODES[1:]
MODES = ALIGN_MODES + [("ROIPool", 0)]
SIZES = [(16, 7), (40, 5)]                              # (channels, pooler resolution): 40 is no multiple of 32
mode_id = lambda m: "%s-%d" % m  # noqa: E731


def make_rois():
    """[N * 16, 4] boxes image by image and their valid flags: the hand-built ones in image 0, seeded ones in image 1"""
    hand = [
        [300.0, 200.0, 340.0, 260.0],     # wholly outside the image
        [-10.0, 20.0, 14.0, 50.0],        # across the left border
        [30.0, -12.0, 70.0, 18.0],        # the top border
        [110.0, 30.0, 140.0, 70.0],       # the right border
        [40.0, 80.0, 90.0, 110.0],        # the bottom border
        [50.0, 20.0, 50.0, 60.0],         # zero width
        [-200.0, -150.0, 330.0, 250.0],   # covers the whole image, sqrt(area) >= 448: coarsest level, 16.6 x 12.5 pixels, grid >= 2 x 3
        [40.0, 30.0, 50.0, 41.0],         # 2.5 x 2.75 pixels of the finest level
        [10.0, 6.0, 30.0, 22.0],          # scaled corners 2.5, 1.5, 7.5, 5.5
        [-2.0, -6.0, 18.0, 14.0],         # scaled corners -0.5, -1.5, 4.5, 3.5
        [20.0, 10.0, 90.0, 70.0],         # twice the same box
        [20.0, 10.0, 90.0, 70.0],
        [-20.0, -20.0, 140.0, 110.0],     # sqrt(area) in [112, 224): the second level
        [-60.0, -60.0, 200.0, 170.0],     # in [224, 448): the third level
        [5.0, 5.0, 60.0, 40.0],           # two invalid slots
        [64.0, 48.0, 100.0, 90.0],
    ]
    g = torch.Generator().manual_seed(11)
    xy = torch.rand(P_SLOTS, 2, generator=g) * torch.tensor([110.0, 80.0]) - 8.0
    wh = torch.exp(torch.rand(P_SLOTS, 2, generator=g) * 4.0 + 0.7)
    rois = torch.cat([torch.tensor(hand), torch.cat([xy, xy + wh], 1)])
    valid = torch.ones(N * P_SLOTS, dtype=torch.uint8)
    valid[14] = valid[15] = 0
    return rois, valid


@functools.lru_cache(maxsize=None)
def make_case(C, ties=False):
    """features NCHW fp32 on the CPU (ties: quantised to the integers 0..3), rois, image index, valid flags, and a dy per resolution"""
    g = torch.Generator().manual_seed(100 + C)
    if ties:
        feats = [torch.randint(0, 4, (N, C, h, w), generator=g).float() for h, w in SHAPES]
    else:
        feats = [torch.randn(N, C, h, w, generator=g) for h, w in SHAPES]
    rois, valid = make_rois()
    batch = torch.arange(N, dtype=torch.int32).repeat_interleave(P_SLOTS)
    dys = {p: torch.randn(N * P_SLOTS, C, p, p, generator=g) for p in (5, 7)}
    return feats, rois, batch, valid, dys


def nhwc(fs, dtype=torch.float32):
    return [f.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV) for f in fs]


@functools.lru_cache(maxsize=None)
def reference(mode, C, P, ties=False, dtype=torch.float64, rounded=None):
    """the restatement's output and level gradients, computed once per case; rounded: features and dy rounded to this 16-bit type first"""
    feats, rois, batch, valid, dys = make_case(C, ties)
    rnd = (lambda t: t.to(rounded).float()) if rounded is not None else (lambda t: t)
    fr = [rnd(f).to(dtype).clone().requires_grad_(True) for f in feats]
    out = R64.roi_pooler(fr, rois, batch, P, mode[0], mode[1], SCALES, 2, valid, return_argmax=mode[0] == "ROIPool")
    y, arg = out if mode[0] == "ROIPool" else (out, None)
    y.backward(rnd(dys[P]).to(dtype))
    return y.detach(), arg, [f.grad if f.grad is not None else torch.zeros_like(f) for f in fr]


def close(a, b, rtol, atol):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (a.shape, b.shape)
    print("max |a - b| %.3e at scale %.3e" % (float(np.abs(a - b).max()), float(np.abs(b).max())))
    assert np.allclose(a, b, rtol=rtol, atol=atol), (float(np.abs(a - b).max()), float(np.abs(b).max()))


def test_case_covers_every_level_and_an_adaptive_grid_of_three():
    rois, valid = make_rois()
    lv = R64.assign_levels(rois)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3] and int(lv[6]) == 3
    h, w = float(rois[6, 3] - rois[6, 1]) / 32, float(rois[6, 2] - rois[6, 0]) / 32
    assert int(np.ceil(h / 5)) >= 3 and int(np.ceil(w / 7)) >= 3


@pytest.mark.parametrize("C,P", SIZES)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_fwd_bwd_vs_fp64_restatement(mode, C, P):
    """fp32 kernels against the fp64 restatement on the same fp32 values, the bounds of test_roi_align_fwd_bwd_vs_oracle: output
    rtol 1e-4 / atol 1e-5, gradients rtol 1e-3 / atol 1e-5 - through autograd in both backward forms (ROIs image by image: the tiled
    gather; no layout promise: the atomic scatter).  Invalid slots: zero output."""
    from ubteacher import ops
    feats, rois, batch, valid, dys = make_case(C)
    ref_y, _, ref_g = reference(mode, C, P)
    dy = dys[P].permute(0, 2, 3, 1).contiguous().to(DEV)
    for per_image in (P_SLOTS, 0):
        fh = [f.requires_grad_(True) for f in nhwc(feats)]
        y = ops.roi_align(fh, SCALES, 2, rois.to(DEV), batch.to(DEV), valid.to(DEV), P, rois_per_image=per_image, pooler=mode[0],
                          sampling_ratio=mode[1])
        close(y.permute(0, 3, 1, 2), ref_y, rtol=1e-4, atol=1e-5)
        assert float(y.detach()[14:16].abs().max()) == 0
        y.backward(dy)
        for a, b in zip(fh, ref_g):
            close(a.grad.permute(0, 3, 1, 2), b, rtol=1e-3, atol=1e-5)
    assert all(float(b.abs().max()) > 0 for b in ref_g)


@pytest.mark.parametrize("ties", [False, True], ids=["randn", "ties"])
@pytest.mark.parametrize("C,P", SIZES)
def test_roi_pool_output_and_argmax_are_exact(C, P, ties):
    """RoIPool selects, it does not compute: output and argmax equal the fp32 restatement's exactly, also where equal values compete
    (features quantised to 0..3: the first maximum in row-major order wins); the gradient within the RoIAlign backward bound"""
    from ubteacher import hip
    feats, rois, batch, valid, dys = make_case(C, ties)
    ref_y, ref_a, _ = reference(("ROIPool", 0), C, P, ties, torch.float32)
    y, a = hip.roi_align_fwd(nhwc(feats), SCALES, 2, rois.to(DEV), batch.to(DEV), valid.to(DEV), P, pooler="ROIPool")
    assert a.dtype == torch.int32
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), ref_y)
    assert torch.equal(a.permute(0, 3, 1, 2).cpu().long(), ref_a)
    assert bool((ref_a == -1).any()) and bool((ref_a >= 0).any())
    _, _, ref_g = reference(("ROIPool", 0), C, P, ties)
    shapes = [(N, h, w, C) for h, w in SHAPES]
    dy = dys[P].permute(0, 2, 3, 1).contiguous().to(DEV)
    got = hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, rois.to(DEV), valid.to(DEV), dy, P_SLOTS, pooler="ROIPool", argmax=a)
    for g, b in zip(got, ref_g):
        close(g.permute(0, 3, 1, 2), b, rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_16_bit_io(mode, kind):
    """16-bit features / output / dy in both library builds, in the manner of test_roi_align_bf16_io: the inputs are rounded to the 16-bit
    type once.  Forward: the fp32 kernel's result on those values, rounded once - exactly; and against the restatement on those values
    within the fp32 forward bound plus one rounding of the result (relative 2^-8 in bf16, 2^-11 in fp16).  RoIPool's forward is exact
    against the restatement.  Backward: the gather writes the fp32 gradient of the rounded dy, rounded once; the scatter adds the same
    fp32 values (<= 1e-4 of the map's scale: the order of the atomics differs between launches)."""
    from ubteacher import hip
    C, P = 40, 7
    h16 = torch.bfloat16 if kind == "bf16" else torch.float16
    eps = 2.0 ** -8 if kind == "bf16" else 2.0 ** -11
    feats, rois, batch, valid, dys = make_case(C)
    ref_y, ref_a, _ = reference(mode, C, P, False, torch.float64, h16)
    kw = dict(pooler=mode[0], sampling_ratio=mode[1])
    r, b, v = rois.to(DEV), batch.to(DEV), valid.to(DEV)
    shapes = [(N, h, w, C) for h, w in SHAPES]
    hip.set_h16(kind)
    try:
        f16 = nhwc(feats, h16)
        f32 = [f.float() for f in f16]
        y16, y32 = hip.roi_align_fwd(f16, SCALES, 2, r, b, v, P, **kw), hip.roi_align_fwd(f32, SCALES, 2, r, b, v, P, **kw)
        a16 = None
        if mode[0] == "ROIPool":
            (y16, a16), (y32, a32) = y16, y32
            assert torch.equal(a16, a32) and torch.equal(a16.permute(0, 3, 1, 2).cpu().long(), ref_a)
            assert torch.equal(y16.permute(0, 3, 1, 2).float().cpu().double(), ref_y)
        assert y16.dtype == h16 and torch.equal(y16, y32.to(h16))
        got, ref = y16.permute(0, 3, 1, 2).float().cpu().double(), ref_y
        err = (got - ref).abs()
        print("16-bit forward: max error %.3e at scale %.3e" % (float(err.max()), float(ref.abs().max())))
        assert bool((err <= eps * ref.abs() + 1e-4 * ref.abs() + 1e-5).all())
        dy16 = dys[P].permute(0, 2, 3, 1).contiguous().to(h16).to(DEV)
        g32 = hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, r, v, dy16.float(), P_SLOTS, argmax=a16, **kw)
        g16 = hip.roi_align_bwd_tiled(shapes, h16, SCALES, 2, r, v, dy16, P_SLOTS, argmax=a16, **kw)
        for x, z in zip(g16, g32):
            assert x.dtype == h16 and torch.equal(x, z.to(h16))
        s32 = [torch.zeros(s, device=DEV) for s in shapes]
        s16 = [torch.zeros(s, device=DEV) for s in shapes]
        hip.roi_align_bwd(s32, SCALES, 2, r, b, v, dy16.float(), argmax=a16, **kw)
        hip.roi_align_bwd(s16, SCALES, 2, r, b, v, dy16, argmax=a16, **kw)
        for x, z in zip(s16, s32):
            assert float((x - z).abs().max()) <= 1e-4 * float(z.abs().max() + 1e-6)
    finally:
        hip.set_h16("bf16")


_FWD_SCRIPT = """
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
from ubteacher import hip
from tests.test_roi_pooler_gpu import NEW_ALIGN_MODES, SCALES, SIZES, make_case, nhwc
out = {}
for C, P in SIZES:
    feats, rois, batch, valid, dys = make_case(C)
    r, b, v = rois.cuda(), batch.cuda(), valid.cuda()
    for mode in NEW_ALIGN_MODES:
        for name, dt in (("f32", torch.float32), ("h16", torch.bfloat16)):
            out["%%s-%%d-%%d-%%d-%%s" %% (mode[0], mode[1], C, P, name)] = hip.roi_align_fwd(
                nhwc(feats, dt), SCALES, 2, r, b, v, P, pooler=mode[0], sampling_ratio=mode[1]).cpu()
torch.save(out, sys.argv[1])
"""


def test_per_roi_forward_kernel_equals_per_bin_kernel_bit_for_bit(tmp_path):
    """The forward runs one workgroup per ROI (tap tables in LDS); UTV2_ROI_FWD_PER_ROI=0 keeps one wave per (roi, bin).  Both build the
    same tables from the same sample positions and add the taps in the same order, so in every new RoIAlign mode the outputs are
    bit-identical (the switch is read once per process: subprocesses, as in test_roi_align_fwd_per_roi_kernel_matches_per_bin_kernel)."""
    code = _FWD_SCRIPT % (os.path.join(ROOT, "unbiased-teacher-v2_amd"), ROOT)
    outs = {}
    for flag in ("0", "1"):
        path = str(tmp_path / ("roi%s.pt" % flag))
        e = dict(os.environ); e["UTV2_ROI_FWD_PER_ROI"] = flag
        r = subprocess.run([sys.executable, "-c", code, path], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[flag] = torch.load(path)
    assert len(outs["0"]) == len(NEW_ALIGN_MODES) * len(SIZES) * 2
    for k in outs["0"]:
        a, b = outs["0"][k], outs["1"][k]
        assert torch.isfinite(b.float()).all() and float(b.float().abs().max()) > 0, k
        assert torch.equal(a, b), (k, float((a.float() - b.float()).abs().max()))


@pytest.mark.parametrize("C,P", SIZES)
@pytest.mark.parametrize("mode", MODES, ids=mode_id)
def test_tiled_gather_equals_scatter_and_is_deterministic(mode, C, P):
    """the deterministic gather against the atomic scatter within the bound of
    test_roi_align_bwd_tiled_gather_equals_scatter_and_is_deterministic (2e-5 of the map's scale), bit-identical between two runs; a dy
    that is non-zero on the invalid slots only leaves every gradient map exactly zero"""
    from ubteacher import hip
    feats, rois, batch, valid, dys = make_case(C)
    r, b, v = rois.to(DEV), batch.to(DEV), valid.to(DEV)
    kw = dict(pooler=mode[0], sampling_ratio=mode[1])
    if mode[0] == "ROIPool":
        kw["argmax"] = hip.roi_align_fwd(nhwc(feats), SCALES, 2, r, b, v, P, pooler="ROIPool")[1]
    shapes = [(N, h, w, C) for h, w in SHAPES]
    dy = dys[P].permute(0, 2, 3, 1).contiguous().to(DEV)
    ref = [torch.zeros(s, device=DEV) for s in shapes]
    hip.roi_align_bwd(ref, SCALES, 2, r, b, v, dy, **kw)
    got = hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, r, v, dy, P_SLOTS, **kw)
    again = hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, r, v, dy, P_SLOTS, **kw)
    for x, y, z in zip(got, ref, again):
        print("gather - scatter: %.3e at scale %.3e" % (float((x - y).abs().max()), float(y.abs().max())))
        assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max() + 1e-6)
        assert torch.equal(x, z)
    assert all(float(y.abs().max()) > 0 for y in ref)
    dy_inv = torch.zeros_like(dy)
    dy_inv[14:16] = dy[14:16]
    scat = [torch.zeros(s, device=DEV) for s in shapes]
    hip.roi_align_bwd(scat, SCALES, 2, r, b, v, dy_inv, **kw)
    for x in hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, r, v, dy_inv, P_SLOTS, **kw) + scat:
        assert float(x.abs().max()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# bins wider than the tap table: the sample-by-sample path of the forward kernels and of the atomic scatter
ROI_MAXT = 18                                           # csrc/rcnn.hip: taps per axis the table path keeps
LONG_SLOTS = 6
LONG_MODES = [("ROIAlignV2", 0), ("ROIAlign", 0), ("ROIAlignV2", 2)]
LONG_C = 16


@functools.lru_cache(maxsize=None)
def make_long_case():
    """features NCHW fp32 on the CPU, long thin boxes of the finest level (and one ordinary box, one invalid slot) image by image,
    image index, valid flags, a dy for resolution 7"""
    g = torch.Generator().manual_seed(177)
    feats = [torch.randn(N, LONG_C, h, w, generator=g) for h, w in SHAPES]
    boxes = [
        [40.0, 0.0, 46.0, 520.0],         # bins of 18.6 rows at resolution 7
        [40.0, 0.0, 46.0, 600.0],         # of 18.75 rows at resolution 8
        [0.0, 40.0, 1000.0, 46.0],        # at sampling ratio 2 the two samples of a bin lie about 18 columns apart
        [0.0, 40.0, 1100.0, 46.0],        # about 20 (resolution 7) and 17 (resolution 8) columns apart
        [20.0, 10.0, 90.0, 70.0],         # an ordinary box: the table path next to the others
        [10.0, 0.0, 16.0, 560.0],         # the invalid slot
    ]
    rois = torch.cat([torch.tensor(boxes), torch.tensor(boxes) + torch.tensor([3.25, 1.5, 3.25, 1.5])])
    valid = torch.ones(N * LONG_SLOTS, dtype=torch.uint8)
    valid[LONG_SLOTS - 1] = valid[2 * LONG_SLOTS - 1] = 0
    batch = torch.arange(N, dtype=torch.int32).repeat_interleave(LONG_SLOTS)
    dy = torch.randn(N * LONG_SLOTS, LONG_C, 7, 7, generator=g)
    return feats, rois, batch, valid, dy


@functools.lru_cache(maxsize=None)
def long_reference(mode, P):
    """the fp64 restatement's output of the long-box case and, at resolution 7, its level gradients; computed once"""
    feats, rois, batch, valid, dy = make_long_case()
    fr = [f.double().clone().requires_grad_(P == 7) for f in feats]
    y = R64.roi_pooler(fr, rois, batch, P, mode[0], mode[1], SCALES, 2, valid)
    if P != 7:
        return y.detach(), None
    y.backward(dy.double())
    return y.detach(), [f.grad if f.grad is not None else torch.zeros_like(f) for f in fr]


def widest_bin_span(rois, valid, mode, P):
    """per ROI the largest number of pixel rows or columns of its level that the counted samples of one of its bins put weight on
    (0: none, or an invalid slot) - the restatement's geometry and tap rule in fp64"""
    lv = R64.assign_levels(rois)
    off = 0.5 if mode[0] == "ROIAlignV2" else 0.0
    spans = []
    for r in range(rois.shape[0]):
        best = 0
        if bool(valid[r]):
            (h, w), sc = SHAPES[int(lv[r])], SCALES[int(lv[r])]
            b = rois[r].double() * sc - off
            for lo, hi, size in ((b[1], b[3], h), (b[0], b[2], w)):
                side = float(hi - lo) if off else max(float(hi - lo), 1.0)
                g = mode[1] if mode[1] > 0 else int(np.ceil(side / P))
                for p in range(P if g > 0 else 0):
                    v = lo + p * side / P + (torch.arange(g, dtype=torch.float64) + 0.5) * (side / P) / g
                    ok, lo_px, hi_px, _ = R64._axis(v, size)
                    if bool(ok.any()):
                        best = max(best, int(hi_px[ok].max() - lo_px[ok].min()) + 1)
        spans.append(best)
    return spans


@pytest.mark.parametrize("P", [7, 8])
@pytest.mark.parametrize("mode", LONG_MODES, ids=mode_id)
def test_long_case_has_bins_wider_than_the_tap_table(mode, P):
    """no GPU needed: in every mode and at both resolutions a valid ROI of the long-box case has a bin whose samples touch more than
    ROI_MAXT pixels of an axis (the kernels then leave the table path), and the ordinary box has none"""
    _, rois, _, valid, _ = make_long_case()
    spans = widest_bin_span(rois, valid, mode, P)
    print("widest bin per ROI, %s at resolution %d: %s" % (mode_id(mode), P, spans))
    assert max(spans) > ROI_MAXT
    assert 0 < spans[4] <= ROI_MAXT and spans[LONG_SLOTS - 1] == 0
    assert set(R64.assign_levels(rois[:4]).tolist()) == {0}


@pytest.mark.parametrize("mode", LONG_MODES, ids=mode_id)
def test_bins_wider_than_the_tap_table_vs_fp64_restatement(mode):
    """Bins of more than ROI_MAXT pixels take the sample-by-sample path: the per-ROI forward's fall-back at resolution 7, the
    per-(roi, bin) forward at resolution 8 (the per-ROI kernel stops at 7), the atomic scatter at 7; the tiled gather sums sample by
    sample at any bin size.  Bounds of test_fwd_bwd_vs_fp64_restatement: output rtol 1e-4 / atol 1e-5, gradients rtol 1e-3 / atol 1e-5."""
    from ubteacher import hip
    feats, rois, batch, valid, dy = make_long_case()
    for P in (7, 8):
        assert max(widest_bin_span(rois, valid, mode, P)) > ROI_MAXT
    kw = dict(pooler=mode[0], sampling_ratio=mode[1])
    r, b, v = rois.to(DEV), batch.to(DEV), valid.to(DEV)
    for P in (7, 8):
        y = hip.roi_align_fwd(nhwc(feats), SCALES, 2, r, b, v, P, **kw)
        close(y.permute(0, 3, 1, 2), long_reference(mode, P)[0], rtol=1e-4, atol=1e-5)
        assert float(y[LONG_SLOTS - 1].abs().max()) == 0 and float(y[0].abs().max()) > 0
    ref_g = long_reference(mode, 7)[1]
    shapes = [(N, h, w, LONG_C) for h, w in SHAPES]
    dyh = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
    scat = [torch.zeros(s, device=DEV) for s in shapes]
    hip.roi_align_bwd(scat, SCALES, 2, r, b, v, dyh, **kw)
    for got in (hip.roi_align_bwd_tiled(shapes, torch.float32, SCALES, 2, r, v, dyh, LONG_SLOTS, **kw), scat):
        for a, g in zip(got, ref_g):
            close(a.permute(0, 3, 1, 2), g, rtol=1e-3, atol=1e-5)
    assert float(ref_g[0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# whole steps
H, W = 96, 128
STEP_MODES = [("ROIAlign", 2), ("ROIPool", 0)]


def _step_cfg(mode, amp=False):
    from ubteacher.presets import get_config
    cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "MODEL.DEVICE", "cuda", "MODEL.ROI_BOX_HEAD.POOLER_TYPE", mode[0],
                                 "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", mode[1]])
    cfg.SOLVER.AMP.ENABLED = amp
    return cfg


def _oracle_checks(cfg, nb, orac, sd_s, sd_t, rec, rpn_keys, roi_keys, tr, mean, pstd):
    """tests/test_backbone_variants_gpu.py::_rcnn_oracle_checks - the same checks and tolerances - with the pseudo-label SELECTION
    decoupled the way tests/test_rcnn_step_gpu.py::test_rcnn_step_fp32_tight_with_the_product_pseudo_boxes decouples it: the oracle's
    own teacher (with the restated pooler) must give the product's pseudo boxes - the same count per image, as there, and here also the
    same boxes, classes and scores to 1e-3 pixels / 1e-4 - and the oracle's student half is then handed the product's boxes.
    Why: the RPN's pseudo losses sum over anchors the Matcher's exact-equality low-quality rule makes positive, and that rule breaks
    its ties differently for pseudo boxes that differ in the last fp32 bits.  This set-up (R-50, 1 + 1 images, the threshold in the
    widest gap around the median score) keeps 48 - 59 pseudo boxes, and with the oracle's own boxes the comparison measures that rule,
    not the pooler - measured on an MI355X, |product - oracle| / oracle of loss_rpn_loc_pseudo, pseudo boxes agreeing to 6e-5 pixels
    in every row: default pooler ("ROIAlignV2", 0) 8.0e-2, ("ROIAlign", 2) 3.2e-2, ("ROIPool", 0) 1.3e-2, while every loss the pooler
    feeds (loss_cls, loss_box_reg and their pseudo forms) agrees to 6e-4 or better in all three."""
    post = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN

    def compact_roi(keys, nprops, ngts):
        return [torch.cat((keys[i, :nprops[i]], keys[i, post:post + ngts[i]])) for i in range(keys.shape[0])]

    t_sd = O.ema_update(sd_s, sd_t, cfg.SEMISUPNET.EMA_KEEP_RATE)
    gl = tr._last_pseudo
    with torch.no_grad():
        own, _ = O.rcnn_teacher(t_sd, [d["image"] for d in orac[3]], mean, pstd, thr=cfg.SEMISUPNET.BBOX_THRESHOLD)
    assert sum(len(p["boxes"]) for p in own) > 0, "test setup: teacher produced no pseudo boxes"
    pseudo = []
    for i, p in enumerate(own):
        m = gl["valid"][i].bool()
        assert int(m.sum()) == len(p["boxes"])
        q = dict(boxes=gl["boxes"][i][m].cpu(), classes=gl["classes"][i][m].long().cpu(), scores=gl["scores"][i][m].cpu(),
                 pred_boxes_std=gl["pred_boxes_std"][i][m].cpu())
        print("pseudo boxes: %d, max |product - oracle| %.3e pixels" % (len(p["boxes"]), float((q["boxes"] - p["boxes"]).abs().max())))
        assert float((q["boxes"] - p["boxes"]).abs().max()) <= 1e-3 and torch.equal(q["classes"], p["classes"].long())
        assert float((q["scores"] - p["scores"]).abs().max()) <= 1e-4
        pseudo.append(q)
    with torch.no_grad():
        _, props_sup, _ = O.rcnn_student_losses(sd_s, [d["image"] for d in orac[0] + orac[1]], [d["gt"] for d in orac[0] + orac[1]],
                                                rpn_keys[0], [torch.zeros(2000)] * (2 * nb), False, mean, pstd)
        _, props_uns, _ = O.rcnn_student_losses(sd_s, [d["image"] for d in orac[2]], pseudo, rpn_keys[1], [torch.zeros(2000)] * nb,
                                                True, mean, pstd)
    keys = dict(rpn_sup=rpn_keys[0], rpn_unsup=rpn_keys[1],
                roi_sup=compact_roi(roi_keys[0], [len(p["boxes"]) for p in props_sup], [len(d["gt"]["boxes"]) for d in orac[0] + orac[1]]),
                roi_unsup=compact_roi(roi_keys[1], [len(p["boxes"]) for p in props_uns], [len(p["boxes"]) for p in pseudo]))
    rec_o, new_s, new_t, grads, _ = O.rcnn_semisup_step(sd_s, sd_t, orac, keys, keep_rate=cfg.SEMISUPNET.EMA_KEEP_RATE,
                                                       lam_u=cfg.SEMISUPNET.UNSUP_LOSS_WEIGHT, lam_r=cfg.SEMISUPNET.UNSUP_REG_LOSS_WEIGHT,
                                                       thr=cfg.SEMISUPNET.BBOX_THRESHOLD, lr=0.01, mean=mean, pix_std=pstd,
                                                       pseudo_override=pseudo)
    for k, v in rec_o.items():
        assert k in rec, k
        print("%-24s product %.7f oracle %.7f" % (k, rec[k], v))
        tol = 2e-2 if k == "loss_rpn_loc_pseudo" else 5e-3 if k == "loss_rpn_cls_pseudo" else 1e-3
        assert abs(rec[k] - v) <= tol * max(abs(v), 1e-6), (k, rec[k], v)
    assert rec_o["loss_box_reg_pseudo"] > 0 and rec_o["loss_rpn_cls_pseudo"] > 0 and rec_o["loss_rpn_loc_pseudo"] > 0
    t_after, s_after = cpu_state(tr.model_teacher), cpu_state(tr.model)
    for k in new_t:
        assert torch.equal(t_after[k], new_t[k]), k
    for k in new_s:
        err = float((s_after[k].double() - new_s[k].double()).abs().max())
        upd = float((new_s[k].double() - sd_s[k].double()).abs().max())
        assert err <= 1e-4 * float(new_s[k].abs().max()) + 4e-2 * upd + 1e-12, k


@pytest.mark.parametrize("mode", STEP_MODES, ids=mode_id)
def test_rcnn_step_parity(mode, monkeypatch):
    """One Faster-RCNN semi-supervised step (one labeled, one unlabeled image) against the oracle step whose `roi_align` is the
    restatement of the configured pooler (oracle.FAST_ROI_ALIGN stays False, so the patched global is the one its ROI pooler calls):
    the checks and tolerances of tests/test_backbone_variants_gpu.py::test_rcnn_step_parity - losses, pseudo boxes, teacher EMA
    exact, student update (see _oracle_checks)."""
    from tests.test_backbone_variants_gpu import _gap_threshold
    from ubteacher.engine import UBRCNNTeacherTrainer
    assert O.FAST_ROI_ALIGN[0] is False
    monkeypatch.setattr(O, "roi_align", R64.one_level(*mode))
    nb = 1
    cfg = _step_cfg(mode)
    torch.manual_seed(0)
    prod, orac = make_batch(31, nb, nb, H, W, "cuda")
    tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    assert (tr.model.roi_heads.pooler_type, tr.model_teacher.roi_heads.sampling_ratio) == mode
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1)
    pstd = torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
    sd_s = rcnn_tune(cpu_state(tr.model), [d["image"] for d in orac[3]], mean, pstd)
    sd_t = dict(sd_s)
    sd_t["roi_heads.box_predictor.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    with torch.no_grad():
        dets, _ = O.rcnn_teacher(O.ema_update(sd_s, sd_t, cfg.SEMISUPNET.EMA_KEEP_RATE), [d["image"] for d in orac[3]], mean, pstd, thr=-1.0)
    cfg.SEMISUPNET.BBOX_THRESHOLD = _gap_threshold(torch.cat([d["scores"] for d in dets]))
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    g = torch.Generator().manual_seed(99)
    rpn_keys, roi_keys = [], []

    def rpn_src(n, m, device):
        k = torch.rand(n, m, generator=g)
        rpn_keys.append(k)
        return k.to(device)

    def roi_src(n, m, device):
        k = torch.rand(n, m, generator=g)
        roi_keys.append(k)
        return k.to(device)

    tr.model.proposal_generator.sample_keys = rpn_src
    tr.model.roi_heads.sample_keys = roi_src
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    _oracle_checks(cfg, nb, orac, sd_s, sd_t, rec, rpn_keys, roi_keys, tr, mean, pstd)


_AMP_LOSSES = {}


def _amp_and_fp32_losses(mode, spy):
    """losses of the fp32 and of the fp16-AMP step of one pooler mode on the same batch, weights and sampling keys (cached per mode)"""
    from ubteacher import ops
    from ubteacher.engine import UBRCNNTeacherTrainer
    if mode in _AMP_LOSSES:
        return _AMP_LOSSES[mode]
    recs = {}
    try:
        for amp in (False, True):
            cfg = _step_cfg(mode, amp)
            torch.manual_seed(0)
            prod, orac = make_batch(31, 1, 1, H, W, "cuda")
            tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
            assert ops.PRECISION[0] == ("fp16" if amp else "fp32")
            mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1)
            pstd = torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
            sd_s = rcnn_tune(cpu_state(tr.model), [d["image"] for d in orac[3]], mean, pstd)
            sd_t = dict(sd_s)
            sd_t["roi_heads.box_predictor.bbox_pred_std.bias"] = torch.full((4,), -3.0)
            tr.model.load_state_dict(sd_s)
            tr.model_teacher.load_state_dict(sd_t)
            tr.iter = 1
            tr.optimizer.param_groups[0]["lr"] = 0.01
            g = torch.Generator().manual_seed(99)
            src = lambda n, m, device: torch.rand(n, m, generator=g).to(device)  # noqa: E731
            tr.model.proposal_generator.sample_keys = src
            tr.model.roi_heads.sample_keys = src
            spy.clear()
            tr.run_step_full_semisup()
            rec = tr.flush_metrics()
            torch.cuda.synchronize()
            recs[amp] = {k: v for k, v in rec.items() if k.startswith("loss")}
            if amp:    # the pooler's level gradients went to the RPN conv's dgrad epilogue (FanIn), in the configured mode
                assert spy and all(s == (mode[0], mode[1], True) for s in spy), spy
    finally:
        ops.set_precision("fp32")
    _AMP_LOSSES[mode] = recs
    return recs


@pytest.mark.parametrize("mode", STEP_MODES, ids=mode_id)
def test_rcnn_fp16_amp_step_runs_the_fanin_path_and_stays_close_to_fp32(mode, monkeypatch):
    """An fp16-AMP step per mode: the pooler's backward writes its level gradients into the FanIn buffers the RPN conv's dgrad adds (it
    writes every element, so the hand-off holds for every mode), the losses are finite and deviate from the fp32 step's by no more
    than twice what the default pooler's deviate (floor 1e-3) - the rule of test_x101_fp16_step_fused_and_close_to_fp32."""
    monkeypatch.setenv("UTV2_PRECISION", "fp16")
    from ubteacher import hip
    monkeypatch.setattr(O, "roi_align", R64.one_level(*mode))      # rcnn_tune runs the oracle's forward
    spy = []
    orig = hip.roi_align_bwd_tiled

    def tiled(*a, **k):
        spy.append((k.get("pooler", "ROIAlignV2"), k.get("sampling_ratio", 0), k.get("outs") is not None))
        return orig(*a, **k)

    monkeypatch.setattr(hip, "roi_align_bwd_tiled", tiled)
    got = _amp_and_fp32_losses(mode, spy)
    monkeypatch.setattr(O, "roi_align", R64.one_level("ROIAlignV2", 0))
    base = _amp_and_fp32_losses(("ROIAlignV2", 0), spy)

    def dev(r):
        return max(abs(r[True][k] - r[False][k]) / max(abs(r[False][k]), 1e-6) for k in r[False] if abs(r[False][k]) > 1e-6)
    print("AMP deviation: %s %.3e, default pooler %.3e" % (mode_id(mode), dev(got), dev(base)))
    assert all(np.isfinite(v) for r in (got, base) for d in r.values() for v in d.values())
    assert dev(got) <= 2 * max(dev(base), 1e-3), (dev(got), dev(base))
