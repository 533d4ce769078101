"""The formulas csrc/rcnn.hip keeps in ONE helper for several kernels, on the branches no other test pins through every caller:
smooth_l1 (RPN loss and ROI box loss give the same bits for the same difference), ctr_apply_deltas (the box the RPN "giou" loss decodes
is the box rpn_decode writes), softmax_row on short rows, rpn_level_of at the level boundaries.  References: tests/rpn_ref64.py and
tests/loss_ref64.py, at the bounds tests/test_loss_kernels_fp64_gpu.py derives for these kernels."""
import math

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import rpn_ref64 as R64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
M_SOFTMAX, M_RPN = 16, 2          # the families' factors of tests/test_loss_kernels_fp64_gpu.py


def hip():
    from ubteacher import hip as H
    return H


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f32(v):
    return float(np.float32(v))


def ulp(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


# =================================================================================================
# smooth-L1: d == 0, |d| == beta, one ulp either side, at beta 0, below 1e-5 and 0.5.  The anchor / proposal IS its gt box, so every
# target is 0 in any precision and the difference is the delta itself; one element is live per launch (the other three coordinates of
# the one valid slot / foreground row are 0 and add exact zeros), so the launch's sum is that element's term.
# =================================================================================================
BOX = torch.tensor([16.0, 32.0, 48.0, 96.0])


def rpn_one(H, v, c, slot, beta):
    """RPN loss (N = 1, R = 8, npos = 4, dense): positive slot `slot` alone is valid and holds delta v in coordinate c"""
    R, npos, nneg = 8, 4, 4
    s = dict(pos_idx=torch.arange(npos)[None], neg_idx=torch.arange(npos, R)[None], pos_valid=torch.zeros((1, npos), dtype=torch.uint8),
             neg_valid=torch.zeros((1, nneg), dtype=torch.uint8), matched32=torch.zeros((1, R), dtype=torch.int32),
             has_gt=torch.ones((1, 1), dtype=torch.uint8))
    s["pos_valid"][0, slot] = 1
    dl = torch.zeros((1, R, 4))
    dl[0, slot, c] = v
    sums, _, gdl = H.rpn_loss_fwd(dev(torch.zeros((1, R))), dev(dl), None, 1, 1, R, dev(BOX.repeat(R, 1)), {k: dev(t) for k, t in s.items()},
                                  dev(BOX.view(1, 1, 4)), None, (1.0, 1.0, 1.0, 1.0), loc_mode=0, smooth_l1_beta=beta)
    return sums.cpu()[1], gdl.cpu()[0, slot, c], gdl.cpu()


def roi_one(H, v, c, row, beta, nbox):
    """ROI box loss (R = 8, mode 1, class-agnostic or K = 3 per class): row `row` alone is foreground (class 1) and holds delta v"""
    R, K = 8, 3
    cls = torch.full((R,), K, dtype=torch.int64)
    cls[row] = 1
    co = 4 * (1 if nbox > 1 else 0)
    dl = torch.zeros((R, 4 * nbox))
    dl[row, co + c] = v
    prop = BOX.repeat(R, 1)
    out, gd, _ = H.roi_box_loss(dev(dl), dev(torch.zeros((R, 4 * nbox))), dev(cls), dev(prop), dev(prop), None, K, 1, 1.0, 1.0, 62.5, 0.0, 0.0,
                                nbox=nbox, smooth_l1_beta=beta)
    return out.cpu()[0], gd.cpu()[row, co + c], gd.cpu()


@pytest.mark.parametrize("beta", [0.0, 1e-6, 0.5])
def test_smooth_l1_edges_same_bits_from_both_kernels_and_vs_fp64(beta):
    H = hip()
    b = f32(beta)
    vals = sorted({0.0, b, -b, ulp(b, True), ulp(b, False), -ulp(b, True), -ulp(b, False)})
    for i, v in enumerate(vals):
        c, j = i % 4, (i // 4) % 4
        t_rpn, g_rpn, all_rpn = rpn_one(H, v, c, j, b)
        d64 = torch.tensor([v], dtype=F64)
        term64 = R64.smooth_l1(d64, b)
        quad = b >= 1e-5 and abs(v) < b
        g64 = v / b if quad else float(np.sign(v))
        print("smooth_l1 beta %g d %.9g: term %.9g (fp64 %.17g) grad %.9g (fp64 %.17g)" % (b, v, float(t_rpn), float(term64), float(g_rpn), g64))
        for nbox in (1, 3):
            t_roi, g_roi, all_roi = roi_one(H, v, c, j, b, nbox)
            assert same_bits(t_rpn, t_roi) and same_bits(g_rpn, g_roi), (b, v, nbox)     # one function: the same bits
            assert int((all_roi != 0).sum()) == int(g64 != 0)                            # nothing but the live element
        assert int((all_rpn != 0).sum()) == int(g64 != 0)
        # the sum of one term and exact zeros: the RPN loss's forward bound (4 terms per slot, 8 tree levels)
        ref, bound = L64.sum_bound(term64, 4, 8, M_RPN)
        assert abs(float(t_rpn) - ref) <= bound, (b, v, float(t_rpn), ref, bound)
        # derivative: a sign (exact), or d / beta - ONE correctly rounded fp32 division of two fp32 numbers: half an ulp
        assert abs(float(g_rpn) - g64) <= U * abs(g64), (b, v, float(g_rpn), g64)


# =================================================================================================
# RPN "giou": torch.clamp(max=scale_clamp) on dw.  One level of 2 x 2 cells, A = 3, N = 1; weights 1, so dw / ww is the delta.
# =================================================================================================
def giou_value_f32(box, gt):
    """giou_loss_grad's value expression in fp32 on the CPU, operation by operation (IEEE +, -, *, /, min, max: the same bits)"""
    px1, py1, px2, py2 = [torch.tensor(float(v), dtype=F32) for v in box]
    gx, gy, gz, gw = [torch.tensor(float(v), dtype=F32) for v in gt]
    a1, a2 = (gz - gx) * (gw - gy), (px2 - px1) * (py2 - py1)
    ltx, lty, rbx, rby = torch.max(gx, px1), torch.max(gy, py1), torch.min(gz, px2), torch.min(gw, py2)
    zero = torch.zeros((), dtype=F32)
    I = (torch.max(rbx - ltx, zero) * torch.max(rby - lty, zero)) if (rbx > ltx and rby > lty) else zero
    Un = a1 + a2 - I
    C = (torch.max(px2, gz) - torch.min(px1, gx)) * (torch.max(py2, gw) - torch.min(py1, gy))
    eps = torch.tensor(1e-7, dtype=F32)
    return 1.0 - (I / (Un + eps) - (C - Un) / (C + eps))


def test_rpn_giou_clamp_gradient_and_the_decoded_box_is_rpn_decodes():
    H = hip()
    hw, A, N = [4], 3, 1
    R, ch = 12, 15
    clamp = R64.SCALE_CLAMP
    c32 = f32(clamp)
    anchors = torch.tensor([[5000.0 + 32 * i, 5000.0, 5016.0 + 32 * i, 5024.0] for i in range(R)])
    gt = torch.tensor([4000.0, 4500.0, 6500.0, 5600.0])
    head = torch.zeros((N * 4, ch))
    head[:, :A] = -torch.arange(R, dtype=F32).view(4, A)                     # logit order == anchor order
    dws = [c32, ulp(c32, True), 10.0, 0.5]                                     # at the bound, one ulp above, well above, uncut
    for r, dw in enumerate(dws):
        p, a = divmod(r, A)
        head[p, A + 4 * a: A + 4 * a + 4] = torch.tensor([0.25, -0.125, dw, 0.25])
    hd = dev(head)
    # the boxes rpn_decode writes for these anchors and deltas (an image nothing clips on)
    keys = H.rpn_rank_keys(hd, hw, N, A)
    top = H.topk_rows(keys, dev(torch.tensor([0, R], dtype=torch.int64)), 1, R, R)
    boxes, scores, _, keep = H.rpn_decode(top, hd, dev(anchors), dev(torch.tensor([[1e6, 1e6]])), hw, [R], N, A, (1.0, 1.0, 1.0, 1.0), clamp, 0.0)
    boxes = boxes.cpu()[0]
    assert torch.equal(scores.cpu()[0], -torch.arange(R, dtype=F32)) and bool(keep.cpu().all())
    # the fp64 reference decodes the same boxes (to fp32 rounding of exp and four multiply-adds)
    ref_boxes = R64.apply_deltas(head[:, A:].reshape(R, 4).double(), anchors.double(), (1.0, 1.0, 1.0, 1.0), c32)
    assert torch.all((boxes.double() - ref_boxes).abs() <= 8 * U * ref_boxes.abs().max())
    sbase = dict(pos_idx=torch.arange(4)[None], neg_idx=torch.arange(4, 8)[None], neg_valid=torch.zeros((1, 4), dtype=torch.uint8),
                 matched32=torch.zeros((1, R), dtype=torch.int32), has_gt=torch.ones((1, 1), dtype=torch.uint8))
    for r, dw in enumerate(dws):
        s = dict(sbase, pos_valid=torch.zeros((1, 4), dtype=torch.uint8))
        s["pos_valid"][0, r] = 1
        sums, _, gdl = H.rpn_loss_fwd(hd, hd, hw, N, A, R, dev(anchors), {k: dev(t) for k, t in s.items()}, dev(gt.view(1, 1, 4)), None,
                                      (1.0, 1.0, 1.0, 1.0), loc_mode=1, scale_clamp=clamp)
        g = gdl.cpu()[0, r]
        print("giou clamp dw %.9g: loss %.9g gdl %s" % (dw, float(sums.cpu()[1]), g.tolist()))
        assert bool(torch.isfinite(g).all())
        if dw > c32:
            assert float(g[2]) == 0.0                       # cut: exactly no gradient
        else:
            assert float(g[2]) != 0.0                       # the bound itself passes it
        # one live slot: the launch's sum is the slot's loss - and it is the GIoU loss OF THE BOX rpn_decode WROTE, bit for bit
        assert same_bits(sums.cpu()[1], giou_value_f32(boxes[r], gt)), (dw, float(sums.cpu()[1]))
    # everything from the bound up decodes the bound's box (the anchors are 32 apart, inside one binade: the shift is exact)
    step = torch.tensor([32.0, 0.0, 32.0, 0.0])
    assert torch.equal(boxes[1] - step, boxes[0]) and torch.equal(boxes[2] - 2 * step, boxes[0]) and not torch.equal(boxes[3] - 3 * step, boxes[0])


# =================================================================================================
# softmax focal on short rows: C = 1 (one lane, CE = 0), 64 (every lane once), 65 (lane 0 twice); R = 5 is no multiple of the four waves
# of a block; a skipped row (target -1) and a row with a logit of 1e4.  Forward bound: L = ceil(R / 1024) = 1, D = 4.
# =================================================================================================
@pytest.mark.parametrize("C", [1, 64, 65])
def test_softmax_focal_short_rows_vs_fp64(C):
    H = hip()
    R, gamma = 5, 1.5
    x, tgt = L64.softmax_case(R, C, 900 + C)
    assert int(tgt[1]) == -1
    x[4, C // 2] = 1e4
    l64, g64, s64 = L64.softmax_focal(x.double(), tgt, gamma)
    _, g32, _ = L64.softmax_focal(x, tgt, gamma)
    xd, td = dev(x), dev(tgt)
    f = H.softmax_focal_fwd(xd, td, gamma).cpu()
    ref, bound = L64.sum_bound(l64, 1, 4, M_SOFTMAX)
    print("softmax C%d R%d: k %.9g ref %.9g bound %.3g" % (C, R, float(f[0]), ref, bound))
    assert math.isfinite(float(f[0])) and abs(float(f[0]) - ref) <= bound
    g = H.softmax_focal_bwd(xd, td, gamma, dev(torch.tensor([0.37], dtype=F32))).cpu()
    c32 = torch.tensor(0.37, dtype=F32)
    ok, res = L64.grad_ok(g, g64[0] * c32.double(), g32[0] * c32, s64 * float(c32), M_SOFTMAX)
    print("softmax C%d R%d: worst ratio %.3f" % (C, R, res["ratio"]))
    assert ok, res
    assert torch.all(g[1] == 0)


# =================================================================================================
# level lookup: three levels of (4, 1, 1) pixels, N = 2, A = 3 - rows, candidate slots and anchors on the first element, the last one
# and both sides of each level boundary.  Every head element is distinct, deltas are 0 and anchors are small integers, so a decoded box
# IS the anchor it came from and a score IS the logit it was read from.
# =================================================================================================
def test_level_lookup_is_one_for_rank_keys_decode_and_the_head_form_loss():
    H = hip()
    hw, N, A = [4, 1, 1], 2, 3
    R, ch, rows = 18, 16, 12
    g = torch.Generator().manual_seed(5)
    head = torch.zeros((rows, ch))
    head[:, :A] = torch.randperm(rows * A, generator=g).float().view(rows, A) - 17.0       # distinct logits, both signs and a zero
    anchors = torch.tensor([[8.0 * r, 16.0, 8.0 * r + 32.0, 80.0] for r in range(R)])
    hd = dev(head)
    # rank keys, in memory order: (order-preserving logit bits + 2^31) * 2^31 + (2^31 - 1 - (pixel * A + anchor))
    keys = H.rpn_rank_keys(hd, hw, N, A).cpu()
    row0 = [0, 8, 10]
    exp = []
    for r in range(rows):
        lvl = max(i for i in range(3) if r >= row0[i])
        p = (r - row0[lvl]) % hw[lvl]
        for a in range(A):
            i = int(np.float32(float(head[r, a])).view(np.int32))
            exp.append(((i ^ ((i >> 31) & 0x7FFFFFFF)) + 2 ** 31) * 2 ** 31 + (2 ** 31 - 1 - (p * A + a)))
    assert keys.tolist() == exp
    # decode of every anchor of every (level, image) row, best logit first
    off = [0]
    for l in range(3):
        for n in range(N):
            off.append(off[-1] + hw[l] * A)
    ks = [h * A for h in hw]
    top = H.topk_rows(dev(keys), dev(torch.tensor(off, dtype=torch.int64)), 3 * N, max(ks), max(ks))
    boxes, scores, lvls, keep = [t.cpu() for t in H.rpn_decode(top, hd, dev(anchors), dev(torch.tensor([[1e4, 1e4]] * N)), hw, ks, N, A,
                                                               (1.0, 1.0, 1.0, 1.0), R64.SCALE_CLAMP, 0.0)]
    obj = torch.zeros((N, R))
    for n in range(N):
        for r in range(R):
            obj[n, r] = head.view(-1)[L64.rpn_head_offsets(hw, N, A, ch, n, r)[0]]
    a0 = [0, 12, 15, 18]
    for n in range(N):
        for l in range(3):
            order = torch.argsort(obj[n, a0[l]:a0[l + 1]], descending=True) + a0[l]
            assert torch.equal(scores[n, a0[l]:a0[l + 1]], obj[n, order]) and torch.equal(boxes[n, a0[l]:a0[l + 1]], anchors[order])
            assert torch.all(lvls[n, a0[l]:a0[l + 1]] == l)
    assert bool(keep.all())
    # the head-form loss reads what the dense form reads, and its backward writes where rpn_head_offsets says
    head[:, A:A + 4 * A] = torch.randn((rows, 4 * A), generator=g)
    hd = dev(head)
    dl = torch.zeros((N, R, 4))
    for n in range(N):
        for r in range(R):
            od = L64.rpn_head_offsets(hw, N, A, ch, n, r)[1]
            dl[n, r] = head.view(-1)[od:od + 4]
    edge = [0, 11, 12, 14, 15, 17]
    rest = [r for r in range(R) if r not in edge]
    s = dict(pos_idx=torch.tensor([edge, edge[::-1]]), neg_idx=torch.tensor([rest[:6], rest[6:]]), pos_valid=torch.ones((N, 6), dtype=torch.uint8),
             neg_valid=torch.ones((N, 6), dtype=torch.uint8), matched32=torch.zeros((N, R), dtype=torch.int32),
             has_gt=torch.ones((N, 1), dtype=torch.uint8))
    sd = {k: dev(t) for k, t in s.items()}
    gtb = torch.tensor([[[20.0, 10.0, 70.0, 90.0]], [[40.0, 20.0, 100.0, 70.0]]])
    for loc_mode in (0, 1):
        common = (N, A, R, dev(anchors), sd, dev(gtb), None, (1.0, 1.0, 1.0, 1.0))
        dense = H.rpn_loss_fwd(dev(obj), dev(dl), None, *common, loc_mode=loc_mode)
        hf = H.rpn_loss_fwd(hd, hd, hw, *common, loc_mode=loc_mode)
        for x, y in zip(dense, hf):
            assert same_bits(x, y)
        gh = torch.zeros_like(hd)
        one = dev(torch.ones(1))
        H.rpn_loss_bwd(hf[1], hf[2], one, one, hw, N, A, ch, R, sd, gh, gh)
        eh = torch.zeros(head.numel())
        gobj, gdl = hf[1].cpu(), hf[2].cpu()
        for n in range(N):
            for j in range(12):
                r = int(s["pos_idx"][n, j]) if j < 6 else int(s["neg_idx"][n, j - 6])
                oo, od = L64.rpn_head_offsets(hw, N, A, ch, n, r)
                eh[oo] = gobj[n, j]
                if j < 6:
                    eh[od:od + 4] = gdl[n, j]
        assert same_bits(gh.reshape(-1), eh)
