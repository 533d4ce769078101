"""fp64 autograd reference of the ROI box loss with MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE "giou" (the five modes of
utv2_roi_box_loss_f): roi_heads/fast_rcnn.py:938-1090 with fvcore's smooth_l1_loss(beta) where the reference passes self.smooth_l1_beta
(:966-968, :993-995, :1052-1054; nl_loss takes beta and never reads it, :1228-1292; tsbetter is called at 0.0, :1070-1075) and
fvcore's giou_loss on the boxes decoded by Box2BoxXYXYTransform.apply_deltas (:998-1002).  Mode 2, and every mode at beta < 1e-5 except
4, is tests/loss_ref64.roi_box_loss as it is; the per-class layout is the gather / scatter of tests/loss_ref64_percls.py."""
import math

import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_percls as P64

GIOU_EPS = 1e-7


def smooth_l1(x, beta):
    """fvcore.nn.smooth_l1_loss, reduction none, of x = input - target"""
    n = x.abs()
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def giou_loss(b1, b2, eps=GIOU_EPS):
    """fvcore.nn.giou_loss, reduction none: boxes [., 4] (x1, y1, x2, y2)"""
    x1, y1, x2, y2 = b1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = b2.unbind(dim=-1)
    xk1, yk1, xk2, yk2 = torch.max(x1, x1g), torch.max(y1, y1g), torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.where((yk2 > yk1) & (xk2 > xk1), (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    area_c = (torch.max(x2, x2g) - torch.min(x1, x1g)) * (torch.max(y2, y2g) - torch.min(y1, y1g))
    return 1 - (inter / (union + eps) - (area_c - union) / (area_c + eps))


def decode(d, pb, wx, wy, scale_clamp):
    """Box2BoxXYXYTransform.apply_deltas (box_regression.py:75-129): deltas in the order x1, x2, y1, y2 -> boxes x1, y1, x2, y2"""
    w, h = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
    q = [torch.clamp(d[:, k] / (wx if k < 2 else wy), min=-scale_clamp, max=scale_clamp) for k in range(4)]
    return torch.stack((q[0] * w + pb[:, 0], q[2] * h + pb[:, 1], q[1] * w + pb[:, 2], q[3] * h + pb[:, 3]), dim=1)


NLL_CONST = 2 * math.log(2 * math.pi)


def roi_box_loss(deltas, stdl, cls, prop, gtb, gstd, num_classes, mode, wx, wy, scale_clamp, ts_better, t_cert, beta=0.0, nll_const=None):
    """-> (per-row loss [R], [addends of gd [R, 4]], [addends of gs [R, 4]]) - the form of tests/loss_ref64.roi_box_loss.
    nll_const: nl_loss's additive 2 log(2 pi); given (the reference builds it as a float32 tensor, fast_rcnn.py:1283-1285, and a test
    against the reference executed in fp64 passes that value), modes 0, 1 and 3 are restated here even at beta 0"""
    assert mode in (0, 1, 2, 3, 4) and beta >= 0
    if mode == 2 or (mode != 4 and beta < 1e-5 and nll_const is None):
        return L64.roi_box_loss(deltas, stdl, cls, prop, gtb, gstd, num_classes, mode, wx, wy, scale_clamp, ts_better, t_cert)
    dt = deltas.dtype
    R = deltas.shape[0]
    dl = deltas.detach().clone().requires_grad_(True)
    sl = stdl.detach().clone().requires_grad_(True)
    fg = torch.nonzero((cls >= 0) & (cls < num_classes)).squeeze(1)
    loss = torch.zeros(R, dtype=dt)
    zero = [torch.zeros((R, 4), dtype=dt)]
    if fg.numel() == 0:
        return loss, zero, zero
    d, sd, pb, gb = dl[fg], sl[fg], prop[fg].to(dt), gtb[fg].to(dt)
    if mode == 4:
        rows = giou_loss(decode(d, pb, wx, wy, scale_clamp), gb)
        parts = [rows.sum()]
    else:
        sw, sh = pb[:, 2] - pb[:, 0] + 1.0, pb[:, 3] - pb[:, 1] + 1.0
        t = torch.stack((wx * (gb[:, 0] - pb[:, 0]) / sw, wx * (gb[:, 2] - pb[:, 2]) / sw, wy * (gb[:, 1] - pb[:, 1]) / sh,
                         wy * (gb[:, 3] - pb[:, 3]) / sh), dim=1)
        l1 = smooth_l1(d - t, beta)
        parts = [l1.sum()]
        rows = l1.sum(dim=1)
        if mode == 0:
            bx = decode(d, pb, wx, wy, scale_clamp)
            a1 = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
            a2 = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            whx = (torch.min(gb[:, 2], bx[:, 2]) - torch.max(gb[:, 0], bx[:, 0])).clamp(min=0)
            why = (torch.min(gb[:, 3], bx[:, 3]) - torch.max(gb[:, 1], bx[:, 1])).clamp(min=0)
            inter = whx * why
            iou = inter / (a1 + a2 - inter)
            sq = torch.square(torch.sigmoid(sd))
            nll = (torch.square(t - d) / (2 * sq) + 0.5 * torch.log(sq)).sum(dim=1) + (NLL_CONST if nll_const is None else nll_const)
            parts += [0.05 * (nll * iou.detach()).sum(), 0.05 * (nll.detach() * iou).sum()]
            rows = rows + 0.05 * nll * iou
    loss[fg] = rows.detach()
    return loss, L64._grads(parts, dl), L64._grads(parts, sl)


def roi_box_loss_pc(deltas, stdl, cls, prop, gtb, K, mode, wx, wy, scale_clamp, beta=0.0, nll_const=None):
    """per-class layout -> (per-row loss [R], [addends of gd [R, 4K]], [addends of gs [R, 4K]]) - the form of loss_ref64_percls"""
    col = P64.select_columns(cls, K)
    loss, gd, gs = roi_box_loss(torch.gather(deltas, 1, col), torch.gather(stdl, 1, col), cls, prop, gtb, None, K, mode, wx, wy, scale_clamp,
                                0.0, 0.0, beta, nll_const)
    fg = ((cls >= 0) & (cls < K))[:, None].to(deltas.dtype)
    return loss, [torch.zeros_like(deltas).scatter_(1, col, p * fg) for p in gd], [torch.zeros_like(deltas).scatter_(1, col, p * fg) for p in gs]


def branch_case(R, K, seed, beta):
    """[R, 4K] heads whose selected columns sit ON the branch points: rows 0, 6, 12, ... have gt == proposal (t = 0) and d cycling through
    +-beta (|d - t| == beta bit for bit, `beta` being an fp32 value), +-beta / 2 (quadratic side), +-(2 beta + 1/4) (linear side) and 0;
    rows 5, 11, ... the same offsets around a non-zero exact t; and for the GIoU rows 1 + 6i: a prediction disjoint from its gt box,
    2 + 6i: one contained in it, 3 + 6i: a zero-area prediction (x1 == x2), 4 + 6i: one containing it.  Proposals have power-of-two sides
    minus 1 (get_deltas divides by side + 1) and whole-pixel gt offsets: t is exact in fp32.  The row classes include -1, K, 0 and K - 1."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.round(torch.rand((R, 2), generator=g) * 100)
    side = torch.tensor([15.0, 31.0, 63.0])[torch.randint(0, 3, (R, 2), generator=g)]
    prop = torch.cat((xy, xy + side), dim=1)
    off = torch.round(torch.randn((R, 4), generator=g) * 2)                  # gt - proposal, whole pixels: t = w * off / 2^k is exact
    off[0::6] = 0.0                                                           # t = 0: d = +-beta there is d - t == beta bit for bit
    gtb = prop + off
    cls = torch.randint(-1, K + 1, (R,), generator=g, dtype=torch.int64)
    n = min(R, 12)
    cls[:n] = torch.arange(n) % K                                             # two full cycles of the row kinds are foreground
    if R > 13:
        cls[12], cls[13] = -1, K
    cls[R - 1] = K - 1
    wx, wy = L64.ROI_W
    s1 = side + 1.0
    t = torch.stack((wx * off[:, 0] / s1[:, 0], wx * off[:, 2] / s1[:, 0], wy * off[:, 1] / s1[:, 1], wy * off[:, 3] / s1[:, 1]), dim=1)
    b = torch.tensor(beta, dtype=torch.float32)
    kinds = [b, -b, b / 2, -b / 2, 2 * b + 0.25, -(2 * b + 0.25), torch.tensor(0.0)]
    sel = torch.stack([t[r] + torch.stack([kinds[(r + k) % len(kinds)] for k in range(4)]) for r in range(R)])
    w, h = side[:, 0], side[:, 1]
    for r in range(R):                                                        # the GIoU geometries, through the decode d / w * side
        m = r % 6
        if m == 1:    # disjoint: the whole box moves 2 widths to the right
            sel[r] = torch.tensor([2 * wx, 2 * wx, 0.0, 0.0])
        elif m == 2:  # contained in the gt box (gt = the proposal grown by 2): shrink by a quarter side
            gtb[r] = prop[r] + torch.tensor([-2.0, -2.0, 2.0, 2.0])
            sel[r] = torch.tensor([wx / 4, -wx / 4, wy / 4, -wy / 4])
        elif m == 3:  # zero area: x1 and x2 meet in the middle
            sel[r] = torch.tensor([wx / 2, -wx / 2, 0.0, 0.0])
        elif m == 4:  # contains the gt box
            gtb[r] = prop[r] + torch.tensor([2.0, 2.0, -2.0, -2.0])
            sel[r] = torch.tensor([-wx / 4, wx / 4, -wy / 4, wy / 4])
    deltas = torch.randn((R, 4 * K), generator=g) * 0.5
    std = torch.randn((R, 4 * K), generator=g)
    col = P64.select_columns(cls, K)
    deltas.scatter_(1, col, sel)
    return {"deltas": deltas, "std": std, "cls": cls, "prop": prop, "gtb": gtb, "col": col, "t": t}
