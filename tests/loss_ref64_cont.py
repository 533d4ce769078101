"""fp64 autograd reference of the positive-location terms of the CONTINUOUS FCOS regression head (MODEL.FCOS.REG_DISCRETE False;
csrc/fcos.hip utv2_fcos_loc_terms_cont_*) and its input grids.  HELPER MODULE: no tests in it (tests/test_fcos_cont.py anchors it on
the CPU against the executed-reference golden, tests/test_fcos_cont_gpu.py runs the kernels against it).

Same conventions as tests/loss_ref64.py (dtype of the inputs = the precision, gradients from torch.autograd only, a gradient returned
as its list of addends): the only difference to loss_ref64.loc_terms is d = relu(row[0:4]) in the place of the Integral
(fcos/fcos.py:364, fcos_outputs.py:349-350) and the row layout [ltrb 4 | std 4 | ctr 1 | pad]."""
import math

import torch
import torch.nn.functional as F

from tests.loss_ref64 import LT_KL_WCTR, LT_KLLOSS, LT_QUALITY_IOU, _grads, _ltrb_iou


def loc_terms_cont(box_row, t, bvars, labels, flags, ts_better, ts_cert, num_classes=80, coef=(1.0, 1.0, 1.0, 1.0)):
    """-> (terms [P, 8]: the per-row addends of the 8 sums, [addends of dbox [P, BS] for coef = (c_bce, c_giou, c_nll, c_l1)],
    info: sign of d - t, selection mask and d of the positive rows)"""
    P, BS = box_row.shape
    dt = box_row.dtype
    box = box_row.detach().clone().requires_grad_(True)
    pos = torch.nonzero((labels >= 0) & (labels != num_classes)).squeeze(1)
    terms = torch.zeros((P, 8), dtype=dt)
    if pos.numel() == 0:
        return terms, [torch.zeros_like(box_row)], {"sign": torch.zeros((0, 4)), "sel": torch.zeros((0, 4), dtype=torch.bool)}
    row = box[pos]
    tt = t[pos].to(dt)
    d = F.relu(row[:, 0:4])
    std, c = row[:, 4:8], row[:, 8]
    lr, tb = tt[:, [0, 2]], tt[:, [1, 3]]
    ctr_t = torch.sqrt((lr.min(dim=1)[0] / lr.max(dim=1)[0]) * (tb.min(dim=1)[0] / tb.max(dim=1)[0]))
    iou, giou = _ltrb_iou(d, tt, None, True)
    iou_t = iou.detach()
    if flags & LT_QUALITY_IOU:
        ctr_t = iou_t
    loc_type = (flags >> 2) & 3
    gl = 1 - giou if loc_type == 0 else (-torch.log(iou) if loc_type == 1 else 1 - iou)
    if flags & LT_KLLOSS:
        n = (d - tt).abs()
        sl1 = torch.where(n < 1.0, 0.5 * n ** 2, n - 0.5)
        nll = (torch.exp(-std) * sl1 + 0.5 * std).sum(dim=1)
        w = ctr_t if flags & LT_KL_WCTR else torch.ones_like(ctr_t)
    else:
        sq = torch.square(torch.sigmoid(std))
        nll = (torch.square(tt - d) / (2 * sq) + 0.5 * torch.log(sq)).sum(dim=1) + 2 * math.log(2 * math.pi)
        w = iou_t
    bce = F.binary_cross_entropy_with_logits(c, ctr_t, reduction="none")
    v = torch.zeros((pos.numel(), 8), dtype=dt)
    v[:, 0] = 1
    v[:, 1] = ctr_t
    v[:, 2] = bce
    v[:, 3] = gl * ctr_t
    v[:, 4] = nll * w
    sel = torch.zeros((pos.numel(), 4), dtype=torch.bool)
    l1 = None
    if bvars is not None:
        cs = 1 - torch.sigmoid(std.detach())
        ct = 1 - torch.sigmoid(bvars[pos].to(dt))
        sel = (ct > ts_cert) & (ct > cs + ts_better)
        l1 = ((d - tt).abs() * sel.to(dt))
        v[:, 5] = sel.to(dt).sum(dim=1)
        v[:, 6] = l1.sum(dim=1)
    terms[pos] = v.detach()
    parts = [coef[0] * v[:, 2].sum(), coef[1] * v[:, 3].sum(), coef[2] * v[:, 4].sum(), None if l1 is None else coef[3] * l1.sum()]
    return terms, _grads(parts, box), {"sign": torch.sign(d - tt).detach(), "sel": sel, "d": d.detach()}


# =================================================================================================
# input grids (fp32, CPU, seeded).  Every value is a dyadic rational of a few bits or a plain random fp32 number, so d, t and d - t are
# the same numbers in fp32 and fp64: a tie, a dead ReLU or |d - t| == 1 is met in both precisions or in neither.
# =================================================================================================
TS_BETTER, TS_CERT = 0.1, 0.5    # as tests/loss_ref64.loc_case; no (std, bvars) pair of the grids comes near ct == cs + 0.1


def cont_case(P, BS, seed, with_bvars=True, labels_mode="mixed"):
    """box [P, BS], reg targets [P, 4], bvars [P, 4] | None, labels [P].  Row r % 12 selects a branch point:
      1 stored value exactly 0 on every side     2 negative on two sides          3 -0.0
      4 all four distances dead (IoU = 1 / (ta + 1))   5 d == t on all sides      6 d == t on one side, d < t / d > t on the others
      7 |d - t| == 1 on all sides (above and below)    8 bvars logit 0: ct == ts_cert == 0.5 (the strict > decides)
      9 very small targets (1e-3)                10 large targets (1e3), large d  11 l == r and t == b: centerness target exactly 1
    other rows: random."""
    g = torch.Generator().manual_seed(seed)
    box = torch.zeros((P, BS))
    box[:, 0:4] = torch.randn((P, 4), generator=g) * 3.0 + 2.0
    box[:, 4:8] = torch.tensor([0.0, 1.5, -1.5, 5.0, -5.0, 20.0, -20.0])[torch.randint(0, 7, (P, 4), generator=g)]
    box[:, 8] = torch.tensor([0.0, 50.0, -50.0, 1.5, -0.75])[torch.randint(0, 5, (P,), generator=g)]
    box[:, 9:] = torch.randn((P, BS - 9), generator=g)        # pad columns: never read
    tv = torch.tensor([0.5, 1.375, 3.375, 7.375, 12.375, 15.375, 40.625])
    t = tv[torch.randint(0, len(tv), (P, 4), generator=g)]
    bv = torch.tensor([0.0, -3.0, 3.0, -8.0])[torch.randint(0, 4, (P, 4), generator=g)]
    for r in range(P):
        k = r % 12
        if k == 1:
            box[r, 0:4] = 0.0
        elif k == 2:
            box[r, 0], box[r, 3] = -1.25, -7.0
        elif k == 3:
            box[r, 0:4] = torch.tensor([-0.0, 2.5, -0.0, 4.25])
        elif k == 4:
            box[r, 0:4] = torch.tensor([-1.0, 0.0, -0.0, -3.5])
        elif k == 5:
            box[r, 0:4] = t[r]
        elif k == 6:
            box[r, 0:4] = t[r] + torch.tensor([0.0, -0.25, 0.25, 0.0])
        elif k == 7:
            box[r, 0:4] = t[r] + torch.tensor([1.0, -1.0, 1.0, 1.0])
            box[r, 1] = max(float(box[r, 1]), 0.375)      # t = 0.5: d = 0.375, |d - t| < 1
        elif k == 8:
            bv[r] = 0.0
        elif k == 9:
            t[r] = torch.tensor([1e-3, 2e-3, 1e-3, 1e-3])
            box[r, 0:4] = torch.tensor([1e-3, 0.5, 0.0, 3e-3])
        elif k == 10:
            t[r] = torch.tensor([1e3, 750.0, 1.5, 1e3])
            box[r, 0:4] = torch.tensor([990.0, 1e3, 2.0, 1e3])
        elif k == 11:
            t[r, 2], t[r, 3] = t[r, 0], t[r, 1]
    labels = torch.randint(0, 80, (P,), generator=g, dtype=torch.int32)
    if labels_mode == "skipped":
        labels[:] = -1
    elif labels_mode == "background":
        labels[:] = 80
    elif labels_mode == "mixed" and P > 2:
        labels[13::17] = -1
        labels[14::9] = 80
    return box.contiguous(), t.contiguous(), (bv.contiguous() if with_bvars else None), labels


def better_tie_case(BS=16):
    """rows where ct == cs + ts_better holds EXACTLY in fp32 (ts_better = 0: cs == ct from equal logits) next to rows one step to either
    side: the strict > keeps the equal row out of the selection.  -> (box, t, bvars, labels, ts_better, ts_cert)"""
    box = torch.zeros((6, BS))
    box[:, 0:4] = torch.tensor([2.0, 3.0, 1.5, 2.5])
    t = torch.tensor([[2.5, 2.5, 2.5, 2.5]]).repeat(6, 1)
    box[:, 4:8] = torch.tensor([-2.0, -2.0, -2.0, -3.0, -3.0, -3.0])[:, None]
    bv = torch.stack([torch.full((4,), float(v)) for v in (-2.0, -2.5, -1.5, -3.0, -3.5, -2.5)])
    return box, t, bv, torch.zeros(6, dtype=torch.int32), 0.0, 0.5
