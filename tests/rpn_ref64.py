"""Plain torch references of what the RPN's config keys switch on (MODEL.RPN.SMOOTH_L1_BETA / BBOX_REG_LOSS_TYPE "giou" /
BOUNDARY_THRESH, MODEL.ANCHOR_GENERATOR.SIZES / ASPECT_RATIOS / OFFSET).  HELPER MODULE: no tests in it (tests/test_rpn_keys.py anchors it
on the executed reference's golden, tests/test_rpn_keys_gpu.py holds the kernels and the model to it).

Like tests/loss_ref64.py, which it builds on: every function works in the dtype of its floating inputs (float64 = r64, float32 = r32),
gradients come from torch.autograd only, torch.min / torch.max / clamp stand where fvcore / Detectron2 use them, and a gradient is
returned as the list of its addends."""
import math

import torch

from tests import loss_ref64 as L64

SCALE_CLAMP = math.log(1000.0 / 16)


# =================================================================================================
# localisation loss: D2 _dense_box_regression_loss [D2-recall] as proposal_generator/rpn.py:194-202 calls it
# =================================================================================================
def smooth_l1(d, beta):
    """fvcore smooth_l1_loss of the difference d"""
    n = d.abs()
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def apply_deltas(deltas, boxes, weights, scale_clamp=SCALE_CLAMP):
    """D2 Box2BoxTransform.apply_deltas (centre-size), no clip"""
    w, h = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    cx, cy = boxes[..., 0] + 0.5 * w, boxes[..., 1] + 0.5 * h
    dx, dy = deltas[..., 0] / weights[0], deltas[..., 1] / weights[1]
    dw = torch.clamp(deltas[..., 2] / weights[2], max=scale_clamp)
    dh = torch.clamp(deltas[..., 3] / weights[3], max=scale_clamp)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1)


def giou_parts(b1, b2, eps=1e-7):
    """fvcore giou_loss = 1 - iou + pen -> (iou, pen) elementwise"""
    x1, y1, x2, y2 = b1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = b2.unbind(dim=-1)
    xk1, yk1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xk2, yk2 = torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.where((yk2 > yk1) & (xk2 > xk1), (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    iou = inter / (union + eps)
    xc1, yc1 = torch.min(x1, x1g), torch.min(y1, y1g)
    xc2, yc2 = torch.max(x2, x2g), torch.max(y2, y2g)
    area_c = (xc2 - xc1) * (yc2 - yc1)
    return iou, (area_c - union) / (area_c + eps)


def rpn_loss(x, dl, anchors, s, gt_boxes, gt_scores, weights, loc_mode=0, beta=0.0, scale_clamp=SCALE_CLAMP):
    """loss_ref64.rpn_loss with the localisation term of the keys.  x [N, S] / dl [N, npos, 4]: the logits / deltas of the sampling
    slots.  -> (cls [N, S], loc: per-element [N, npos, 4] (smooth-L1) or per-slot [N, npos] (giou) terms, gobj, [addends of gdl], s: the largest addend
    magnitude of every gdl element)"""
    dt = x.dtype
    cls, _, gobj, _ = L64.rpn_loss(x, dl, anchors, s, gt_boxes, gt_scores, weights)
    dl = dl.detach().clone().requires_grad_(True)
    N, npos = s["pos_idx"].shape
    hg = s["has_gt"].reshape(N, 1).bool()
    g = torch.gather(s["matched32"].long(), 1, s["pos_idx"])
    pv = s["pos_valid"].bool() & hg
    one = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=dt)
    a = torch.where(pv[..., None], anchors.to(dt)[s["pos_idx"]], one)
    b = torch.where(pv[..., None], torch.gather(gt_boxes.to(dt), 1, g[..., None].expand(-1, -1, 4)), one)
    if loc_mode == 0:
        sw, sh = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
        sx, sy = a[..., 0] + 0.5 * sw, a[..., 1] + 0.5 * sh
        tw, th = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
        tx, ty = b[..., 0] + 0.5 * tw, b[..., 1] + 0.5 * th
        t = torch.stack((weights[0] * (tx - sx) / sw, weights[1] * (ty - sy) / sh, weights[2] * torch.log(tw / sw),
                         weights[3] * torch.log(th / sh)), dim=-1)
        loc = smooth_l1(dl - t, beta) * pv.to(dt)[..., None]
        parts = L64._grads([loc.sum()], dl)
        # on the quadratic side the derivative (delta - target) / beta is a difference of two addends, delta / beta and target / beta:
        # the larger of them is the comparator's cancellation scale there; elsewhere the derivative is a sign, its own scale
        quad = ((dl - t).abs() < beta) & pv[..., None] if beta >= 1e-5 else torch.zeros_like(dl, dtype=torch.bool)
        s = torch.where(quad, torch.max(dl.abs(), t.abs()) / (beta if beta >= 1e-5 else 1.0), parts[0].abs()).detach()
    else:
        iou, pen = giou_parts(apply_deltas(dl, a, weights, scale_clamp), b)
        m = pv.to(dt)
        loc = (1 - iou + pen) * m
        parts = L64._grads([(-iou * m).sum(), (pen * m).sum()], dl)
        s = L64.total_and_scale(parts)[1]
    return cls, loc.detach(), gobj, parts, s


# =================================================================================================
# labels: D2 Matcher (thresholds lo / hi, allow_low_quality_matches), an image without gt all negative, then Boxes.inside_box
# (rpn.py:117-131) [D2-recall]; and the "k smallest keys" draw of the product's samplers
# =================================================================================================
def inside_box(anchors, hw, thresh):
    h, w = hw
    return (anchors[:, 0] >= -thresh) & (anchors[:, 1] >= -thresh) & (anchors[:, 2] < w + thresh) & (anchors[:, 3] < h + thresh)


def rpn_labels(anchors, gt_boxes, gt_valid, image_sizes, lo, hi, boundary_thresh):
    """anchors [R, 4], gt_boxes [N, G, 4], gt_valid [N, G] -> (labels [N, R] int8 in {-1, 0, 1}, matched gt slot [N, R] int32)"""
    N, R = gt_boxes.shape[0], anchors.shape[0]
    labels = torch.zeros((N, R), dtype=torch.int8)
    matched = torch.zeros((N, R), dtype=torch.int32)
    a = anchors.double()
    for n in range(N):
        slots = torch.nonzero(gt_valid[n].bool()).squeeze(1)
        if slots.numel():
            gb = gt_boxes[n, slots].double()
            wh = (torch.min(gb[:, None, 2:], a[:, 2:]) - torch.max(gb[:, None, :2], a[:, :2])).clamp(min=0)
            inter = wh.prod(dim=2)
            area = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[:, None] + (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
            iou = torch.where(inter > 0, inter / (area - inter), torch.zeros((), dtype=torch.float64))
            vals, idx = iou.max(dim=0)
            lab = torch.full((R,), -1, dtype=torch.int8)
            lab[vals < lo] = 0
            lab[vals >= hi] = 1
            lab[(iou == iou.max(dim=1)[0][:, None]).any(dim=0)] = 1
            labels[n], matched[n] = lab, slots[idx].int()
        if boundary_thresh >= 0:
            labels[n][~inside_box(anchors, image_sizes[n], boundary_thresh)] = -1
    return labels, matched


def sample(labels, keys, batch, frac):
    """the samplers' padded form: the <= int(batch * frac) positives and the negatives that fill the batch, by ascending key then index"""
    N, R = labels.shape
    npos_max = int(batch * frac)
    out = dict(pos_idx=torch.zeros((N, npos_max), dtype=torch.int64), pos_valid=torch.zeros((N, npos_max), dtype=torch.uint8),
               neg_idx=torch.zeros((N, batch), dtype=torch.int64), neg_valid=torch.zeros((N, batch), dtype=torch.uint8))
    for n in range(N):
        pos = torch.nonzero(labels[n] == 1).squeeze(1)
        neg = torch.nonzero(labels[n] == 0).squeeze(1)
        pos = pos[torch.argsort(keys[n, pos], stable=True)][:npos_max]
        neg = neg[torch.argsort(keys[n, neg], stable=True)][:batch]
        out["pos_idx"][n, :pos.numel()] = pos
        out["pos_valid"][n, :pos.numel()] = 1
        out["neg_idx"][n, :neg.numel()] = neg
        out["neg_valid"][n, :min(neg.numel(), batch - pos.numel())] = 1
    return out


# =================================================================================================
# D2 DefaultAnchorGenerator [D2-recall]
# =================================================================================================
def _per_level(params, n):
    params = list(params)
    if not isinstance(params[0], (list, tuple)):
        return [list(params)] * n
    if len(params) == 1:
        return [list(params[0])] * n
    assert len(params) == n
    return [list(p) for p in params]


def anchor_tables(level_hw, strides, sizes, ratios, offset=0.0):
    """one [h * w * A, 4] float32 table per level, order (h, w, sizes outer x ratios inner)"""
    sizes, ratios = _per_level(sizes, len(strides)), _per_level(ratios, len(strides))
    out = []
    for (h, w), st, sz, rt in zip(level_hw, strides, sizes, ratios):
        cell = []
        for s in sz:
            area = s ** 2.0
            for r in rt:
                cw = math.sqrt(area / r)
                chh = r * cw
                cell.append([-cw / 2.0, -chh / 2.0, cw / 2.0, chh / 2.0])
        cell = torch.tensor(cell, dtype=torch.float32)
        sx = torch.tensor([offset * st + i * st for i in range(w)], dtype=torch.float32)
        sy = torch.tensor([offset * st + i * st for i in range(h)], dtype=torch.float32)
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
        out.append((shifts.view(-1, 1, 4) + cell.view(1, -1, 4)).reshape(-1, 4))
    return out


# =================================================================================================
# input grids
# =================================================================================================
def rpn_key_case(seed, A=3, beta=0.11, with_scores=True, giou=False):
    """loss_ref64.rpn_case (edge grid: an image without gt, empty slots naming non-finite values, a delta equal to its target) at A
    anchors per cell, with deltas and boxes that are multiples of 1/64, and on image 0:
      smooth-L1 rows (positive slots 3, 4, 5): delta - target == beta bit for bit, one fp32 ulp below, one ulp above - the gt box is the
        anchor itself (every target 0 in any precision), so the difference is the delta;
      giou rows: slot 3 disjoint from its gt, 4 contained in it, 5 containing it, 6 with dw above SCALE_CLAMP (derivative exactly 0)."""
    hw = (12, 5) if A >= 3 else (36, 15)      # rpn_case's levels; three times the pixels at A < 3: its 32 slots per image need R >= 32
    c = L64.rpn_case(seed, hw=hw, A=A, with_scores=with_scores)
    q = lambda t: torch.round(t * 64.0) / 64.0   # noqa: E731
    fin = torch.isfinite(c["deltas"])
    c["deltas"] = torch.where(fin, q(c["deltas"]), c["deltas"])
    c["anchors"], c["gt_boxes"] = q(c["anchors"]), q(c["gt_boxes"])
    s, m = c["s"], c["s"]["matched32"]
    b32 = torch.tensor(beta if beta else 0.11, dtype=torch.float32)
    used = {int(m[0, s["pos_idx"][0, 2]])}
    rows = [int(s["pos_idx"][0, j]) for j in (3, 4, 5, 6)]
    G = c["gt_boxes"].shape[1]
    free = [g for g in range(G) if g not in used]
    if not giou:
        g1 = free[0]
        for r in rows[:3]:
            m[0, r] = g1
        # three anchors share one gt box, equal to all of them: give them the same box
        c["gt_boxes"][0, g1] = c["anchors"][rows[0]]
        for r in rows[1:3]:
            c["anchors"][r] = c["anchors"][rows[0]]
        up = torch.nextafter(b32, torch.tensor(2.0))
        dn = torch.nextafter(b32, torch.tensor(0.0))
        c["deltas"][0, rows[0]] = torch.stack((b32, -b32, b32, -b32))
        c["deltas"][0, rows[1]] = torch.stack((dn, -dn, dn, dn))
        c["deltas"][0, rows[2]] = torch.stack((up, -up, -up, up))
    else:
        g1 = free[0]
        c["gt_boxes"][0, g1] = torch.tensor([20.0, 20.0, 40.0, 44.0])
        geo = [([100.0, 100.0, 116.0, 108.0], [0.0, 0.0, 0.0, 0.0]),            # disjoint
               ([24.0, 26.0, 32.0, 34.0], [0.125, 0.0, 0.25, -0.25]),          # inside the gt
               ([22.0, 24.0, 38.0, 40.0], [0.0, 0.0, 1.0, 1.5]),               # grows around it
               ([24.0, 24.0, 40.0, 40.0], [0.25, 0.0, 5.0, 0.5])]              # dw = 5 > log(62.5) = 4.135
        for r, (an, de) in zip(rows, geo):
            m[0, r] = g1
            c["anchors"][r] = torch.tensor(an)
            c["deltas"][0, r] = torch.tensor(de)
    c["rows"] = rows
    # the level-first head of the same numbers (ch = 5 A + 1: one pad column)
    N, hw, ch, R = c["N"], c["hw"], c["ch"], c["R"]
    head = torch.zeros((N * sum(hw), ch))
    for n in range(N):
        for r in range(R):
            oo, od = L64.rpn_head_offsets(hw, N, A, ch, n, r)
            head.view(-1)[oo] = c["obj"][n, r]
            head.view(-1)[od:od + 4] = c["deltas"][n, r]
    c["head"] = head
    return c
