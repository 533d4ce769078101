"""Plain high-precision references of the fused loss kernels (csrc/fcos.hip, csrc/rcnn.hip), the comparator that holds a kernel to them,
and the deterministic input grids.  HELPER MODULE: no tests in it (tests/test_loss_ref64.py anchors it on the CPU,
tests/test_loss_kernels_fp64_gpu.py runs the kernels against it).

Every reference is written from the formula with torch ops, works in the dtype of its floating inputs (float64 = the reference r64,
float32 = the same function in fp32, r32) and takes its gradients from torch.autograd only.  torch.min / torch.max / clamp / abs stand
exactly where the reference uses them, so the behaviour on ties is autograd's (half / half for min and max, inclusive bounds for clamp,
0 for abs at 0 - pinned by test_loss_ref64.py::test_tie_semantics_of_autograd), not a second hand derivation.

A gradient is returned as the list of the ADDENDS that form it (one autograd call each); the reference gradient is their sum and
`s`, the largest addend magnitude per element, scales the cancellation term of the comparator.

`mut` selects a deliberately WRONG variant (test_loss_ref64.py shows that the comparator rejects each of them on the edge grids):
  tie1      min / max send the whole gradient to the first operand on a tie (instead of half)
  nosmooth  IoU without the +1 smoothing
  certge    ct >= ts_cert instead of ct > ts_cert
  clampex   the derivative of the clamp is 0 AT the bound (exclusive)
  series1   log1p(e) replaced by e below the kernel's series switch (e < 1e-2)
  alphaneg  the alpha weight applied for alpha < 0 too
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24   # unit roundoff of fp32


# =================================================================================================
# small pieces
# =================================================================================================
def _min(a, b, mut):
    return torch.where(a <= b, a, b) if mut == "tie1" else torch.min(a, b)


def _max(a, b, mut):
    return torch.where(a >= b, a, b) if mut == "tie1" else torch.max(a, b)


def _grads(parts, leaf):
    """one autograd gradient per addend (zeros where an addend does not depend on the leaf)"""
    out = []
    for p in parts:
        if p is None or not p.requires_grad:
            out.append(torch.zeros_like(leaf))
            continue
        g, = torch.autograd.grad(p, leaf, retain_graph=True, allow_unused=True)
        out.append(torch.zeros_like(leaf) if g is None else g)
    return out


def total_and_scale(parts):
    """(sum of the addends, largest addend magnitude)"""
    tot = parts[0].clone()
    s = parts[0].abs()
    for p in parts[1:]:
        tot = tot + p
        s = torch.max(s, p.abs())
    return tot, s


# =================================================================================================
# sigmoid focal loss: fvcore.nn.sigmoid_focal_loss as called at fcos/fcos_outputs.py:329-335,619-625 (oracle/utv2_oracle.py:56-64),
# one-hot target from labels (label < 0: row skipped, label == C: background, all-zero target)
# =================================================================================================
def focal(x, labels, C, alpha, gamma, mut=None):
    """-> (loss [P, C], [addends of d sum / dx])"""
    x = x.detach().clone().requires_grad_(True)
    t = (labels[:, None] == torch.arange(C)[None, :]).to(x.dtype)
    live = (labels >= 0).to(x.dtype)[:, None]
    p = torch.sigmoid(x)
    if mut == "series1":
        e = torch.exp(-x.abs())
        ce = torch.clamp(x, min=0) - x * t + torch.where(e < 1e-2, e, torch.log1p(e))
    else:
        ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    mod = (1 - p_t) ** gamma
    at = alpha * t + (1 - alpha) * (1 - t) if (alpha >= 0 or mut == "alphaneg") else torch.ones_like(t)
    loss = ce * mod * at * live
    # the two addends of the product rule: d ce * mod and ce * d mod
    parts = _grads([(ce * mod.detach() * at * live).sum(), (ce.detach() * mod * at * live).sum()], x)
    return loss.detach(), parts


# =================================================================================================
# FCOS positive-location terms: fcos/fcos_outputs.py:340-416 (supervised), :514-590 (pseudo); Integral :44-77; centerness target
# :80-88; IoU target :91-129; IOULoss layers/iou_loss.py:26-76; NLLoss layers/kl_loss.py:69-105; KLLoss :11-66
# =================================================================================================
LT_QUALITY_IOU, LT_KLLOSS, LT_KL_WCTR = 1, 2, 16
LEGAL_FLAGS = [q | (lt << 2) | k for lt in (0, 1, 2) for q in (0, 1) for k in (0, LT_KLLOSS, LT_KLLOSS | LT_KL_WCTR)]


def _ltrb_iou(d, t, mut, need_giou):
    ta = (t[:, 0] + t[:, 2]) * (t[:, 1] + t[:, 3])
    pa = (d[:, 0] + d[:, 2]) * (d[:, 1] + d[:, 3])
    wi = _min(d[:, 0], t[:, 0], mut) + _min(d[:, 2], t[:, 2], mut)
    hi = _min(d[:, 3], t[:, 3], mut) + _min(d[:, 1], t[:, 1], mut)
    ai = wi * hi
    au = ta + pa - ai
    sm = 0.0 if mut == "nosmooth" else 1.0
    iou = (ai + sm) / (au + sm)
    if not need_giou:
        return iou, None
    gw = _max(d[:, 0], t[:, 0], mut) + _max(d[:, 2], t[:, 2], mut)
    gh = _max(d[:, 3], t[:, 3], mut) + _max(d[:, 1], t[:, 1], mut)
    ac = gw * gh
    return iou, iou - (ac - au) / ac


def loc_terms(box_row, t, bvars, labels, flags, ts_better, ts_cert, num_classes=80, coef=(1.0, 1.0, 1.0, 1.0), mut=None):
    """-> (terms [P, 8]: the per-row addends of the LT_NSUM sums, [addends of dbox [P, BS] for coef = (c_bce, c_giou, c_nll, c_l1)],
    info: dict of the branch decisions (sign of d - t, selection mask) for the positive rows)"""
    P, BS = box_row.shape
    dt = box_row.dtype
    box = box_row.detach().clone().requires_grad_(True)
    pos = torch.nonzero((labels >= 0) & (labels != num_classes)).squeeze(1)
    terms = torch.zeros((P, 8), dtype=dt)
    if pos.numel() == 0:
        return terms, [torch.zeros_like(box_row)], {"sign": torch.zeros((0, 4)), "sel": torch.zeros((0, 4), dtype=torch.bool)}
    row = box[pos]
    tt = t[pos].to(dt)
    prob = F.softmax(row[:, :68].reshape(-1, 17), dim=1)
    d = (prob * torch.arange(17, dtype=dt)[None, :]).sum(dim=1).reshape(-1, 4)     # Integral
    std, c = row[:, 68:72], row[:, 72]
    lr, tb = tt[:, [0, 2]], tt[:, [1, 3]]
    ctr_t = torch.sqrt((lr.min(dim=1)[0] / lr.max(dim=1)[0]) * (tb.min(dim=1)[0] / tb.max(dim=1)[0]))
    iou, giou = _ltrb_iou(d, tt, mut, True)
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
        sel = ((ct >= ts_cert) if mut == "certge" else (ct > ts_cert)) & (ct > cs + ts_better)
        l1 = ((d - tt).abs() * sel.to(dt))
        v[:, 5] = sel.to(dt).sum(dim=1)
        v[:, 6] = l1.sum(dim=1)
    terms[pos] = v.detach()
    parts = [coef[0] * v[:, 2].sum(), coef[1] * v[:, 3].sum(), coef[2] * v[:, 4].sum(), None if l1 is None else coef[3] * l1.sum()]
    grads = _grads(parts, box)
    return terms, grads, {"sign": torch.sign(d - tt).detach(), "sel": sel, "d": d.detach()}


# =================================================================================================
# softmax focal loss of the ROI head: roi_heads/fast_rcnn.py:925-936 + FocalLoss :1405-1429
# =================================================================================================
def softmax_focal(x, target, gamma, mut=None):
    """-> (per-row loss [R] (0 where target < 0), [gradient [R, C]], s [R, C])"""
    x = x.detach().clone().requires_grad_(True)
    live = target >= 0
    ce = F.cross_entropy(x, target.clamp(min=0).long(), reduction="none")
    ce2 = ce.detach().clone().requires_grad_(True)
    loss2 = (1 - torch.exp(-ce2)) ** gamma * ce2
    dce, = torch.autograd.grad((loss2 * live.to(x.dtype)).sum(), ce2)
    loss = ((1 - torch.exp(-ce)) ** gamma * ce) * live.to(x.dtype)
    g, = torch.autograd.grad(loss.sum(), x)
    onehot = F.one_hot(target.clamp(min=0).long(), x.shape[1]).to(x.dtype)
    # d loss / dx = dce * (softmax - onehot): the two addends
    s = dce.abs()[:, None] * torch.max(F.softmax(x.detach(), dim=1), onehot)
    return loss.detach(), [g], s


# =================================================================================================
# RPN losses on the sampled anchors: proposal_generator/rpn.py:153-225 (D2 Box2BoxTransform.get_deltas for the targets)
# =================================================================================================
def rpn_head_offsets(head_hw, N, A, ch, n, r):
    """element offsets (objectness logit, first delta) of anchor r of image n in the level-first head output"""
    a0, row0 = 0, 0
    for hw in head_hw:
        if r < a0 + hw * A:
            q = r - a0
            p, a = q // A, q % A
            row = row0 + n * hw + p
            return row * ch + a, row * ch + A + a * 4
        a0 += hw * A
        row0 += N * hw
    raise IndexError(r)


def rpn_loss(x, dl, anchors, s, gt_boxes, gt_scores, weights):
    """x [N, S]: the objectness logit of every sampling slot (positives first; any finite placeholder on slots without weight),
    dl [N, npos, 4]: the deltas of the positive slots.  -> (cls [N, S], loc [N, npos, 4] per-slot losses, gobj, gdl)"""
    dt = x.dtype
    x = x.detach().clone().requires_grad_(True)
    dl = dl.detach().clone().requires_grad_(True)
    N, npos = s["pos_idx"].shape
    nneg = s["neg_idx"].shape[1]
    idx = torch.cat((s["pos_idx"], s["neg_idx"]), dim=1)
    valid = torch.cat((s["pos_valid"], s["neg_valid"]), dim=1).bool()
    hg = s["has_gt"].reshape(N, 1).bool()
    g = torch.gather(s["matched32"].long(), 1, idx)
    w = valid.to(dt)
    if gt_scores is not None:
        w = w * torch.where(hg, torch.gather(gt_scores.to(dt), 1, g), torch.zeros((), dtype=dt))
    tgt = torch.cat((torch.ones((N, npos), dtype=dt), torch.zeros((N, nneg), dtype=dt)), dim=1)
    cls = F.binary_cross_entropy_with_logits(x, tgt, reduction="none") * w
    pv = (s["pos_valid"].bool() & hg)
    a = anchors.to(dt)[s["pos_idx"]]                                   # [N, npos, 4]
    b = torch.gather(gt_boxes.to(dt), 1, g[:, :npos, None].expand(-1, -1, 4))
    one = torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=dt)
    a = torch.where(pv[..., None], a, one)
    b = torch.where(pv[..., None], b, one)
    sw, sh = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    sx, sy = a[..., 0] + 0.5 * sw, a[..., 1] + 0.5 * sh
    tw, th = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    tx, ty = b[..., 0] + 0.5 * tw, b[..., 1] + 0.5 * th
    t = torch.stack((weights[0] * (tx - sx) / sw, weights[1] * (ty - sy) / sh, weights[2] * torch.log(tw / sw),
                     weights[3] * torch.log(th / sh)), dim=-1)
    loc = (dl - t).abs() * pv.to(dt)[..., None]
    gobj, = torch.autograd.grad(cls.sum(), x)
    gdl, = torch.autograd.grad(loc.sum(), dl)
    return cls.detach(), loc.detach(), gobj, gdl


# =================================================================================================
# box regression losses of the boundary-variance predictor: roi_heads/fast_rcnn.py:938-1090 (box_reg_loss "nlloss" / smooth_l1 beta 0,
# box_reg_pseudo_loss "tsbetter" / smooth_l1), nl_loss :1228-1292, matched IoU :20-44, Box2BoxXYXYTransform box_regression.py:11-129
# =================================================================================================
def _clamp(v, c, mut):
    if mut == "clampex":
        return torch.where((v > -c) & (v < c), v, torch.clamp(v.detach(), min=-c, max=c))
    return torch.clamp(v, min=-c, max=c)


def roi_box_loss(deltas, stdl, cls, prop, gtb, gstd, num_classes, mode, wx, wy, scale_clamp, ts_better, t_cert, mut=None):
    """-> (per-row loss [R], [addends of gd [R, 4]], [addends of gs [R, 4]])"""
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
    sw, sh = pb[:, 2] - pb[:, 0] + 1.0, pb[:, 3] - pb[:, 1] + 1.0
    t = torch.stack((wx * (gb[:, 0] - pb[:, 0]) / sw, wx * (gb[:, 2] - pb[:, 2]) / sw, wy * (gb[:, 1] - pb[:, 1]) / sh,
                     wy * (gb[:, 3] - pb[:, 3]) / sh), dim=1)
    if mode == 2:
        ct = 1 - torch.sigmoid(gstd[fg].to(dt) if gstd is not None else torch.zeros_like(d))
        cs = 1 - torch.sigmoid(sd.detach())
        sel = (ct > cs + ts_better) & ((ct >= t_cert) if mut == "certge" else (ct > t_cert))
        l1 = (d - t).abs() * sel.to(dt)
        parts = [l1.sum()]
        rows = l1.sum(dim=1)
    else:
        l1 = (d - t).abs()
        parts = [l1.sum()]
        rows = l1.sum(dim=1)
        if mode == 0:
            w, h = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
            q0, q1 = _clamp(d[:, 0] / wx, scale_clamp, mut), _clamp(d[:, 1] / wx, scale_clamp, mut)
            q2, q3 = _clamp(d[:, 2] / wy, scale_clamp, mut), _clamp(d[:, 3] / wy, scale_clamp, mut)
            px1, px2, py1, py2 = q0 * w + pb[:, 0], q1 * w + pb[:, 2], q2 * h + pb[:, 1], q3 * h + pb[:, 3]
            a1 = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
            a2 = (px2 - px1) * (py2 - py1)
            whx = (_min(gb[:, 2], px2, mut) - _max(gb[:, 0], px1, mut)).clamp(min=0)
            why = (_min(gb[:, 3], py2, mut) - _max(gb[:, 1], py1, mut)).clamp(min=0)
            inter = whx * why
            iou = inter / (a1 + a2 - inter)
            sq = torch.square(torch.sigmoid(sd))
            nll = (torch.square(t - d) / (2 * sq) + 0.5 * torch.log(sq)).sum(dim=1) + 2 * math.log(2 * math.pi)
            parts += [0.05 * (nll * iou.detach()).sum(), 0.05 * (nll.detach() * iou).sum()]
            rows = rows + 0.05 * nll * iou
    loss[fg] = rows.detach()
    return loss, _grads(parts, dl), _grads(parts, sl)


# =================================================================================================
# the comparator
# =================================================================================================
def _np(a):
    return a.detach().cpu().double().numpy().reshape(-1) if torch.is_tensor(a) else np.asarray(a, dtype=np.float64).reshape(-1)


def _cls(a):
    """class of a non-finite value: 1 NaN, 2 +inf, 3 -inf, 0 finite"""
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def grad_ratio(k, r64, r32, s=None):
    """Elementwise rule  |k - r64| <= M * max(|r32 - r64|, u |r64|) + M u s   <=>   ratio <= M  with
    ratio = |k - r64| / (max(|r32 - r64|, u |r64|) + u s).
    Excluded from the ratio, and counted in `excluded` (the 2 % cap):
      * r64 not finite: the kernel must give the same class of non-finite value;
      * r64 finite, r32 not (fp32 autograd overflowed on its way): no fp32 yardstick - the kernel must be finite with the sign of r64;
      * the reference is DEGENERATE: r64 == r32 == 0 and every addend is 0 (s == 0) while the kernel returns a finite non-zero value -
        fp64 autograd cancels exactly (sigmoid(50) - 1, g_j - sum p_i g_i at the mode of a one-bin row) where the true value is ~1e-23;
        the kernel's value must then be below u max |r64| of the case, the fp32 resolution of the case's own gradients.  Rows that
        must be exactly zero (skipped labels, background, pad columns) are asserted exactly by the tests, not through this rule.
    -> dict(ratio: the worst ratio, excluded: fraction of excluded elements, class_ok, n, argmax)"""
    k, r64, r32 = _np(k), _np(r64), _np(r32)
    s = np.zeros_like(r64) if s is None else _np(s)
    assert k.shape == r64.shape == r32.shape == s.shape, (k.shape, r64.shape, r32.shape, s.shape)
    fin64 = np.isfinite(r64)
    no32 = fin64 & ~np.isfinite(r32)
    degen = fin64 & (r64 == 0) & (r32 == 0) & (s == 0) & (k != 0) & np.isfinite(k)
    floor = U * float(np.abs(r64[fin64]).max()) if fin64.any() else 0.0
    class_ok = bool(np.all(_cls(k[~fin64]) == _cls(r64[~fin64]))) and bool(np.all(np.isfinite(k[no32]) & (np.sign(k[no32]) == np.sign(r64[no32])))) \
        and bool(np.all(np.abs(k[degen]) <= floor))
    fin = fin64 & ~no32 & ~degen
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(k[fin] - r64[fin])
        den = np.maximum(np.abs(r32[fin] - r64[fin]), U * np.abs(r64[fin])) + U * np.where(np.isfinite(s[fin]), s[fin], 0.0)
        ratio = np.where(err == 0, 0.0, np.where(den > 0, err / den, np.inf))
        ratio = np.where(np.isnan(err), np.inf, ratio)   # the kernel is not finite where the reference is
    worst = float(ratio.max()) if ratio.size else 0.0
    return {"ratio": worst, "excluded": float((~fin).mean()) if fin.size else 0.0, "class_ok": class_ok, "n": int(fin.sum()),
            "argmax": int(np.flatnonzero(fin)[int(ratio.argmax())]) if ratio.size else -1}


def grad_ok(k, r64, r32, s, M, cap=0.02):
    res = grad_ratio(k, r64, r32, s)
    return res["ratio"] <= M and res["class_ok"] and res["excluded"] <= cap, res


def sum_bound(r64_terms, L, D, M):
    """|k - sum r64| <= (L + D + 2 M) u sum |r64_i|  -> (reference sum, bound)"""
    r = _np(r64_terms)
    return float(r.sum()), (L + D + 2 * M) * U * float(np.abs(r).sum())


# =================================================================================================
# input grids (fp32, CPU, seeded; the same values go to the kernel and, cast to fp64, to the reference)
# =================================================================================================
FOCAL_POINTS = [0.0, 1e-8, 1.0, 10.0, 20.0, 50.0, 87.0, 88.8, 100.0, 1e4]


def focal_edge_values():
    pts = torch.tensor([v for a in FOCAL_POINTS for v in ((a, -a) if a else (a,))], dtype=torch.float32)
    sw = torch.linspace(4.55, 4.66, 32, dtype=torch.float32)
    return torch.cat((pts, sw, -sw))                      # 19 + 64 values, both sides of the series switch at |x| = 4.605


def focal_case(P, C, seed, edge=True):
    """logits [P, C] / labels [P].  edge (P >= 2 E, E = the number of edge values): edge value i sits in the TARGET column of row i (a
    positive: label i % C) and in column i % C of row E + i, a background row (a negative) - and, for C > 1, in the next column of row i
    as well (a negative of a positive row); the rest is a seeded normal around the prior-bias initialisation -4.6 with labels -1
    (skipped), C (background) and valid.  Smaller P: the edge values fill the matrix in order.  not edge: N(0, 1), the golden-like grid."""
    g = torch.Generator().manual_seed(seed)
    if not edge:
        x = torch.randn((P, C), generator=g)
    else:
        x = torch.randn((P, C), generator=g) * 0.5 - 4.6
    labels = torch.randint(0, C, (P,), generator=g, dtype=torch.int32)
    if P > 2:
        labels[1::7] = -1
        labels[2::5] = C
    if edge:
        ev = focal_edge_values()
        E = ev.numel()
        if P >= 2 * E:
            for i in range(E):
                c = i % C
                labels[i], labels[E + i] = c, C
                x[i, c] = ev[i]
                x[E + i, c] = ev[i]
                if C > 1:
                    x[i, (c + 1) % C] = ev[i]
        else:
            flat = x.reshape(-1)
            n = min(flat.numel(), E)
            flat[:n] = ev[:n]
            labels[0] = 0
    return x.contiguous(), labels


def focal_edge_coverage(x, labels, C):
    """(edge values never met as a positive, never met as a negative of a live row)"""
    live = labels >= 0
    tgt = labels[:, None] == torch.arange(C)[None, :]
    posv, negv = x[tgt & live[:, None]], x[~tgt & live[:, None]]
    ev = focal_edge_values()
    return [float(v) for v in ev if not bool((posv == v).any())], [float(v) for v in ev if not bool((negv == v).any())]


def loc_case(P, BS, seed, edge=True, with_bvars=True, all_background=False):
    """box [P, BS], reg targets [P, 4], bvars [P, 4] | None, labels [P]; ts_cert = 0.5, ts_better = 0.1, 80 classes.  Integer targets only meet
    rows whose d is an exact integer in fp32 and fp64 (one bin at +60); the random rows draw targets n + 3/8, which a sharply peaked
    softmax (d within rounding of an integer) cannot tie with in one precision and miss in the other."""
    g = torch.Generator().manual_seed(seed)
    box = torch.zeros((P, BS))
    scale = torch.where(torch.arange(P) % 2 == 0, 1.0, 10.0)[:, None] if edge else torch.ones((P, 1))
    box[:, :68] = torch.randn((P, 68), generator=g) * scale
    tv = torch.tensor([1e-3, 0.5, 1.375, 3.375, 7.375, 12.375, 15.375, 15.99]) if edge else torch.tensor([0.75, 2.25, 5.5, 9.25])
    t = tv[torch.randint(0, len(tv), (P, 4), generator=g)]
    if not edge:
        t = t + torch.rand((P, 4), generator=g) * 0.125
        box[:, 68:72] = torch.randn((P, 4), generator=g)
        box[:, 72] = torch.randn(P, generator=g)
        bv = torch.randn((P, 4), generator=g) * 3
    else:
        sv = torch.tensor([0.0, 5.0, -5.0, 20.0, -20.0])
        box[:, 68:72] = sv[torch.randint(0, 5, (P, 4), generator=g)]
        box[:, 72] = torch.tensor([0.0, 50.0, -50.0, 1.5])[torch.randint(0, 4, (P,), generator=g)]
        bvv = torch.tensor([0.0, -3.0, 3.0, -8.0])     # ct = 1 - sigmoid: 0.5 exactly (== ts_cert: the strict > decides), 0.953, 0.047, 0.9997
        bv = bvv[torch.randint(0, 4, (P, 4), generator=g)]
        for r in range(P):
            k = r % 8
            if k == 1:      # one bin at +60: d is an exact integer in fp32 and fp64; integer targets: all four sides tie
                j = torch.randint(1, 16, (4,), generator=g)
                box[r, :68] = 0
                for b in range(4):
                    box[r, b * 17 + int(j[b])] = 60.0
                t[r] = j.float()
            elif k == 2:    # as above, no tie: d integer against other targets, l == r
                j = torch.randint(1, 16, (4,), generator=g)
                box[r, :68] = 0
                for b in range(4):
                    box[r, b * 17 + int(j[b])] = 60.0
                t[r] = torch.randint(1, 16, (4,), generator=g).float()   # integer targets: an accidental tie is exact in both precisions
                t[r, 2] = t[r, 0]
            elif k == 3:    # two adjacent bins equal: d = j + 1/2 exactly; half of these rows tie on it
                j = torch.randint(0, 15, (4,), generator=g)
                box[r, :68] = 0
                for b in range(4):
                    box[r, b * 17 + int(j[b])] = 60.0
                    box[r, b * 17 + int(j[b]) + 1] = 60.0
                if (r // 8) % 2 == 0:
                    t[r] = j.float() + 0.5
            elif k == 4:    # uniform logits: d = 8 (to rounding); extreme aspect ratio
                box[r, :68] = 0.25
                t[r] = torch.tensor([1e-3, 15.99, 15.99, 1e-3])
            elif k == 5:    # l == r and t == b: centerness target exactly 1
                t[r, 2] = t[r, 0]
                t[r, 3] = t[r, 1]
    labels = torch.randint(0, 80, (P,), generator=g, dtype=torch.int32)
    if all_background:
        labels[:] = 80
        labels[::3] = -1
    elif P > 2:
        labels[5::11] = -1
        labels[6::4] = 80
    return box.contiguous(), t.contiguous(), (bv.contiguous() if with_bvars else None), labels


def loc_clear_of_thresholds(box, t, bv, labels, ts_better=0.1, ts_cert=0.5, margin=1e-3):
    """True when no positive row of a RANDOM (not edge) case sits within `margin` of a branch threshold"""
    b = box.double()
    pos = (labels >= 0) & (labels != 80)
    d = (F.softmax(b[:, :68].reshape(-1, 17), dim=1) * torch.arange(17, dtype=torch.float64)).sum(1).reshape(-1, 4)
    ok = ((d - t.double()).abs() > margin) & (((d - t.double()).abs() - 1).abs() > margin)
    if bv is not None:
        cs, ct = 1 - torch.sigmoid(b[:, 68:72]), 1 - torch.sigmoid(bv.double())
        ok = ok & ((ct - ts_cert).abs() > margin) & ((ct - cs - ts_better).abs() > margin)
    return bool(ok[pos].all())


def benign_loc_case(P, BS, seed, with_bvars=True):
    for k in range(64):
        c = loc_case(P, BS, seed + 1000 * k, edge=False, with_bvars=with_bvars)
        if loc_clear_of_thresholds(*c):
            return c
    raise RuntimeError("no threshold-free draw")


def softmax_case(R, C, seed, edge=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, C), generator=g)
    tgt = torch.randint(0, C, (R,), generator=g, dtype=torch.int32)
    if edge:
        for r in range(R):
            k, tr = r % 8, int(tgt[r])
            if k == 1:
                tgt[r] = -1
            elif k in (2, 3, 4):      # the true class ahead of all others by exactly 0, 20, 40
                x[r] = torch.round(x[r])
                m = torch.cat((x[r, :tr], x[r, tr + 1:])).max() if C > 1 else x[r, tr]
                x[r, tr] = m + (0.0, 20.0, 40.0)[k - 2]
            elif k == 5:              # behind by 50: CE = 50
                x[r] = torch.round(x[r])
                m = torch.cat((x[r, :tr], x[r, tr + 1:])).max()
                x[r, tr] = m - 50.0
            elif k == 6:
                x[r] = x[r] + 1e4
    return x.contiguous(), tgt


def rpn_case(seed, N=3, hw=(12, 5), A=3, npos=9, nneg=23, G=4, edge=True, with_scores=True):
    """a dense case and the level-first head layout of the same numbers"""
    g = torch.Generator().manual_seed(seed)
    R = sum(hw) * A
    xy = torch.rand((R, 2), generator=g) * 64
    wh = torch.tensor([8.0, 16.0, 32.0])[torch.randint(0, 3, (R, 2), generator=g)]
    anchors = torch.cat((xy, xy + wh), dim=1)
    obj = torch.randn((N, R), generator=g) * (4.0 if edge else 1.0)
    deltas = torch.randn((N, R, 4), generator=g)
    gxy = torch.rand((N, G, 2), generator=g) * 64
    gt_boxes = torch.cat((gxy, gxy + 4 + torch.rand((N, G, 2), generator=g) * 40), dim=2)
    gt_scores = (torch.rand((N, G), generator=g) * 0.5 + 0.5) if with_scores else None
    matched = torch.randint(0, G, (N, R), generator=g, dtype=torch.int32)
    s = {"matched32": matched, "has_gt": torch.ones((N, 1), dtype=torch.uint8)}
    perm = torch.stack([torch.randperm(R, generator=g)[:npos + nneg] for _ in range(N)])
    s["pos_idx"], s["neg_idx"] = perm[:, :npos].contiguous(), perm[:, npos:].contiguous()
    s["pos_valid"] = torch.ones((N, npos), dtype=torch.uint8)
    s["neg_valid"] = torch.ones((N, nneg), dtype=torch.uint8)
    if edge:
        s["has_gt"][N - 1] = 0                                   # an image without gt
        s["pos_valid"][:, npos - 2:] = 0                         # empty sampling slots ...
        s["neg_valid"][:, nneg - 3:] = 0
        for n in range(N):                                       # ... whose index names a non-finite logit / delta
            obj[n, s["pos_idx"][n, npos - 1]] = float("nan")
            obj[n, s["neg_idx"][n, nneg - 1]] = float("inf")
            deltas[n, s["pos_idx"][n, npos - 2]] = float("-inf")
        obj[0, s["pos_idx"][0, 0]] = 30.0                        # saturation on both sides of both targets
        obj[0, s["pos_idx"][0, 1]] = -30.0
        obj[0, s["neg_idx"][0, 0]] = 90.0
        obj[0, s["neg_idx"][0, 1]] = -90.0
        obj[0, s["neg_idx"][0, 2]] = 0.0
        # a delta exactly equal to its target: gt == anchor -> all four targets are 0 in any precision
        r0, g0 = int(s["pos_idx"][0, 2]), int(matched[0, s["pos_idx"][0, 2]])
        gt_boxes[0, g0] = anchors[r0]
        deltas[0, r0] = 0.0
        deltas[0, r0, 1] = 0.5
    ch = 5 * A + 1    # one pad column: ch > 5 A is legal
    head = torch.zeros((N * sum(hw), ch))
    for n in range(N):
        for r in range(R):
            oo, od = rpn_head_offsets(hw, N, A, ch, n, r)
            head.view(-1)[oo] = obj[n, r]
            head.view(-1)[od:od + 4] = deltas[n, r]
    return {"N": N, "hw": list(hw), "A": A, "R": R, "ch": ch, "anchors": anchors.contiguous(), "obj": obj.contiguous(),
            "deltas": deltas.contiguous(), "head": head, "gt_boxes": gt_boxes.contiguous(), "gt_scores": gt_scores, "s": s,
            "weights": (1.0, 1.0, 1.0, 1.0)}


def rpn_slot_inputs(c, dtype):
    """the logits / deltas of the sampling slots (what the reference sees): finite placeholders on slots that carry no weight"""
    s = c["s"]
    idx = torch.cat((s["pos_idx"], s["neg_idx"]), dim=1)
    valid = torch.cat((s["pos_valid"], s["neg_valid"]), dim=1).bool()
    x = torch.gather(c["obj"], 1, idx)
    x = torch.where(valid, x, torch.zeros(())).to(dtype)
    dl = torch.gather(c["deltas"], 1, s["pos_idx"][..., None].expand(-1, -1, 4))
    dl = torch.where((s["pos_valid"].bool() & s["has_gt"].bool())[..., None], dl, torch.zeros(())).to(dtype)
    return x, dl


ROI_W, ROI_CLAMP = (10.0, 5.0), 62.5


def roi_case(R, seed, edge=True):
    """deltas / std are the column slices [0:4] / [4:8] of one [R, 8] matrix: used as they are (row pitch ld = 8) or as contiguous copies (ld = 4)"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.round(torch.rand((R, 2), generator=g) * 100)
    wh = torch.tensor([16.0, 32.0, 64.0])[torch.randint(0, 3, (R, 2), generator=g)]
    prop = torch.cat((xy, xy + wh), dim=1)
    gtb = prop + torch.round(torch.randn((R, 4), generator=g) * 3)
    gtb[:, 2:] = torch.max(gtb[:, 2:], gtb[:, :2] + 4)
    deltas = torch.randn((R, 4), generator=g) * 0.5
    std = torch.randn((R, 4), generator=g)
    gstd = torch.tensor([0.0, -3.0, 3.0, -8.0])[torch.randint(0, 4, (R, 4), generator=g)] if edge else torch.randn((R, 4), generator=g) * 3
    cls = torch.randint(0, 80, (R,), generator=g, dtype=torch.int64)
    if edge:
        std = torch.tensor([0.0, 5.0, -5.0, 20.0, -20.0, 1.0])[torch.randint(0, 6, (R, 4), generator=g)]
        for r in range(R):
            k = r % 10
            if k == 1:
                cls[r] = -1
            elif k == 2:      # background; std logit -90: sigma^2 underflows, the loss must stay finite
                cls[r] = 80
                std[r] = -90.0
            elif k == 3:      # gt == proposal, zero deltas: four ties, IoU 1
                gtb[r] = prop[r]
                deltas[r] = 0.0
            elif k == 4:      # the decoded box is disjoint from the gt
                gtb[r] = prop[r] + 500.0
                deltas[r] = 0.0
            elif k == 5:      # the decoded box touches the gt: rbx - ltx == 0
                deltas[r] = 0.0
                w = prop[r, 2] - prop[r, 0]
                gtb[r] = torch.stack((prop[r, 2], prop[r, 1], prop[r, 2] + w, prop[r, 3]))
            elif k == 6:      # one side at d / w == -+scale_clamp exactly (625 / 10 and 312.5 / 5 are exact): the box grows, the IoU still
                j = (r // 10) % 4   # depends on that side, so the derivative of the clamp AT its bound decides the gradient
                deltas[r, j] = (-625.0, 625.0, -312.5, 312.5)[j]
            elif k == 7:      # ... and beyond the bound
                j = (r // 10) % 4
                deltas[r, j] = (-626.0, 700.0, -313.0, 400.0)[j]
    m = torch.cat((deltas, std), dim=1).contiguous()
    return {"mat": m, "cls": cls, "prop": prop.contiguous(), "gtb": gtb.contiguous(), "gstd": gstd.contiguous()}


def roi_branches(c, dtype, wx=ROI_W[0], wy=ROI_W[1], clamp=ROI_CLAMP):
    """the branch decisions of roi_box_loss mode 0 on the foreground rows, evaluated in `dtype`: signs of v -+ clamp, px1 - gb.x,
    px2 - gb.z, py1 - gb.y, py2 - gb.w, rbx - ltx, rby - lty and of d - t"""
    fg = (c["cls"] >= 0) & (c["cls"] < 80)
    d, pb, gb = c["mat"][fg, :4].to(dtype), c["prop"][fg].to(dtype), c["gtb"][fg].to(dtype)
    w, h = pb[:, 2] - pb[:, 0], pb[:, 3] - pb[:, 1]
    v = torch.stack((d[:, 0] / wx, d[:, 1] / wx, d[:, 2] / wy, d[:, 3] / wy), dim=1)
    q = torch.clamp(v, min=-clamp, max=clamp)
    px1, px2, py1, py2 = q[:, 0] * w + pb[:, 0], q[:, 1] * w + pb[:, 2], q[:, 2] * h + pb[:, 1], q[:, 3] * h + pb[:, 3]
    sw, sh = w + 1.0, h + 1.0
    t = torch.stack((wx * (gb[:, 0] - pb[:, 0]) / sw, wx * (gb[:, 2] - pb[:, 2]) / sw, wy * (gb[:, 1] - pb[:, 1]) / sh,
                     wy * (gb[:, 3] - pb[:, 3]) / sh), dim=1)
    cols = [torch.sign(v - clamp), torch.sign(v + clamp), torch.sign(d - t),
            torch.sign(torch.stack((px1 - gb[:, 0], px2 - gb[:, 2], py1 - gb[:, 1], py2 - gb[:, 3],
                                    torch.min(gb[:, 2], px2) - torch.max(gb[:, 0], px1), torch.min(gb[:, 3], py2) - torch.max(gb[:, 1], py1)), dim=1))]
    return torch.cat(cols, dim=1).double()
