"""Plain reference of the DECISION kernels (box <-> gt matching, the RPN / ROI samplers, FCOS target assignment, NMS, the ragged top-k and
the RPN decode) on inputs for which fp32 is exact, and the branch cases that put an input exactly on every comparison of those kernels.

Every coordinate is an integer with |c| <= 1024, so every difference, product and sum the kernels form (sides <= 2048, areas <= 2^22,
unions <= 2^23) is exact in fp32 and the geometry can be done in Python ints / fractions.Fraction.  The only inexact operation is the one
IEEE division of an IoU, np.float32(inter) / np.float32(union), and a threshold is np.float32(thr) - what torch does for a float32 tensor
against a Python scalar.  Hence no tolerance: the tests compare integers, bytes and fp32 bit patterns.

Nothing here calls the project's oracle or a torch op; tests/test_assign_ref.py holds the two against each other on the CPU.  Each case
builder returns its inputs and a CENSUS - how often the inputs hit each decision point, counted in exact arithmetic - so that a case
that stops hitting its branch fails on the CPU.  `flipped(rule)` turns one comparison of the reference into its neighbour (> into >=,
first-wins into last-wins): the CPU test shows that every such flip changes the expected output of some case, i.e. the same one-token
change in a kernel cannot pass tests/test_assign_exact_gpu.py."""
import contextlib
from fractions import Fraction

import numpy as np

F32 = np.float32
LIMIT = 1024
INF = 100000000.0

_FLIPPED = set()
FLIPS = ("match_first", "rpn_hi", "rpn_lo", "roi_thr", "fcos_inside", "fcos_soi_hi", "fcos_soi_lo", "fcos_first", "nms_thr", "decode_min")


@contextlib.contextmanager
def flipped(rule):
    assert rule in FLIPS
    _FLIPPED.add(rule)
    try:
        yield
    finally:
        _FLIPPED.discard(rule)


def _gt(a, b, rule):
    """a > b (flipped: a >= b)"""
    return a >= b if rule in _FLIPPED else a > b


def _ge(a, b, rule):
    """a >= b (flipped: a > b)"""
    return a > b if rule in _FLIPPED else a >= b


def _lt(a, b, rule):
    """a < b (flipped: a <= b)"""
    return a <= b if rule in _FLIPPED else a < b


def _le(a, b, rule):
    """a <= b (flipped: a < b)"""
    return a < b if rule in _FLIPPED else a <= b


# ---------------------------------------------------------------------------------------------------------------------------------
# precondition
def int_boxes(boxes, limit=LIMIT):
    """[..., 4] array -> list of (x0, y0, x1, y1) Python ints; ValueError outside the exact domain"""
    a = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if not np.all(np.isfinite(a)) or np.any(a != np.round(a)):
        raise ValueError("assign_ref: box coordinates must be integers")
    if np.any(np.abs(a) > limit):
        raise ValueError("assign_ref: box coordinates must lie in [-%d, %d]" % (limit, limit))
    if np.any(a[:, 2] < a[:, 0]) or np.any(a[:, 3] < a[:, 1]):
        raise ValueError("assign_ref: x1 >= x0 and y1 >= y0")
    return [tuple(int(v) for v in r) for r in a]


def iou_parts(a, b):
    """(intersection, union) of two integer boxes, as ints"""
    w = max(min(a[2], b[2]) - max(a[0], b[0]), 0)
    h = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    inter = w * h
    return inter, (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter


def iou(a, b):
    """D2 pairwise_iou rule: inter > 0 ? inter / (area_a + area_b - inter) : 0 - one correctly rounded fp32 division"""
    inter, union = iou_parts(a, b)
    return F32(inter) / F32(union) if inter > 0 else F32(0)


def iou_exact(a, b):
    inter, union = iou_parts(a, b)
    return Fraction(inter, union) if inter > 0 else Fraction(0)


def pairwise_iou(a, b):
    A, B = int_boxes(a), int_boxes(b)
    return np.array([[iou(x, y) for y in B] for x in A], dtype=F32).reshape(len(A), len(B))


# ---------------------------------------------------------------------------------------------------------------------------------
# matcher
def match(boxes, gt_boxes, gt_valid):
    """one image: max IoU per box over the valid gts in slot order (first gt attaining it wins; the argument is the SLOT), -1 / 0 when
    no gt is valid; gt_max [G] per gt (0 for an invalid slot)"""
    B, Gs = int_boxes(boxes), int_boxes(gt_boxes)
    slots = [g for g in range(len(Gs)) if gt_valid[g]]
    mx = np.full(len(B), -1, dtype=F32)
    arg = np.zeros(len(B), dtype=np.int32)
    gmax = np.zeros(len(Gs), dtype=F32)
    for p, b in enumerate(B):
        best, bi = F32(-1), 0
        for g in slots:
            v = iou(Gs[g], b)
            if _gt(v, best, "match_first"):
                best, bi = v, g
            if v > gmax[g]:
                gmax[g] = v
        mx[p], arg[p] = best, bi
    return mx, arg, gmax


def lowq(boxes, gt_boxes, gt_valid, gmax):
    """box p is marked when iou(g, p) == gt_max[g] for some valid g (D2 set_low_quality_matches_, with its quirk: a gt no box overlaps
    has gt_max 0 and marks every box that has IoU 0 with it)"""
    B, Gs = int_boxes(boxes), int_boxes(gt_boxes)
    slots = [g for g in range(len(Gs)) if gt_valid[g]]
    return np.array([int(any(iou(Gs[g], b) == gmax[g] for g in slots)) for b in B], dtype=np.uint8)


def match_census(boxes, gt_boxes, gt_valid, marks=(Fraction(7, 10), Fraction(3, 10), Fraction(1, 2))):
    B, Gs = int_boxes(boxes), int_boxes(gt_boxes)
    slots = [g for g in range(len(Gs)) if gt_valid[g]]
    c = dict(iou_eq_7_10=0, iou_eq_3_10=0, iou_eq_1_2=0, iou_one=0, argmax_tie=0, gt_untouched=0, zero_area_gt=0, zero_area_box=0,
             n_valid=len(slots), max_only_at_last=0)
    names = dict(zip(marks, ("iou_eq_7_10", "iou_eq_3_10", "iou_eq_1_2")))
    area = lambda b: (b[2] - b[0]) * (b[3] - b[1])
    c["zero_area_gt"] = sum(area(Gs[g]) == 0 for g in slots)
    c["zero_area_box"] = sum(area(b) == 0 for b in B)
    for b in B:
        vals = [iou_exact(Gs[g], b) for g in slots]
        if not vals:
            continue
        m = max(vals)
        if m in names:
            c[names[m]] += 1
        c["iou_one"] += m == 1
        c["argmax_tie"] += m > 0 and vals.count(m) > 1
    for g in slots:
        vals = [iou_exact(Gs[g], b) for b in B]
        m = max(vals)
        c["gt_untouched"] += m == 0
        c["max_only_at_last"] += m > 0 and vals.count(m) == 1 and vals[-1] == m
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# samplers
def _by_key(idx, keys):
    return sorted(idx, key=lambda i: (float(keys[i]), i))


def rpn_labels_and_sample(mx, lq, has_gt, keys, lo, hi, npos_max, batch):
    """one image.  v < lo: negative; v >= hi or low-quality match: positive; else ignored; an image without gt: all negative.  The
    npos_max smallest keys of the positives (equal keys in index order), then negatives fill batch - npos.
    -> labels int8 [R], pos_idx / pos_valid [npos_max], neg_idx / neg_valid [batch] (idx 0 where not valid)"""
    R = len(mx)
    lo32, hi32 = F32(lo), F32(hi)
    labels = np.zeros(R, dtype=np.int8)
    for r in range(R):
        v = F32(mx[r])
        lab = 0 if _lt(v, lo32, "rpn_lo") else -1
        if _ge(v, hi32, "rpn_hi"):
            lab = 1
        if lq[r]:
            lab = 1
        if not has_gt:
            lab = 0
        labels[r] = lab
    pos = _by_key([r for r in range(R) if labels[r] == 1], keys)[:npos_max]
    neg = _by_key([r for r in range(R) if labels[r] == 0], keys)[:max(batch - len(pos), 0)]
    pos_idx, pos_valid = np.zeros(npos_max, dtype=np.int64), np.zeros(npos_max, dtype=np.uint8)
    neg_idx, neg_valid = np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.uint8)
    pos_idx[:len(pos)], pos_valid[:len(pos)] = pos, 1
    neg_idx[:len(neg)], neg_valid[:len(neg)] = neg, 1
    return labels, pos_idx, pos_valid, neg_idx, neg_valid


def roi_sample(boxes, valid, mx, arg, keys, gt_boxes, gt_classes, gt_valid, gt_scores, gt_std, thr, num_classes, B, nfg_max):
    """one image.  Foreground = has_gt and v >= thr (and the matched class is not the background id); foreground first, each group in
    ascending (key, slot) order, capped by nfg_max / B; an empty slot carries class -1 and zeros."""
    P = len(mx)
    has_gt = bool(np.any(gt_valid))
    thr32 = F32(thr)
    cls = {}
    for i in range(P):
        if valid[i]:
            fg = has_gt and _ge(F32(mx[i]), thr32, "roi_thr")
            cls[i] = int(gt_classes[arg[i]]) if fg else num_classes
    fg = _by_key([i for i in cls if cls[i] != num_classes], keys)[:nfg_max]
    bg = _by_key([i for i in cls if cls[i] == num_classes], keys)[:B - len(fg)]
    out = dict(proposal_boxes=np.zeros((B, 4), F32), gt_classes=np.full(B, -1, np.int64), gt_boxes=np.zeros((B, 4), F32),
               valid=np.zeros(B, np.uint8), sampled_idx=np.zeros(B, np.int64), gt_confid=np.zeros(B, F32),
               gt_loc_std=np.zeros((B, 4), F32))
    for j, i in enumerate(fg + bg):
        out["proposal_boxes"][j] = boxes[i]
        out["gt_classes"][j] = cls[i]
        out["valid"][j] = 1
        out["sampled_idx"][j] = i
        if has_gt:
            out["gt_boxes"][j] = gt_boxes[arg[i]]
            out["gt_confid"][j] = gt_scores[arg[i]]
            out["gt_loc_std"][j] = gt_std[arg[i]]
    out["nfg"] = len(fg)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# FCOS targets
def fcos_locations(level_hw, strides):
    """[(level, x, y)] of every location, level-first, rows then columns: x = column * stride + stride // 2"""
    out = []
    for l, ((h, w), s) in enumerate(zip(level_hw, strides)):
        out += [(l, x * s + s // 2, y * s + s // 2) for y in range(h) for x in range(w)]
    return out


def _fcos_image(locs, strides, soi, boxes, classes, valid, std, num_classes, drop_empty, radius, census):
    """one active image -> per location (label, reg [4], bvar [4], gt slot)"""
    slots = [g for g in range(len(boxes)) if valid[g]]
    L = len(locs)
    if not slots:
        census["empty_images"] += 1
        return [((-1 if drop_empty & 1 else num_classes), [0.0] * 4, [0.0] * 4, -1)] * L
    area = {g: (boxes[g][2] - boxes[g][0]) * (boxes[g][3] - boxes[g][1]) for g in slots}
    rad = Fraction(radius)
    first = boxes[slots[0]]
    cs_none = rad > 0 and first[0] + first[2] == 0          # the reference's `center_x[..., 0].sum() == 0`
    census["cs_quirk_images"] += cs_none
    rows = []
    for (l, xs, ys) in locs:
        s = strides[l]
        lo, hi = soi[l]
        best, bi = None, slots[0]
        inside_any = sampled_any = False
        cand_areas = []
        for g in slots:
            b = boxes[g]
            ltrb = (xs - b[0], ys - b[1], b[2] - xs, b[3] - ys)
            mn_box, mxv = min(ltrb), max(ltrb)
            mn = mn_box
            inside_any |= mn_box > 0
            if rad > 0:
                cx, cy, sr = Fraction(b[0] + b[2], 2), Fraction(b[1] + b[3], 2), rad * s
                x0, y0 = max(cx - sr, b[0]), max(cy - sr, b[1])
                x1, y1 = min(cx + sr, b[2]), min(cy + sr, b[3])
                mn_sq = min(xs - (cx - sr), ys - (cy - sr), cx + sr - xs, cy + sr - ys)
                mn = Fraction(-1) if cs_none else min(xs - x0, ys - y0, x1 - xs, y1 - ys)
                if not cs_none:
                    census["cs_on_radius"] += mn == 0 and mn_box > 0 and mn_sq == 0
                    census["cs_clipped"] += mn_sq > 0 and mn <= 0
            sampled_any |= mn > 0
            ins = _gt(mn, 0, "fcos_inside")
            cared = _ge(mxv, lo, "fcos_soi_lo") and _le(mxv, hi, "fcos_soi_hi")
            census["on_edge"] += mn == 0 and lo <= mxv <= hi and rad == 0
            census["one_inside"] += mn == 1 and lo <= mxv <= hi
            census["mx_eq_soi_lo"] += mn > 0 and mxv == lo
            census["mx_eq_soi_hi"] += mn > 0 and mxv == hi
            census["mx_below_soi_lo"] += mn > 0 and mxv == lo - 1
            census["mx_above_soi_hi"] += mn > 0 and mxv == hi + 1
            if mn > 0 and not (lo <= mxv <= hi):
                cand_areas.append(("uncared", area[g]))
            if ins and cared:
                if mn > 0 and lo <= mxv <= hi:
                    cand_areas.append(("cared", area[g]))
                if best is None or _lt(area[g], best, "fcos_first"):
                    best, bi = area[g], g
        cared_a = [a for k, a in cand_areas if k == "cared"]
        if cared_a:
            census["area_tie"] += cared_a.count(min(cared_a)) > 1
            census["smaller_uncared"] += any(k == "uncared" and a < min(cared_a) for k, a in cand_areas)
        bg = best is None
        ignored = bool(drop_empty & 2) and inside_any and not sampled_any
        census["ignored"] += ignored
        census["positive"] += (not bg) and not ignored
        b = boxes[bi]
        reg = [float(Fraction(v, s)) for v in (xs - b[0], ys - b[1], b[2] - xs, b[3] - ys)]
        bv = [99999.0] * 4 if bg else [float(v) for v in std[bi]]
        rows.append((-1 if ignored else num_classes if bg else int(classes[bi]), reg, bv, bi))
    return rows


FCOS_CENSUS = ("empty_images", "inactive_images", "cs_quirk_images", "cs_on_radius", "cs_clipped", "on_edge", "one_inside", "mx_eq_soi_lo",
               "mx_eq_soi_hi", "mx_below_soi_lo", "mx_above_soi_hi", "area_tie", "smaller_uncared", "ignored", "positive")


def fcos_targets(level_hw, strides, soi, gt_boxes, gt_classes, gt_valid, gt_std, num_classes, drop_empty, active=None, center_radius=0.0,
                 batch=None, img0=0):
    """the contract of ubteacher.hip.fcos_targets: level-first rows p = batch * level_off + n * HW_l + hw.
    -> labels int32 [P], reg_targets f32 [P, 4], bvars f32 [P, 4], gt_inds int32 [P], census"""
    n_gt, MAXG = np.asarray(gt_classes).shape
    N = n_gt if batch is None else int(batch)
    if float(F32(center_radius)) != center_radius or any((Fraction(center_radius) * s * 2).denominator != 1 for s in strides):
        raise ValueError("assign_ref: radius * stride must be a multiple of 1/2")
    for s in strides:
        if s & (s - 1):
            raise ValueError("assign_ref: strides must be powers of two")
    locs = fcos_locations(level_hw, strides)
    L = len(locs)
    census = dict.fromkeys(FCOS_CENSUS, 0)
    per_image = []
    for n in range(N):
        gi = n - img0
        if not (0 <= gi < n_gt) or (active is not None and not active[n]):
            census["inactive_images"] += 1
            per_image.append([(-1, [0.0] * 4, [0.0] * 4, -1)] * L)
            continue
        boxes = int_boxes(gt_boxes[gi])
        std = gt_std[gi] if gt_std is not None else np.zeros((MAXG, 4))
        per_image.append(_fcos_image(locs, strides, soi, boxes, gt_classes[gi], gt_valid[gi], std, num_classes, drop_empty,
                                     center_radius, census))
    labels, reg, bv, ginds = [], [], [], []
    off = 0
    for (h, w) in level_hw:
        for n in range(N):
            for r in per_image[n][off:off + h * w]:
                labels.append(r[0]); reg.append(r[1]); bv.append(r[2]); ginds.append(r[3])
        off += h * w
    return (np.array(labels, np.int32), np.array(reg, F32).reshape(-1, 4), np.array(bv, F32).reshape(-1, 4), np.array(ginds, np.int32),
            census)


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS
def nms(boxes, scores, classes, valid, thr, class_aware, post_topk=-1, max_out=None):
    """one image -> (kept slots in (score desc, slot asc) order, census).  Suppression when iou > thr (strict; 0 / 0 suppresses
    nothing); class-aware = torchvision's coordinate trick box + cls * (max_coord + 1) over the valid boxes; max_out truncates; then
    the kthvalue rule: with more than post_topk kept, keep every kept slot whose score >= the post_topk-th kept score."""
    M = len(scores)
    vs = [i for i in range(M) if valid[i]]
    raw = int_boxes(boxes)
    sc = [float(F32(s)) for s in scores]
    census = dict(iou_eq_thr=0, score_tie=0, suppressed=0, zero_sign_tie=0, n_valid=len(vs))
    if not vs:
        return [], census
    if class_aware:
        off1 = max(max(raw[i]) for i in vs) + 1
        bx = {i: tuple(c + int(classes[i]) * off1 for c in raw[i]) for i in vs}
        if max(max(abs(c) for c in b) for b in bx.values()) > (1 << 22):
            raise ValueError("assign_ref: cls * (max_coord + 1) + coord must stay within 2^22")
    else:
        bx = {i: raw[i] for i in vs}
    order = sorted(vs, key=lambda i: (-sc[i], i))        # -0.0 == +0.0: the slot decides
    census["score_tie"] = sum(sc[a] == sc[b] for a, b in zip(order, order[1:]))
    census["zero_sign_tie"] = sum(sc[a] == 0 and sc[b] == 0 and np.signbit(F32(scores[a])) != np.signbit(F32(scores[b]))
                                  for a, b in zip(order, order[1:]))
    thr32, thrq = F32(thr), Fraction(thr).limit_denominator(1000)
    removed, keep = set(), []
    for ii, i in enumerate(order):
        if i in removed:
            continue
        keep.append(i)
        for j in order[ii + 1:]:
            inter, union = iou_parts(bx[i], bx[j])
            if union == 0:
                continue
            census["iou_eq_thr"] += j not in removed and Fraction(inter, union) == thrq
            if _gt(F32(inter) / F32(union), thr32, "nms_thr"):
                removed.add(j)
    census["suppressed"] = len(removed)
    census["kept_all"] = len(keep)
    if max_out is not None:
        keep = keep[:max_out]
    if post_topk > 0 and len(keep) > post_topk:
        kth = sc[keep[post_topk - 1]]
        keep = [i for i in keep if sc[i] >= kth]
    return keep, census


# ---------------------------------------------------------------------------------------------------------------------------------
# top-k and the RPN decode
def topk_rows(keys_flat, row_off, k):
    """the k largest non-negative keys of each ragged row, descending, padded with -1"""
    keys_flat = np.asarray(keys_flat, dtype=np.int64)
    out = np.full((len(row_off) - 1, k), -1, dtype=np.int64)
    for r in range(len(row_off) - 1):
        row = keys_flat[row_off[r]:row_off[r + 1]]
        c = np.sort(row[row >= 0])[::-1][:k]
        out[r, :len(c)] = c
    return out


def rpn_rank_keys(head, hw, N, A):
    """sortable key of every objectness logit of the level-first head output [sum_l N * hw_l, ch], in memory order: (monotone image of
    the logit's bits) * 2^31 + (2^31 - 1 - anchor index inside the (level, image) row)"""
    head = np.asarray(head, dtype=F32)
    out, row0 = [], 0
    for n_pix in hw:
        for n in range(N):
            for p in range(n_pix):
                for a in range(A):
                    bits = int(head[row0 + n * n_pix + p, a].view(np.int32))
                    mono = (bits ^ 0x7FFFFFFF if bits < 0 else bits) + (1 << 31)
                    out.append(mono * (1 << 31) + ((1 << 31) - 1 - (p * A + a)))
        row0 += N * n_pix
    return np.array(out, dtype=np.int64)


def _exact32(q, what):
    if F32(float(q)) != q or Fraction(float(F32(float(q)))) != q:
        raise ValueError("assign_ref: %s = %s is not an fp32 number" % (what, q))
    return q


def rpn_decode(top, head, anchors, image_hw, hw, ks, N, A, min_size):
    """Box2BoxTransform.apply_deltas with weights 1 and dw = dh = 0 (so exp(0) = 1 and every step is exact - asserted), clip to
    [0, W] x [0, H], keep iff finite and w > min_size and h > min_size (strict); an empty key (< 0) gives zeros and keep 0.
    -> boxes f32 [N, K, 4] (NaN where a delta is NaN), scores [N, K], lvls int32 [N, K], keep u8 [N, K], census"""
    head = np.asarray(head, dtype=F32)
    anc = np.asarray(anchors, dtype=F32)
    K = int(sum(ks))
    boxes, scores = np.zeros((N, K, 4), F32), np.zeros((N, K), F32)
    lvls, keep = np.zeros((N, K), np.int32), np.zeros((N, K), np.uint8)
    census = dict(empty=0, nonfinite=0, w_eq_min=0, w_min_plus1=0, clip_hi=0, clip_lo=0, kept=0)
    ms = Fraction(float(F32(min_size)))
    row0 = anchor0 = out0 = 0
    for l, (n_pix, k) in enumerate(zip(hw, ks)):
        for n in range(N):
            H, W = (Fraction(float(v)) for v in image_hw[n])
            for j in range(k):
                o = out0 + j
                lvls[n, o] = l
                key = int(top[l * N + n, j])
                if key < 0:
                    census["empty"] += 1
                    continue
                idx = (1 << 31) - 1 - (key & ((1 << 31) - 1))
                p, a = divmod(idx, A)
                row = head[row0 + n * n_pix + p]
                sc, d = row[a], row[A + 4 * a:A + 4 * a + 4]
                if d[2] != 0 or d[3] != 0:
                    raise ValueError("assign_ref: the decode is exact only with dw = dh = 0")
                an = [Fraction(float(v)) for v in anc[anchor0 + idx]]
                w, h = an[2] - an[0], an[3] - an[1]
                cx, cy = an[0] + w / 2, an[1] + h / 2
                ctr = []
                for dv, side, c in ((d[0], w, cx), (d[1], h, cy)):
                    if np.isfinite(dv):
                        _exact32(Fraction(float(dv)) * side, "delta * side")
                        ctr.append(_exact32(Fraction(float(dv)) * side + c, "centre"))
                    else:
                        ctr.append(None)
                finite = bool(np.isfinite(sc)) and None not in ctr
                census["nonfinite"] += not finite
                raw = [None if ctr[0] is None else ctr[0] - w / 2, None if ctr[1] is None else ctr[1] - h / 2,
                       None if ctr[0] is None else ctr[0] + w / 2, None if ctr[1] is None else ctr[1] + h / 2]
                clipped = []
                for e, v in enumerate(raw):
                    if v is None:
                        clipped.append(None)
                        continue
                    _exact32(v, "corner")
                    bound = W if e % 2 == 0 else H
                    census["clip_lo"] += v < 0
                    census["clip_hi"] += v > bound
                    clipped.append(min(max(v, Fraction(0)), bound))
                boxes[n, o] = [np.nan if v is None else float(v) for v in clipped]
                scores[n, o] = sc if finite else 0
                if finite:
                    bw, bh = clipped[2] - clipped[0], clipped[3] - clipped[1]
                    census["w_eq_min"] += bw == ms or bh == ms
                    census["w_min_plus1"] += min(bw, bh) == ms + 1
                    keep[n, o] = _gt(bw, ms, "decode_min") and _gt(bh, ms, "decode_min")
                    census["kept"] += int(keep[n, o])
        row0 += N * n_pix
        anchor0 += n_pix * A
        out0 += k
    return boxes, scores, lvls, keep, census


# =================================================================================================================================
# Branch cases.  Anchors / proposals are 10 x 10 squares on a 20-pitch grid, 17 to a row, so a box touches only the cells it is
# aimed at; index i sits at column i % 17, row i // 17.
def grid_boxes(P, x0=-200, y0=-200, side=10, pitch=20, per_row=17):
    return np.array([[x0 + pitch * (i % per_row), y0 + pitch * (i // per_row), x0 + pitch * (i % per_row) + side,
                      y0 + pitch * (i // per_row) + side] for i in range(P)], dtype=F32)


def _pad_gts(rows, G):
    """rows: list of (slot, box) -> boxes [G, 4] (every other slot holds a POISON box equal to cell 0: IoU 1 if its valid byte were
    ignored), valid [G]"""
    gb = np.tile(grid_boxes(1)[0], (G, 1)).astype(F32)
    gv = np.zeros(G, dtype=np.uint8)
    for slot, box in rows:
        gb[slot], gv[slot] = box, 1
    return gb, gv


def _cell(i, dx0=0, dy0=0, dx1=0, dy1=0):
    b = grid_boxes(i + 1)[i]
    return [b[0] + dx0, b[1] + dy0, b[2] + dx1, b[3] + dy1]


def matcher_threshold_case():
    """seven images over 40 shared anchors (anchor 39 has zero area), G = 4.
    0: IoU exactly 7/10, 3/10, 1/2 and 1 on anchors 0, 1, 2, 3.     1: two gts with IoU 6/10 on anchor 5 (slots 0, 1).
    2: the same pair behind a hole (slots 1, 2; slot 0 a poison).     3: a gt no anchor touches (+ one that matches anchor 7).
    4: a zero-area gt (+ one that matches anchor 8).                  5: no valid gt.       6: per-gt maxima shared by two anchors."""
    P, G = 40, 4
    anchors = grid_boxes(P)
    anchors[39, 2] = anchors[39, 0]
    imgs = [
        [(0, _cell(0, dy1=-3)), (1, _cell(1, dy1=-7)), (2, _cell(2, dy1=-5)), (3, _cell(3))],
        [(0, _cell(5, dy1=-4)), (1, _cell(5, dy0=4))],
        [(1, _cell(5, dy1=-4)), (2, _cell(5, dy0=4))],
        [(0, [900, 900, 950, 950]), (2, _cell(7, dx1=-2))],
        [(1, [3, 5, 3, 9]), (3, _cell(8, dx1=-2))],
        [],
        [(0, [_cell(10)[0] + 5, _cell(10)[1], _cell(11)[0] + 5, _cell(11)[3]])],
    ]
    packed = [_pad_gts(rows, G) for rows in imgs]
    gb = np.stack([p[0] for p in packed])
    gv = np.stack([p[1] for p in packed])
    census = [match_census(anchors, gb[n], gv[n]) for n in range(len(imgs))]
    return dict(boxes=anchors, gt_boxes=gb, gt_valid=gv), census


WAVE_SLOTS = (63, 64, 127, 128, 255)


def matcher_boundary_case(G, P, per_image):
    """two images; valid gt slots only at the wave boundaries 63, 64, 127, 128, 255 (those below G; slot 0 for G = 1); every other slot
    a poison.  The j-th valid gt of image 0 covers the LAST anchor with IoU (10 - j) / 10 (even j) or 2/5 and its left neighbour with
    1/6 (odd j): its maximum is attained by the last anchor alone.  Image 1 uses the valid slots in reverse and aims at anchor 0.
    per_image: image 1 matches its own boxes [N, P, 4], shifted by (3, 1)."""
    slots = [s for s in WAVE_SLOTS if s < G] or [0]
    anchors = grid_boxes(P)
    last = [float(v) for v in anchors[P - 1]]
    rows0 = []
    for j, s in enumerate(slots):
        rows0.append((s, [last[0] - 15, last[1], last[2], last[3]] if j % 2 else [last[0], last[1], last[2], last[3] - j]))
    rows1 = [(s, _cell(0, dx1=-j)) for j, s in enumerate(reversed(slots))]
    packed = [_pad_gts(rows0, G), _pad_gts(rows1, G)]
    gb, gv = np.stack([p[0] for p in packed]), np.stack([p[1] for p in packed])
    boxes = anchors
    if per_image:
        boxes = np.stack([anchors, anchors + np.array([3, 1, 3, 1], dtype=F32)])
    census = [match_census(boxes[n] if per_image else boxes, gb[n], gv[n]) for n in range(2)]
    return dict(boxes=boxes, gt_boxes=gb, gt_valid=gv), census


def random_int_boxes(rng, n, span=60, sizes=(6, 10, 12, 20)):
    xy = rng.integers(0, span, size=(n, 2))
    wh = rng.choice(sizes, size=(n, 2))
    return np.concatenate([xy, xy + wh], axis=1).astype(F32)


def match_all(boxes, gt_boxes, gt_valid):
    """batched match + lowq: boxes [P, 4] shared or [N, P, 4] -> mx [N, P], arg [N, P], gmax [N, G], lowq [N, P]"""
    N = len(gt_valid)
    out = [[], [], [], []]
    for n in range(N):
        b = boxes if np.ndim(boxes) == 2 else boxes[n]
        mx, arg, gm = match(b, gt_boxes[n], gt_valid[n])
        for dst, v in zip(out, (mx, arg, gm, lowq(b, gt_boxes[n], gt_valid[n], gm))):
            dst.append(v)
    return [np.stack(v) for v in out]


def dyadic_keys(rng, shape, levels=8):
    """sampling keys k / levels in [0, 1): exact in fp32, with many equal keys (resolved by index)"""
    return (rng.integers(0, levels, size=shape) / levels).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------
# sampler branch cases
RPN_SAMPLER_CONFIGS = ((4, 8), (4, 4), (16, 64))        # (npos_max, batch)


def rpn_sampler_case(with_lowq):
    """the seven images of the matcher threshold case under the three (npos_max, batch) settings, keys on four values.  Census over
    the 21 (setting, image) pairs: `over` more positives than npos_max, `room0` a negative room of exactly 0, `short` fewer candidates
    than slots, `equal_keys` sampled neighbours that share a key, `empty_images` images without gt."""
    inp, _ = matcher_threshold_case()
    mx, arg, gmax, lq = match_all(inp["boxes"], inp["gt_boxes"], inp["gt_valid"])
    if not with_lowq:
        lq = np.zeros_like(lq)
    N, P = mx.shape
    keys = dyadic_keys(np.random.default_rng(5), (N, P), levels=4)
    census = dict(over=0, room0=0, short=0, equal_keys=0, empty_images=0, lowq_over_ignored=0, lowq_over_negative=0)
    want = {}
    for npos_max, batch in RPN_SAMPLER_CONFIGS:
        for n in range(N):
            has = bool(inp["gt_valid"][n].any())
            r = rpn_labels_and_sample(mx[n], lq[n], has, keys[n], 0.3, 0.7, npos_max, batch)
            want[(npos_max, batch, n)] = r
            lab, pi, pv, ni, nv = r
            census["over"] += int((lab == 1).sum()) > npos_max
            census["room0"] += int(pv.sum()) == batch
            census["short"] += int(pv.sum() + nv.sum()) < batch
            census["empty_images"] += not has
            for idx, val in ((pi, pv), (ni, nv)):
                sel = idx[val == 1]
                census["equal_keys"] += int((keys[n][sel][1:] == keys[n][sel][:-1]).sum())
    for n in range(N):
        if inp["gt_valid"][n].any():
            v = mx[n]
            census["lowq_over_ignored"] += int(((lq[n] == 1) & (v >= F32(0.3)) & (v < F32(0.7))).sum())
            census["lowq_over_negative"] += int(((lq[n] == 1) & (v < F32(0.3))).sum())
    return dict(mx=mx, lowq=lq, gt_valid=inp["gt_valid"], keys=keys), want, census


ROI_CLASSES = 5


def roi_case(P, seed=None):
    """three images of P proposals, G = 4: image 0 ordinary, its proposal 0 the upper half of gt 0 (IoU exactly 1/2 = thr: foreground);
    image 1 without gt; image 2 with every third proposal slot invalid and a gt hole.  Census: `mx_eq_thr` valid proposals whose
    matched IoU is exactly 1/2, `nfg` foreground candidates per image, `equal_keys` valid proposals that share their key with
    another, `invalid_between` invalid slots that have a valid one on either side."""
    rng = np.random.default_rng(P if seed is None else seed)
    G, N = 4, 3
    gb = np.stack([random_int_boxes(rng, G) for _ in range(N)])
    gv = np.ones((N, G), np.uint8)
    gv[1] = 0
    gv[2, 1] = 0
    boxes = np.stack([random_int_boxes(rng, P) for _ in range(N)])
    g0 = gb[0, 0]
    boxes[0, 0] = [g0[0], g0[1], g0[2], g0[1] + (g0[3] - g0[1]) / 2]
    valid = np.ones((N, P), np.uint8)
    valid[2, 1::3] = 0
    gc = rng.integers(0, ROI_CLASSES, size=(N, G)).astype(np.int32)
    gs = (rng.integers(1, 9, size=(N, G)) / 8).astype(F32)
    gstd = (rng.integers(1, 9, size=(N, G, 4)) / 8).astype(F32)
    keys = dyadic_keys(rng, (N, P), levels=8)
    mx, arg, _, _ = match_all(boxes, gb, gv)
    census = dict(mx_eq_thr=0, nfg=[], equal_keys=0, invalid_between=0, has_gt=[int(gv[n].any()) for n in range(N)])
    for n in range(N):
        B, Gs = int_boxes(boxes[n]), int_boxes(gb[n])
        slots = [g for g in range(G) if gv[n, g]]
        for i in range(P):
            if valid[n, i] and slots:
                census["mx_eq_thr"] += max(iou_exact(Gs[g], B[i]) for g in slots) == Fraction(1, 2)
        census["nfg"].append(int(sum(1 for i in range(P) if valid[n, i] and slots and mx[n, i] >= F32(0.5))))
        kv = keys[n][valid[n] == 1]
        census["equal_keys"] += int(len(kv) - len(np.unique(kv)))
        census["invalid_between"] += sum(1 for i in range(1, P - 1) if not valid[n, i] and valid[n, i - 1] and valid[n, i + 1])
    return dict(boxes=boxes, valid=valid, mx=mx, arg=arg, keys=keys, gb=gb, gc=gc, gv=gv, gs=gs, gstd=gstd), census


def roi_sample_image(c, n, B, nfg_max):
    return roi_sample(c["boxes"][n], c["valid"][n], c["mx"][n], c["arg"][n], c["keys"][n], c["gb"][n], c["gc"][n], c["gv"][n], c["gs"][n],
                      c["gstd"][n], 0.5, ROI_CLASSES, B, nfg_max)


# ---------------------------------------------------------------------------------------------------------------------------------
# FCOS: three levels (20 x 13 stride 8, 10 x 7 stride 16, 5 x 4 stride 32) = 260 + 70 + 20 = 350 locations: not a multiple of 256, and
# the level boundary 260 falls inside the second block.  Sizes of interest [-1, 32], [32, 64], [64, INF].
FCOS_HW = [(13, 20), (7, 10), (4, 5)]
FCOS_STRIDES = [8, 16, 32]
FCOS_SOI = [[-1, 32], [32, 64], [64, INF]]
FCOS_SOI_EDGES = [32, 64]

# name -> list of (slot, box, class); MAXG = 4.  Level-0 locations sit at 8 i + 4, level-1 at 16 i + 8, level-2 at 32 i + 16.
FCOS_IMAGES = {
    # x = 12 / 36 and y = 12 / 28 are location coordinates: the locations on the four edges are background
    "edges": [(0, [12, 12, 36, 28], 3)],
    # (52, 52) is one unit inside the top-left corner, (76, 68) one unit inside the bottom-right one
    "one_inside": [(0, [51, 51, 77, 69], 4)],
    # level 0, location (20, 20): r = 32 = soi_hi -> positive; location (68, 68) of the second box: r = 33 -> background
    "soi_hi_l0": [(0, [12, 12, 52, 28], 5), (1, [60, 60, 101, 76], 6)],
    # level 1, location (40, 40): l = 32 = soi_lo -> positive (box 0); second image half: l = 31 -> background at level 1
    "soi_lo_l1": [(0, [8, 32, 48, 48], 7)],
    "soi_lo_l1_minus": [(0, [9, 32, 48, 48], 8)],
    # level 1, location (40, 40): r = 64 = soi_hi -> positive; r = 65 -> background at level 1
    "soi_hi_l1": [(0, [32, 32, 104, 48], 9)],
    "soi_hi_l1_plus": [(0, [32, 32, 105, 48], 10)],
    # two gts of area 384 over (20, 20): slot 0 wins; behind a hole (slot 0 invalid): slot 1 wins
    "area_tie": [(0, [12, 12, 36, 28], 11), (1, [12, 12, 28, 36], 12)],
    "area_tie_hole": [(1, [12, 12, 36, 28], 13), (2, [12, 12, 28, 36], 14)],
    # the thin box (area 320 < 384) covers (20, 20) with t = 40 > soi_hi of level 0: it must not win there
    "smaller_uncared": [(0, [12, 12, 36, 28], 15), (1, [18, -20, 22, 60], 16)],
    "empty": [],
    # centre sampling (radius 1.5: half-width 12 at level 0): centre (40, 32), x = 28 / 52 and y = 20 / 44 lie ON the square
    "cs_radius": [(0, [8, 8, 72, 56], 17)],
    # the box (37 .. 43) is narrower than the square (28 .. 52): x = 36 and 44 are inside the square and outside the clipped region
    "cs_clip": [(0, [37, 8, 43, 56], 18)],
    # first valid box with centre x 0: nothing is sampled, also not for the second box
    "cs_quirk": [(1, [-20, 8, 20, 56], 19), (2, [8, 8, 72, 56], 20)],
}


def fcos_pack(names, MAXG=4, slot0=0):
    """gt arrays [n, MAXG, ...] of the named images; slots shifted by slot0 (valid slots only at the END of a wide table); every
    unused slot holds a poison box covering the whole image: a positive of class 79 at every level-2 location if its valid byte were
    ignored"""
    n = len(names)
    gb = np.tile(np.array([-8, -8, 200, 200], dtype=F32), (n, MAXG, 1))
    gc = np.full((n, MAXG), 79, dtype=np.int32)
    gv = np.zeros((n, MAXG), dtype=np.uint8)
    gs = np.zeros((n, MAXG, 4), dtype=F32)
    for i, name in enumerate(names):
        for slot, box, cls in FCOS_IMAGES[name]:
            s = slot0 + slot
            gb[i, s], gc[i, s], gv[i, s] = box, cls, 1
            gs[i, s] = [cls + 0.25, cls + 0.5, cls + 0.75, cls + 1.0]
    return gb, gc, gv, gs


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS: candidates are 10 x 10 squares on a 20-pitch grid of non-negative coordinates (the class trick needs them non-negative to
# keep classes apart), 50 to a row; scores (1000 - position) / 1024 fall with the SORTED position, and `perm` scatters positions
# over slots so that slot order and score order differ.
def _nms_grid(i):
    x, y = 20 * (i % 50), 20 * (i // 50)
    return [x, y, x + 10, y + 10]


def nms_structured_case(M, nvalid, seed, ncls=1):
    """M slots, nvalid of them valid.  Sorted positions (chunks of 64): 0 suppresses 1 (IoU 7/10 > 6/10), 2 keeps 3 (IoU exactly 6/10),
    4 suppresses 6 which alone would have suppressed 8 (8 is kept), 5 / 7 are identical boxes of different classes (class-aware: both
    kept), 9 / 10 / 11 share one score (slot order).  With three chunks: 12 suppresses 130 and nothing in chunk 1; 63 / 64 share a
    score across the chunk boundary."""
    rng = np.random.default_rng(seed)
    pos_box = {p: _nms_grid(p) for p in range(nvalid)}
    cls_of = {p: int(rng.integers(0, ncls)) for p in range(nvalid)}

    def put(p, q, dy0, dy1, same_class=True):
        if q < nvalid and p < nvalid:
            b = pos_box[p]
            pos_box[q] = [b[0], b[1] + dy0, b[2], b[3] + dy1]
            cls_of[q] = cls_of[p] if same_class else (cls_of[p] + 1) % max(ncls, 2)

    put(0, 1, 0, -3)          # 70 / 100
    put(2, 3, 0, -4)          # 60 / 100: exactly the threshold, kept
    put(4, 6, 2, 2)           # 80 / 120: suppressed
    put(6, 8, 2, 2)           # vs 6: 80 / 120, vs 4: 60 / 140: kept because 6 is gone
    put(5, 7, 0, 0, same_class=False)
    put(12, 130, 0, 0)
    score = {p: F32((1000 - p) / 1024.0) for p in range(nvalid)}
    for grp in ((9, 10, 11), (63, 64)):
        for p in grp:
            if p < nvalid and grp[0] < nvalid:
                score[p] = score[grp[0]]
    slots = rng.permutation(M)[:nvalid]
    boxes = np.tile(np.array([0, 0, 10, 10], dtype=F32), (M, 1))       # invalid slots: a box that would suppress position 0
    scores = np.full(M, 2.0, dtype=F32)                                 # ... and outrank everything
    classes = np.zeros(M, dtype=np.int32)
    valid = np.zeros(M, dtype=np.uint8)
    for p in range(nvalid):
        s = slots[p]
        boxes[s], scores[s], classes[s], valid[s] = pos_box[p], score[p], cls_of[p], 1
    return dict(boxes=boxes, scores=scores, classes=classes, valid=valid)


def kth_tie_index(kept, scores):
    """t of the LAST pair kept[t - 1], kept[t] with equal scores (positions 63 / 64 of the structured case): post_topk = t puts the
    kthvalue threshold on a tie that spans the chunk boundary"""
    return max(t for t in range(1, len(kept)) if scores[kept[t - 1]] == scores[kept[t]])


def nms_random_case(M, seed, ncls, nvalid=None):
    """dense integer boxes with many overlaps, scores in sixteenths (ties), +0.0 / -0.0 among them"""
    rng = np.random.default_rng(seed)
    boxes = random_int_boxes(rng, M, span=40, sizes=(10, 20))
    scores = (rng.integers(0, 16, size=M) / 16).astype(F32)
    scores[rng.random(M) < 0.1] = F32(-0.0)
    classes = rng.integers(0, ncls, size=M).astype(np.int32)
    valid = np.ones(M, dtype=np.uint8)
    if nvalid is not None:
        valid[rng.permutation(M)[nvalid:]] = 0
    return dict(boxes=boxes, scores=scores, classes=classes, valid=valid)


def nms_bucket_case():
    """class-aware: class 3 alone in bucket 3 with exactly 64 candidates; classes 5 and 37 share bucket 5 with 40 + 25 = 65"""
    rng = np.random.default_rng(77)
    classes = np.array([3] * 64 + [5] * 40 + [37] * 25 + [1] * 7, dtype=np.int32)
    M = len(classes)
    classes = classes[rng.permutation(M)]
    boxes = random_int_boxes(rng, M, span=40, sizes=(10, 20))
    scores = (rng.integers(0, 64, size=M) / 64).astype(F32)
    return dict(boxes=boxes, scores=scores, classes=classes, valid=np.ones(M, dtype=np.uint8))


def nms_zero_sign_case():
    """slot 0 scores -0.0, slot 1 +0.0, identical boxes: equal scores, so slot 0 is kept and suppresses slot 1; slots 2 / 3 the same
    pair apart from each other: kept in slot order"""
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [40, 0, 50, 10], [80, 0, 90, 10]], dtype=F32)
    scores = np.array([-0.0, 0.0, -0.0, 0.0], dtype=F32)
    return dict(boxes=boxes, scores=scores, classes=np.zeros(4, dtype=np.int32), valid=np.ones(4, dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------
# top-k rows
TOPK_LISTS = 16      # TK_SPREAD of csrc/topk.hip


def topk_case(k, seed=3):
    """ragged rows of distinct keys (-1 = hole): k - 1, k and k + 1 candidates, a zero-width row in between, keys that differ only in
    the lowest 10-bit digit, only in the top digit (bit 62 set), a row just over 4096 wide (two blocks), and a row whose k + 1
    candidates all sit in columns that one staging list serves"""
    rng = np.random.default_rng(seed)

    def holes(keys, n_cand):
        row = np.full(len(keys), -1, dtype=np.int64)
        sel = rng.permutation(len(keys))[:n_cand]
        row[sel] = keys[sel]
        return row

    def rand_keys(n):
        hi = rng.integers(0x3C000000, 0x3F800000, size=n).astype(np.int64)
        return (hi << 32) | (0xFFFFFFFF - np.arange(n, dtype=np.int64))

    w = max(2 * k, 64)
    rows = [holes(rand_keys(w), max(k - 1, 0)), holes(rand_keys(w), k), np.zeros(0, dtype=np.int64), holes(rand_keys(w), k + 1)]
    base = np.int64(0x3F000000) << 32
    rows.append(base + rng.permutation(1024)[:min(1024, k + 5)].astype(np.int64))                      # lowest digit only
    rows.append((rng.permutation(2048)[:min(2048, k + 5)].astype(np.int64) << 52) | 12345)             # top digit only (bit 62)
    rows.append(holes(rand_keys(4100), min(4100, k + 1)))                                              # two blocks per row
    # one staging list filled to its capacity: the collect kernel sends column i of a row to list (block + wave) % 16 with block =
    # (i // 256) % grid, wave = (i % 256) // 64 and grid = min(256, ceil(widest row / 4096)) blocks per row; k + 1 candidates, all in
    # columns of list 0, in the narrowest row (a multiple of 4096, + 4) that has that many such columns
    W = 4100
    while True:
        grid = min(256, -(-max(W, w) // 4096))
        col = np.arange(W)
        cols0 = col[((col // 256) % grid + (col % 256) // 64) % TOPK_LISTS == 0]
        if len(cols0) >= k + 1:
            break
        W += 4096
    one = np.full(W, -1, dtype=np.int64)
    one[cols0[:k + 1]] = rand_keys(W)[cols0[:k + 1]]
    rows.append(one)
    flat = np.concatenate(rows)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    census = dict(rows=len(rows), zero_width=sum(len(r) == 0 for r in rows), k_minus_1=int((rows[0] >= 0).sum() == k - 1),
                  k_exact=int((rows[1] >= 0).sum() == k), k_plus_1=int((rows[3] >= 0).sum() == k + 1),
                  just_over_4096=sum(len(r) == 4100 for r in rows), one_list=int((one >= 0).sum()), bit62=int(np.any(rows[5] >> 62 == 1)))
    return flat, off, max(len(r) for r in rows), census


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN decode: two levels (3 x 2 and 2 x 1 pixels), A = 2 anchors per pixel, two images of ragged size, weights 1, min_size 4
DEC_HW = [6, 2]
DEC_A = 2
DEC_CH = DEC_A * 5
DEC_SIZES = [(64.0, 96.0), (40.0, 50.0)]      # (H, W)
DEC_MIN = 4.0


def decode_case():
    """anchors: level 0 8 x 8 squares at x = 16 p, two per pixel (the second 4 wide: w == min_size -> dropped; pixel 2's second one
    5 wide -> kept); level 1 32 x 32.  Deltas move boxes past W / H and below 0; one logit is +inf, one delta NaN."""
    N = 2
    anchors = []
    for p in range(DEC_HW[0]):
        anchors.append([16 * p, 8, 16 * p + 8, 16])
        anchors.append([16 * p, 24, 16 * p + (5 if p == 2 else 4), 32])
    for p in range(DEC_HW[1]):
        anchors.append([32 * p, 0, 32 * p + 32, 32])
        anchors.append([32 * p + 8, 8, 32 * p + 40, 40])
    anchors = np.array(anchors, dtype=F32)
    rows = N * sum(DEC_HW)
    head = np.zeros((rows, DEC_CH), dtype=F32)
    rng = np.random.default_rng(5)
    head[:, :DEC_A] = (rng.permutation(rows * DEC_A).reshape(rows, DEC_A) - 10) / 8.0      # distinct logits, some negative
    A = DEC_A

    def delta(l, n, p, a, dx, dy):
        r = sum(N * h for h in DEC_HW[:l]) + n * DEC_HW[l] + p
        head[r, A + 4 * a], head[r, A + 4 * a + 1] = dx, dy
        return r

    delta(0, 0, 5, 0, 1.5, 0.0)        # x: 80 .. 88 -> 92 .. 100: clipped exactly to W = 96 (4 wide = min_size: dropped)
    delta(0, 0, 4, 0, 3.0, 0.0)        # 64 .. 72 -> 88 .. 96: x2 == W without clipping
    delta(0, 0, 0, 0, -0.5, -2.0)      # x: 0 .. 8 -> -4 .. 4, y: 8 .. 16 -> -8 .. 0: clipped to 0, zero height
    delta(0, 1, 3, 0, 0.5, 4.0)        # image 1 (H 40, W 50): x 48 .. 56 -> 52 .. 60 beyond W: both clipped to 50
    delta(1, 1, 1, 1, 0.25, 0.25)      # 40 .. 72 -> 48 .. 80: clipped to W = 50 / H = 40
    r = delta(0, 0, 1, 0, 0.0, 0.0)
    head[r, 0] = np.inf                # infinite logit: not kept, score 0
    delta(0, 1, 1, 1, np.nan, 0.0)     # NaN delta: not kept
    image_hw = np.array(DEC_SIZES, dtype=F32)
    return dict(head=head, anchors=anchors, image_hw=image_hw, N=N)
