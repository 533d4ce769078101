"""Plain references of the scalar loss tails (csrc/fcos.hip fcos_loss_combine_kernel, csrc/rcnn.hip rcnn_loss_combine_kernel), of the
whole fused FCOS loss node (ops._FcosJointLossFn) and of the inference pack kernels, with the rule that holds a kernel to them.
HELPER MODULE: no tests in it (tests/test_loss_tail_ref64.py anchors it on the CPU, tests/test_loss_tails_gpu.py and
tests/test_infer_pack_gpu.py run the kernels against it).

The tails are written from the definitions - FCOSOutputs.losses / pseudo_losses / _kl_mean / _normalisers, the comment blocks above the two
kernels and the trainer's `value * mul / div` weighting - as functions of the raw kernel sums.  They work in the dtype of their inputs
(float64 = r64, float32 on the CPU = r32); `coef` is torch.autograd.grad of the total with respect to the sum leaves, nothing is derived by
hand; normalisers are detached, as in the product.  Scalars (world, weights, the 1e-6 clamp) are taken at their fp32 value in every
precision: they are fp32 numbers in the product (an ATen clamp of an fp32 tensor, a float kernel argument).

Rule per entry (`tail_ok`): |k - r64| <= n 2^-24 sum |addends|, n = the fp32 roundings on the entry's path (`fcos_counts`, `rcnn_counts`:
counted from the formulas, fp32 division correctly rounded), sum |addends| = the same function evaluated at the absolute values of its
inputs (`*_mag`: every tail is a positive combination of its sums once the normalisers are fixed).

`mut` selects a deliberately WRONG variant; test_loss_tail_ref64.py shows that the rules reject each:
  kl4drop    the factor 4 of the "klloss" mean dropped          unifycoef  the unified centerness term keeps its gradient (coef[12])
  nonorm     `norm` ignored when given (local sums)             clamp1     the 1e-6 clamp of the loss normaliser written as 1
  klw1       the KL weight applied once on the supervised branch
  rnclamp    (rcnn) the ROI count not clamped to 1              swap14     (rcnn node) the slices of c[1] and c[4] swapped
  noacc3     (joint) the third location backward overwrites instead of adding
  box0       (gather) box 0 taken when nbox == K                cntle      (pack) d <= cnt[n]
"""
import numpy as np
import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_cont as L64C

U = L64.U
EPS_DEN = float(np.float32(1e-6))     # the clamp of the loss normaliser as the product holds it: an fp32 number


def f32(v):
    """a Python float at its fp32 value"""
    return float(np.float32(v))


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_(True)


def _clamp_min(x, lo):
    return torch.clamp(x.detach(), min=lo)


# =================================================================================================
# FCOS: flags 1 = KL_LOSS on the supervised branch, 2 = KL type "klloss", 4 = UNIFY_CTRCLS, 8 = TS-better pseudo location term.
# sums layout (LT_NSUM): [n_pos, sum ctr target, sum BCE, sum IoU loss x ctr target, sum NLL / KL, n selected, sum selected L1, 0]
# =================================================================================================
def _kl_mean(sums, klloss, mut):
    n = _clamp_min(sums[0], 1.0)
    if klloss and mut != "kl4drop":
        return sums[4] / (4.0 * n)
    return sums[4] / n


def fcos_tail(focal_sup, sums_sup, focal_cls, sums_cls, sums_reg, norm, world, flags, kl_weight, wmul, wdiv, mut=None, dtype=None):
    """-> (rec [8] = cls, loc, ctr, cls_pseudo, ctr_pseudo, loc_pseudo, teacher_better_student, total; coef [26] = d total / d
    (focal_sup[1], sums_sup[8], focal_cls[1], sums_cls[8], sums_reg[8]))"""
    dt = dtype or sums_sup.dtype
    leaves = [_leaf(t, dt) for t in (focal_sup, sums_sup, focal_cls, sums_cls, sums_reg)]
    fs, S, fc, C, R = leaves
    kl, klloss, unify, tsb = bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8)
    world, w = f32(world), f32(kl_weight)
    nrm = None if (norm is None or mut == "nonorm") else norm.detach().to(dt)

    def normalisers(sums, j):
        pair = sums[0:2].detach() if nrm is None else nrm[2 * j:2 * j + 2]     # the all-reduced (n_pos, sum ctr) of the target set
        return torch.clamp(pair[0] / world, min=1.0), torch.clamp(pair[1] / world, min=1.0 if mut == "clamp1" else EPS_DEN)

    # supervised branch (losses())
    npa, den = normalisers(S, 0)
    cls, ctr, loc = fs[0] / npa, S[2] / npa, S[3] / den
    if kl:
        loc = (w * _kl_mean(S, klloss, mut) if mut == "klw1" else w * (w * _kl_mean(S, klloss, mut))) + loc
    # pseudo classification set
    npa_c, _ = normalisers(C, 1)
    cls_p, ctr_p = fc[0] / npa_c, C[2] / npa_c
    if unify:
        ctr_p = (ctr_p - ctr_p.detach()) if mut == "unifycoef" else ctr_p * 0
    # pseudo regression set
    tbs = torch.zeros((), dtype=dt)
    if tsb:
        loc_p = R[6] / _clamp_min(R[5], 1.0)
        tbs = R[5].detach()
    else:
        loc_p = w * _kl_mean(R, klloss, mut)
    vals = [cls, loc, ctr, cls_p, ctr_p, loc_p]
    total = torch.zeros((), dtype=dt)
    for k in range(6):
        total = total + vals[k] * f32(wmul[k]) / f32(wdiv[k])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    coef = torch.cat([torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)])
    rec = torch.stack([v.detach() for v in vals] + [tbs, total.detach()])
    return rec, coef


def fcos_mag(focal_sup, sums_sup, focal_cls, sums_cls, sums_reg, norm, world, flags, kl_weight, wmul, wdiv):
    """sum |addends| of every rec / coef entry in fp64: the tail at the absolute values (normaliser inputs are counts / target sums >= 0)"""
    a = [t.double().abs() for t in (focal_sup, sums_sup, focal_cls, sums_cls, sums_reg)]
    return fcos_tail(*a, None if norm is None else norm.double(), world, flags, abs(kl_weight), [abs(v) for v in wmul], [abs(v) for v in wdiv])


def fcos_counts(flags):
    """fp32 roundings per entry.  g_k = wmul_k / wdiv_k: 1.  A normaliser max(x / world, lo): 1 (the clamp constants are exact).
      cls, ctr, cls_p, ctr_p = sum / npa: 1 + 1 = 2;  their coef g / npa: 1 + 1 + 1 = 3
      loc = S3 / den: 2; with KL: the term w (w (S4 / dn)) has 3 (dn = (4) max(S0, 1) is exact) and one add joins the two: 4
      coef[4] = g / den: 3;  coef[5] = g (w w) / dn: g 1, w w 1, product 1, quotient 1 = 4
      TS-better: loc_p = R6 / max(R5, 1): 1, coef[24] = g / d: 2, rec[6] = R5: 0;  else loc_p = w (R4 / dn): 2, coef[22] = g w / dn: 3
      total = sum of six v_k wmul_k / wdiv_k: the deepest value (loc, 4) + product 1 + quotient 1 + five adds = 11
    -> (n_rec [8], n_coef [26])"""
    kl, tsb = bool(flags & 1), bool(flags & 8)
    nrec = [2, 4 if kl else 2, 2, 2, 2, 1 if tsb else 2, 0, 11]
    ncoef = [0] * 26
    ncoef[0], ncoef[3], ncoef[4], ncoef[5], ncoef[9], ncoef[12] = 3, 3, 3, 4, 3, 3
    ncoef[22], ncoef[24] = 3, 2
    return nrec, ncoef


def fcos_structural_zero(flags):
    """coef entries that must be +0 as bits"""
    kl, unify, tsb = bool(flags & 1), bool(flags & 4), bool(flags & 8)
    used = {0, 3, 4, 9}
    if kl:
        used.add(5)
    if not unify:
        used.add(12)
    used.add(24 if tsb else 22)
    return [i for i in range(26) if i not in used]


# =================================================================================================
# Faster-RCNN: loss_cls = focal / Rn, loss_box_reg = w_box box / Rn (Rn = targets >= 0, at least 1), loss_rpn_cls = w_rpn_cls rpn[0] / norm,
# loss_rpn_loc = w_rpn_loc rpn[1] / norm; total = sum_k wt[k] loss_k, k = {cls, box, rpn_cls, rpn_loc} x {supervised, pseudo}
# =================================================================================================
def rcnn_tail(rpn_sup, rpn_uns, focal_sup, focal_uns, box_sup, box_uns, tgt_sup, tgt_uns, norm_sup, norm_uns, w_rpn_cls, w_rpn_loc, w_box, wt,
              mut=None, dtype=None):
    """-> (rec [9], coef [8] in rec order, grads: d total / d (rpn_sup[2], rpn_uns[2], focal_sup, focal_uns, box_sup, box_uns) leaf by leaf)"""
    dt = dtype or rpn_sup.dtype
    leaves = [_leaf(t, dt) for t in (rpn_sup, rpn_uns, focal_sup, focal_uns, box_sup, box_uns)]
    vals = []
    for b, (rpn, foc, box, tgt, nrm) in enumerate(((leaves[0], leaves[2], leaves[4], tgt_sup, norm_sup),
                                                    (leaves[1], leaves[3], leaves[5], tgt_uns, norm_uns))):
        rn = torch.tensor(float(int((tgt >= 0).sum())), dtype=dt)
        if mut != "rnclamp":
            rn = torch.clamp(rn, min=1.0)
        vals += [foc[0] / rn, f32(w_box) * (box[0] / rn), f32(w_rpn_cls) * (rpn[0] / f32(nrm)), f32(w_rpn_loc) * (rpn[1] / f32(nrm))]
    total = torch.zeros((), dtype=dt)
    for k in range(8):
        total = total + vals[k] * f32(wt[k])
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    # rec order: the gradient of the sum each loss is made of
    coef = torch.stack([grads[2][0], grads[4][0], grads[0][0], grads[0][1], grads[3][0], grads[5][0], grads[1][0], grads[1][1]])
    return torch.stack([v.detach() for v in vals] + [total.detach()]), coef, grads


def rcnn_mag(rpn_sup, rpn_uns, focal_sup, focal_uns, box_sup, box_uns, tgt_sup, tgt_uns, norm_sup, norm_uns, w_rpn_cls, w_rpn_loc, w_box, wt):
    a = [t.double().abs() for t in (rpn_sup, rpn_uns, focal_sup, focal_uns, box_sup, box_uns)]
    return rcnn_tail(*a, tgt_sup, tgt_uns, norm_sup, norm_uns, abs(w_rpn_cls), abs(w_rpn_loc), abs(w_box), [abs(v) for v in wt])[:2]


# fp32 roundings (Rn is an exact count): loss_cls = focal / Rn: 1; the three weighted losses w (sum / n): 2; every coef wt (w / n): 2 (1 / Rn
# and wt x: 2 as well); total = eight v_k wt_k: 2 + 1 + seven adds = 10
RCNN_NREC = [1, 2, 2, 2, 1, 2, 2, 2, 10]
RCNN_NCOEF = [2] * 8


def rcnn_node_slices(c, mut=None):
    """the node's backward in words: the gradient of every input of ops.rcnn_loss_combine, from coef in rec order"""
    i1, i4 = (4, 1) if mut == "swap14" else (1, 4)
    return (torch.stack((c[2], c[3])), torch.stack((c[6], c[7])), c[0:1], c[i4:i4 + 1], c[i1:i1 + 1], c[5:6])


# =================================================================================================
# the rule
# =================================================================================================
def tail_ratio(k, r64, mag, n):
    """worst |k - r64| / (n u mag) over the entries with n > 0; entries with n == 0 (or mag == 0) must equal r64 exactly -> (ratio, exact_ok)"""
    k, r64, mag = L64._np(k), L64._np(r64), L64._np(mag)
    n = np.asarray(n, dtype=np.float64).reshape(-1)
    assert k.shape == r64.shape == mag.shape == n.shape, (k.shape, r64.shape, mag.shape, n.shape)
    if not np.all(np.isfinite(k)):
        return float("inf"), False
    err = np.abs(k - r64)
    den = n * U * mag
    exact = den == 0
    ratio = np.where(exact, 0.0, err / np.where(exact, 1.0, den))
    return float(ratio.max()) if ratio.size else 0.0, bool(np.all(err[exact] == 0))


def tail_ok(k, r64, mag, n):
    ratio, exact_ok = tail_ratio(k, r64, mag, n)
    return ratio <= 1.0 and exact_ok, ratio


def is_pos_zero(t):
    """every element is +0 as bits"""
    return bool(torch.all(t.detach().cpu().contiguous().view(torch.int32) == 0))


# =================================================================================================
# the fused FCOS loss node: focal + location sums of the three target sets -> tail -> gradients of the head outputs
# =================================================================================================
def fcos_joint(logits, box, sets, consts, cont=False, mut=None):
    """sets = ((lab_s, reg_s), (lab_c, reg_c), (lab_r, reg_r, bv_r | None)); consts as ops.fcos_joint_loss takes them.
    -> dict(rec [8], total, sums = (focal_s, sums_s, focal_c, sums_c, sums_r), terms (the per-row addends of those sums), coef [26],
    dlogits / dbox: the lists of addends (one per branch and per addend of that branch, times its tail coefficient))"""
    (lab_s, reg_s), (lab_c, reg_c), (lab_r, reg_r, bv_r) = sets
    alpha, gamma, nc, rm, flags_s, flags_p, tsb, tsc, world, cflags, klw, wmul, wdiv = consts
    C = logits.shape[1]
    loc = L64C.loc_terms_cont if cont else L64.loc_terms
    fl_s, fp_s = L64.focal(logits, lab_s, C, alpha, gamma)
    fl_c, fp_c = L64.focal(logits, lab_c, C, alpha, gamma)
    t_s, g_s, _ = loc(box, reg_s, None, lab_s, flags_s, 0.0, 0.0, num_classes=nc)
    t_c, g_c, _ = loc(box, reg_c, None, lab_c, flags_p, 0.0, 0.0, num_classes=nc)
    t_r, g_r, _ = loc(box, reg_r, bv_r, lab_r, flags_p, tsb, tsc, num_classes=nc)
    sums = (fl_s.sum().reshape(1), t_s.sum(dim=0), fl_c.sum().reshape(1), t_c.sum(dim=0), t_r.sum(dim=0))
    rec, coef = fcos_tail(*sums, None, world, cflags, klw, wmul, wdiv)
    dlogits = [coef[0] * p for p in fp_s] + [coef[9] * p for p in fp_c]
    dbox = []
    for base, gs in ((1, g_s), (10, g_c), (18, g_r)):
        if mut == "noacc3" and base != 18:
            continue
        if len(gs) == 4:      # the addends of sums [2], [3], [4], [6]
            dbox += [coef[base + j] * g for j, g in zip((2, 3, 4, 6), gs)]
        else:                 # no positive row in this set
            dbox += [torch.zeros_like(box)]
    return {"rec": rec, "total": rec[7], "sums": sums, "terms": (fl_s, t_s, fl_c, t_c, t_r), "coef": coef, "dlogits": dlogits, "dbox": dbox}


# =================================================================================================
# the inference pack kernels as plain indexing
# =================================================================================================
def nms_pack(kidx, cnt, boxes, scores, mut=None):
    """kidx [N, D] (-1 = padded slot: row 0 is read), cnt [N], boxes [N, M, 4], scores [N, M] -> (boxes [N, D, 4], scores [N, D], valid [N, D])"""
    N, D = kidx.shape
    ix = kidx.clamp(min=0).long()
    n = torch.arange(N)[:, None].expand(N, D)
    d = torch.arange(D)[None, :].expand(N, D)
    valid = (d <= cnt[:, None]) if mut == "cntle" else (d < cnt[:, None])
    return boxes[n, ix], scores[n, ix], valid.to(torch.uint8)


def roi_infer_gather(flat, score, boxes, K, thr, mut=None):
    """flat [N, k]: the flat (proposal, class) index of every selected key, score [N, k]: its probability; boxes [N, P, 4] | [N, P, K, 4]
    -> (sc, rows, cls, cb, valid)"""
    N, k = flat.shape
    rows, cls = flat // K, flat % K
    n = torch.arange(N)[:, None].expand(N, k)
    if boxes.dim() == 3:
        cb = boxes[n, rows]
    else:
        cb = boxes[n, rows, torch.zeros_like(cls) if mut == "box0" else cls]
    return score, rows, cls.to(torch.int32), cb, (score > thr).to(torch.uint8)


def roi_infer_pack(kidx, cnt, cb, sc, cls, rows, std, P, D, nbox, mut=None):
    """std [N, P, 4 nbox] -> (boxes [N, D, 4], scores, classes, std [N, D, 4 nbox], rows, valid)"""
    N = kidx.shape[0]
    ix = kidx.clamp(min=0).long()
    n = torch.arange(N)[:, None].expand(N, D)
    d = torch.arange(D)[None, :].expand(N, D)
    r = rows[n, ix]
    valid = (d <= cnt[:, None]) if mut == "cntle" else (d < cnt[:, None])
    return cb[n, ix], sc[n, ix], cls[n, ix], std.reshape(N, P, 4 * nbox)[n, r], r, valid.to(torch.uint8)


# =================================================================================================
# inputs of the fused node: one head output, three synthetic target sets (no target kernel involved)
# =================================================================================================
JOINT_P, JOINT_C = 129, 80
TSB, TSC = 0.1, 0.5


def joint_case(layout, seed, BS=80, cont=False):
    """logits [P, 80], box [P, BS], ((lab_s, reg_s), (lab_c, reg_c), (lab_r, reg_r, bv_r)); the label / target sets come from
    loss_ref64.loc_case (loss_ref64_cont.cont_case for the continuous head) with different seeds, the logits from loss_ref64.focal_case.
      fused   the first 64 rows are the supervised images (skipped, < 0, in the pseudo sets), the others the pseudo images (skipped in the
              supervised set): the row layout of a fused batch
      shared  every set covers all rows and the two pseudo sets have the SAME labels: all three location backwards add into the same rows
      empty   an all-background supervised set and pseudo sets without a positive (background on their own rows)"""
    P, C = JOINT_P, JOINT_C
    logits, _ = L64.focal_case(P, C, seed)
    draw = (lambda s: L64C.cont_case(P, BS, s)) if cont else (lambda s: L64.loc_case(P, BS, s))
    box, reg_s, _, lab_s = draw(seed + 1)
    _, reg_c, _, lab_c = draw(seed + 2)
    _, reg_r, bv_r, lab_r = draw(seed + 3)
    lab_s, lab_c, lab_r = lab_s.clone(), lab_c.clone(), lab_r.clone()
    if layout == "fused":
        lab_s[64:] = -1
        lab_c[:64] = -1
        lab_r[:64] = -1
    elif layout == "shared":
        lab_r = lab_c.clone()
    elif layout == "empty":
        lab_s = torch.where(lab_s < 0, lab_s, torch.full_like(lab_s, 80))
        lab_s[64:] = -1
        lab_c[:], lab_r[:] = 80, 80
        lab_c[:64], lab_r[:64] = -1, -1
    else:
        raise ValueError(layout)
    return logits, box, ((lab_s, reg_s), (lab_c, reg_c), (lab_r, reg_r, bv_r))


def joint_consts(cflags, flags_s, flags_p, reg_max, klw=0.05, world=1.0):
    """the `consts` of ops.fcos_joint_loss: six pairwise distinct weights (value * mul / div), all fp32 numbers"""
    wmul = [1.0, 1.25, 0.75, 4.0, 3.0, 2.0]
    wdiv = [1.0, 1.0, 1.0, 5.0, 4.0, 3.0]
    return (0.25, 2.0, 80, reg_max, flags_s, flags_p, f32(TSB), f32(TSC), world, cflags, f32(klw), wmul, wdiv)


# =================================================================================================
# input grids of the two combine kernels (fp32 numbers; the same values go to the kernel and, cast, to the references)
# =================================================================================================
FCOS_SUM_SETS = ["ordinary", "npos0_sup", "npos0_cls", "npos0_reg", "npos0_all", "npa_is_1", "npa_below_1", "den_above", "den_below",
                 "r5_zero", "large"]
FCOS_WMUL, FCOS_WDIV = [1.0, 1.3, 0.7, 4.0, 3.0, 2.0], [1.0, 1.0, 1.0, 5.0, 4.0, 3.0]     # six pairwise distinct mul / div


def fcos_sums(name, world, with_norm):
    """-> (focal_sup [1], sums_sup [8], focal_cls [1], sums_cls [8], sums_reg [8], norm [6] | None), fp32.  The (n_pos, sum ctr) pair the
    normalisers must use sits in `norm` when it is given - the local pair of the sums is then another number - and in the sums otherwise."""
    F = torch.float32
    fs, fc = torch.tensor([812.2513], dtype=F), torch.tensor([433.0917], dtype=F)
    S = torch.tensor([37.0, 21.3761, 30.5217, 17.2533, 140.7519, 0.0, 0.0, 0.0], dtype=F)
    C = torch.tensor([23.0, 12.9107, 19.0311, 10.7713, 61.2209, 0.0, 0.0, 0.0], dtype=F)
    R = torch.tensor([29.0, 16.5023, 22.2519, 12.5011, 96.1277, 55.0, 41.3759, 0.0], dtype=F)
    sets = [S, C, R]
    if name.startswith("npos0"):
        for j, key in enumerate(("sup", "cls", "reg")):
            if name.endswith(key) or name.endswith("all"):
                sets[j][:] = 0.0          # no positive: every location sum is 0; the focal sum (background rows) is not
    elif name == "npa_is_1":
        S[0], C[0] = world, world
    elif name == "npa_below_1":
        S[0], C[0] = world - 1.0, world - 1.0
    elif name == "den_above":
        S[1] = world * 2e-6
    elif name == "den_below":
        S[1] = world * 5e-7
    elif name == "r5_zero":
        R[5] = 0.0
    elif name == "large":
        fs *= 1500.0
        fc *= 1500.0
        for t in sets:
            t[0] = torch.round(t[0] * 30000.0)
            t[1:7] *= 30000.0
            t[5] = torch.round(t[5])
    elif name != "ordinary":
        raise ValueError(name)
    norm = None
    if with_norm:
        norm = torch.cat([t[0:2].clone() for t in sets])
        for t in sets:                     # the local pair: not what the normalisers may use (n_pos still feeds the local KL mean)
            t[0] = torch.floor(t[0] / world) + 2.0
            t[1] = t[1] * 0.37 + 0.25
    return fs, S, fc, C, R, norm


def fcos_dyadic(world):
    """sums on a dyadic grid: counts, weights and world powers of two, sums small integers - every operation of the tail is exact"""
    F = torch.float32
    fs, fc = torch.tensor([24.0], dtype=F), torch.tensor([40.0], dtype=F)
    S = torch.tensor([8.0 * world, 4.0 * world, 12.0, 6.0, 20.0, 0.0, 0.0, 0.0], dtype=F)
    C = torch.tensor([16.0 * world, 2.0 * world, 10.0, 3.0, 9.0, 0.0, 0.0, 0.0], dtype=F)
    R = torch.tensor([4.0, 2.0, 5.0, 7.0, 14.0, 8.0, 18.0, 0.0], dtype=F)
    return fs, S, fc, C, R, [2.0, 4.0, 1.0, 8.0, 2.0, 4.0], [1.0, 2.0, 4.0, 2.0, 8.0, 1.0], 0.25


RCNN_NTGT = [0, 1, 63, 64, 65, 512, 1000]
RCNN_WT = [1.0, 1.1, 0.9, 1.2, 4.0, 3.7, 4.4, 0.0]     # pairwise distinct; loss_rpn_loc_pseudo x 0


def rcnn_sums(n_sup, n_uns, seed, all_empty=False):
    """-> (rpn_sup [2], rpn_uns [2], focal_sup, focal_uns, box_sup, box_uns, tgt_sup [n_sup] int32, tgt_uns [n_uns] int32)"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.rand(8, generator=g) * 300.0 + 1.0
    tg = []
    for n in (n_sup, n_uns):
        t = torch.randint(0, 81, (n,), generator=g, dtype=torch.int32)
        if all_empty:
            t[:] = -1
        elif n > 2:
            t[1::3] = -1        # empty slots mixed in
            t[n - 1] = -7
        tg.append(t)
    return (vals[0:2].clone(), vals[2:4].clone(), vals[4:5].clone(), vals[5:6].clone(), vals[6:7].clone(), vals[7:8].clone(), tg[0], tg[1])
