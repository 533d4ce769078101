"""CPU anchors of tests/loss_ref64.py: the fp64 references agree with the oracle on benign inputs, autograd's tie semantics are what
the kernels' comments claim, the comparator rejects every deliberately wrong variant on the edge grids (and lets two of them through
on a benign, golden-like grid - the reason the edge grids exist), and no input grid needs more than 2 % of its elements excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import utv2_oracle as O
from tests import loss_ref64 as L64
from tests import test_loss_kernels_fp64_gpu as G   # the grids and parameter lists of the GPU module: the two cannot drift

F32, F64 = torch.float32, torch.float64


def near(a64, b32, k=64):
    """agreement to fp32 rounding: k u of the largest magnitude involved"""
    a = np.asarray(a64.detach().double().numpy() if torch.is_tensor(a64) else a64, dtype=np.float64)
    b = np.asarray(b32.detach().double().numpy() if torch.is_tensor(b32) else b32, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    tol = k * L64.U * max(1e-30, float(np.abs(b).max()))
    assert float(np.abs(a - b).max()) <= tol, (float(np.abs(a - b).max()), tol)


# ---- agreement with the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.25, -1.0])
def test_focal_agrees_with_oracle(alpha):
    """alpha = -1: the oracle (fvcore's rule) and the fp64 reference both leave the class weight out"""
    x, lab = L64.focal_case(64, 80, 3, edge=False)
    lab = lab.clamp(min=0)
    loss64, _ = L64.focal(x.double(), lab, 80, alpha, 2.0)
    t = (lab[:, None] == torch.arange(80)[None, :]).float()
    near(loss64, O.sigmoid_focal_loss(x, t, alpha, 2.0))
    if alpha < 0:
        near(loss64, F.binary_cross_entropy_with_logits(x, t, reduction="none") * (1 - torch.sigmoid(x) * t - (1 - torch.sigmoid(x)) * (1 - t)) ** 2)


def test_loc_terms_agree_with_oracle():
    box, t, bv, lab = L64.benign_loc_case(96, 80, 5)
    pos = (lab >= 0) & (lab != 80)
    reg, std, tt = box[pos, :68], box[pos, 68:72], t[pos]
    d32 = O.integral(reg)
    ctr32, iou32 = O.ctrness_targets(tt), O.iou_targets(d32, tt)
    n = int(pos.sum())
    terms, _, info = L64.loc_terms(box.double(), t, bv, lab, 0, 0.1, 0.5)
    near(info["d"], d32)
    near(terms[pos, 1], ctr32)
    near(terms[:, 3].sum(), O.giou_loss_ltrb(d32, tt, ctr32))
    near(terms[:, 4].sum() / n, O.nl_loss(d32, std, tt, iou32))
    near(L64.loc_terms(box.double(), t, bv, lab, L64.LT_QUALITY_IOU, 0.1, 0.5)[0][pos, 1], iou32)
    near(L64.loc_terms(box.double(), t, bv, lab, 1 << 2, 0.1, 0.5)[0][:, 3].sum(), O.giou_loss_ltrb(d32, tt, ctr32, "iou"))
    near(L64.loc_terms(box.double(), t, bv, lab, 2 << 2, 0.1, 0.5)[0][:, 3].sum(), O.giou_loss_ltrb(d32, tt, ctr32, "linear_iou"))
    near(L64.loc_terms(box.double(), t, bv, lab, L64.LT_KLLOSS, 0.1, 0.5)[0][:, 4].sum(), O.kl_loss(d32, std, tt, method="sum"))
    near(L64.loc_terms(box.double(), t, bv, lab, L64.LT_KLLOSS | L64.LT_KL_WCTR, 0.1, 0.5)[0][:, 4].sum(),
         O.kl_loss(d32, std, tt, method="weight_ctr_sum", weight=ctr32))
    # the teacher-better selection of fcos_pseudo_losses (oracle :507-512)
    sel = ((1 - bv[pos].sigmoid()) > 0.5) * ((1 - bv[pos].sigmoid()) > (1 - std.sigmoid()) + 0.1)
    assert torch.equal(sel, info["sel"]) and int(sel.sum()) > 0
    near(terms[:, 6].sum(), (d32[sel] - tt[sel]).abs().sum())


def test_softmax_focal_agrees_with_oracle():
    x, tgt = L64.softmax_case(48, 81, 4, edge=False)
    loss64, _, _ = L64.softmax_focal(x.double(), tgt, 1.5)
    near(loss64.sum() / 48, O.softmax_focal(x, tgt.long(), 1.5))


def test_rpn_loss_agrees_with_oracle():
    g = torch.Generator().manual_seed(8)
    anchors = O.make_anchors([(8, 8)], [8], sizes=(32,))
    anchors = torch.cat(list(anchors)) if isinstance(anchors, (list, tuple)) else anchors
    R, N, batch = anchors.shape[0], 2, 32
    obj, deltas = torch.randn((N, R), generator=g), torch.randn((N, R, 4), generator=g) * 0.3
    gts = [{"boxes": torch.tensor([[4.0, 6.0, 40.0, 44.0], [20.0, 10.0, 60.0, 50.0]]), "scores": torch.tensor([0.9, 0.6])} for _ in range(N)]
    keys = torch.rand((N, R), generator=g)
    for pseudo in (False, True):
        out, samples = O.rpn_losses(anchors, obj, deltas, gts, keys, pseudo, batch=batch)
        npos, nneg = max(len(p) for p, _ in samples), max(len(q) for _, q in samples)
        assert npos > 0
        s = {"pos_idx": torch.zeros((N, npos), dtype=torch.int64), "neg_idx": torch.zeros((N, nneg), dtype=torch.int64),
             "pos_valid": torch.zeros((N, npos), dtype=torch.uint8), "neg_valid": torch.zeros((N, nneg), dtype=torch.uint8),
             "has_gt": torch.ones((N, 1), dtype=torch.uint8), "matched32": torch.zeros((N, R), dtype=torch.int32)}
        for n, (p, q) in enumerate(samples):
            s["pos_idx"][n, :len(p)], s["pos_valid"][n, :len(p)] = p, 1
            s["neg_idx"][n, :len(q)], s["neg_valid"][n, :len(q)] = q, 1
            s["matched32"][n] = O.matcher(O.pairwise_iou(gts[n]["boxes"], anchors), [0.3, 0.7], [0, -1, 1], True)[0].int()
        c = {"obj": obj, "deltas": deltas, "s": s}
        x, dl = L64.rpn_slot_inputs(c, F64)
        gtb, gsc = torch.stack([q["boxes"] for q in gts]), torch.stack([q["scores"] for q in gts])
        cls, loc, _, _ = L64.rpn_loss(x, dl, anchors, s, gtb, gsc if pseudo else None, (1.0, 1.0, 1.0, 1.0))
        near(cls.sum() / (batch * N), out["loss_rpn_cls"])
        near(loc.sum() / (batch * N), out["loss_rpn_loc"])


def test_roi_box_loss_agrees_with_oracle():
    c = L64.roi_case(96, 12, edge=False)
    de, st = c["mat"][:, :4], c["mat"][:, 4:]
    a = (c["cls"], c["prop"], c["gtb"], c["gstd"], 80)
    l0 = L64.roi_box_loss(de.double(), st.double(), *a, 0, 10.0, 10.0, 62.5, 0.1, 0.5)[0]   # the oracle's transform reads weights[0:2] = (10, 10)
    near(l0.sum() / 96, O.roi_box_reg_loss(c["prop"], c["gtb"], de, st, c["cls"]).reshape(()))
    l2 = L64.roi_box_loss(de.double(), st.double(), *a, 2, 10.0, 10.0, 62.5, 0.1, 0.5)[0]
    assert float(l2.sum()) > 0
    near(l2.sum() / 96, O.roi_box_reg_pseudo_loss(c["prop"], c["gtb"], de, st, c["gstd"], c["cls"]))


# ---- tie semantics of autograd -----------------------------------------------------------------
def test_tie_semantics_of_autograd():
    a = torch.tensor([2.0, 3.0], dtype=F64, requires_grad=True)
    b = torch.tensor([2.0, 1.0], dtype=F64, requires_grad=True)
    ga, gb = torch.autograd.grad(torch.min(a, b).sum(), (a, b))
    assert ga.tolist() == [0.5, 0.0] and gb.tolist() == [0.5, 1.0]
    ga, gb = torch.autograd.grad(torch.max(a, b).sum(), (a, b))
    assert ga.tolist() == [0.5, 1.0] and gb.tolist() == [0.5, 0.0]
    v = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0], dtype=F64, requires_grad=True)
    assert torch.autograd.grad(torch.clamp(v, min=-1.0, max=1.0).sum(), v)[0].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]
    assert torch.autograd.grad(v.clamp(min=0).sum(), v)[0].tolist() == [0.0, 0.0, 1.0, 1.0, 1.0]
    assert torch.autograd.grad(v.abs().sum(), v)[0].tolist() == [-1.0, -1.0, 0.0, 1.0, 1.0]


def test_reference_splits_the_gradient_on_a_tie():
    """one bin at +60 and an integer target: d == t on all four sides, in fp32 and in fp64; the GIoU gradient of the reference is the
    half / half split: exactly half-way between the gradients one step to either side"""
    box = torch.zeros((1, 80))
    for b, j in enumerate((3, 5, 7, 9)):
        box[0, b * 17 + j] = 60.0
    t = torch.tensor([[3.0, 5.0, 7.0, 9.0]])
    lab = torch.zeros(1, dtype=torch.int32)
    for dt in (F32, F64):
        assert torch.all(L64.loc_terms(box.to(dt), t, None, lab, 0, 0.1, 0.5)[2]["sign"] == 0)
    d = torch.tensor([3.0, 5.0, 7.0, 9.0], dtype=F64, requires_grad=True)

    def gl(dd, tt):
        return 1 - L64._ltrb_iou(dd[None], tt[None], None, True)[1]
    g_tie, = torch.autograd.grad(gl(d, t[0].double()).sum(), d)
    eps = 1e-9
    g_lo, = torch.autograd.grad(gl(d, t[0].double() + eps).sum(), d)   # d < t on every side
    g_hi, = torch.autograd.grad(gl(d, t[0].double() - eps).sum(), d)   # d > t
    assert float((g_tie - 0.5 * (g_lo + g_hi)).abs().max()) <= 1e-6 * float(g_lo.abs().min())
    assert float((g_lo - g_hi).abs().min()) > 1e-3


# ---- the comparator tells wrong variants from rounding -----------------------------------------
M_MAX = 16


def _focal_pair(edge, mut, alpha=0.25):
    x, lab = L64.focal_case(257, 80, 31, edge=edge)
    _, r64 = L64.focal(x.double(), lab, 80, alpha, 2.0)
    _, r32 = L64.focal(x, lab, 80, alpha, 2.0)
    _, k = L64.focal(x.double(), lab, 80, alpha, 2.0, mut=mut)
    return k, r64, r32


def _loc_pair(edge, mut, flags=0):
    case = L64.loc_case(129, 80, 32) if edge else L64.benign_loc_case(129, 80, 32)
    r64 = L64.loc_terms(case[0].double(), *case[1:], flags, 0.1, 0.5)[1]
    r32 = L64.loc_terms(*case, flags, 0.1, 0.5)[1]
    k = L64.loc_terms(case[0].double(), *case[1:], flags, 0.1, 0.5, mut=mut)[1]
    return k, r64, r32


def _roi_pair(edge, mut, mode=0):
    c = L64.roi_case(255, 33, edge=edge)
    a = (c["cls"], c["prop"], c["gtb"], c["gstd"], 80, mode, 10.0, 5.0, 62.5, 0.1, 0.5)
    r64 = L64.roi_box_loss(c["mat"][:, :4].double(), c["mat"][:, 4:].double(), *a)[1]
    r32 = L64.roi_box_loss(c["mat"][:, :4], c["mat"][:, 4:], *a)[1]
    k = L64.roi_box_loss(c["mat"][:, :4].double(), c["mat"][:, 4:].double(), *a, mut=mut)[1]
    return k, r64, r32


def _passes(pair):
    k, r64, r32 = pair
    kk, _ = L64.total_and_scale(k)
    a, s = L64.total_and_scale(r64)
    b, _ = L64.total_and_scale(r32)
    return L64.grad_ok(kk, a, b, s, M_MAX)[0]


MUTANTS = [("tie1", _loc_pair, {}), ("nosmooth", _loc_pair, {}), ("certge", _loc_pair, {}), ("tie1", _roi_pair, {}),
           ("clampex", _roi_pair, {}), ("certge", _roi_pair, {"mode": 2}), ("series1", _focal_pair, {}), ("alphaneg", _focal_pair, {"alpha": -1.0})]


@pytest.mark.parametrize("mut,pair,kw", MUTANTS, ids=["%s-%s" % (m, p.__name__[1:-5]) for m, p, _ in MUTANTS])
def test_comparator_rejects_wrong_variant_on_edge_grid(mut, pair, kw):
    assert _passes(pair(True, None, **kw))          # the reference itself passes
    assert not _passes(pair(True, mut, **kw))


def test_tie_and_series_mutants_pass_on_benign_grid():
    """why the edge grids exist: a golden-like draw (logits and std of order 1) never meets a tie or the series switch"""
    assert _passes(_loc_pair(False, "tie1"))
    assert _passes(_focal_pair(False, "series1"))


# ---- every grid of the GPU module: same branch in fp32 and fp64, at most 2 % excluded ----------
CAP = 0.02


def _excluded_ok(p64, p32):
    """fraction of elements without a finite r64 AND r32 (the kernel-independent exclusions of loss_ref64.grad_ratio) within the cap, and
    never a whole row (a row class: every row of the gradient keeps compared elements)"""
    a, _ = L64.total_and_scale(p64)
    b, _ = L64.total_and_scale(p32)
    bad = ~torch.isfinite(a) | ~torch.isfinite(b.double())
    rows = bad.reshape(bad.shape[0], -1)
    return float(bad.double().mean()) <= CAP and not bool(rows.all(dim=1).any())


def test_focal_grids_cover_both_targets_and_stay_under_the_cap():
    for P, C in G.FOCAL_SHAPES:
        x, lab = G.focal_grid(P, C)
        if P >= 257:   # every edge value once as a positive and once as a negative of a live row
            assert L64.focal_edge_coverage(x, lab, C) == ([], []), (P, C)
        for gamma in G.FOCAL_GAMMAS:
            for alpha in G.FOCAL_ALPHAS:
                loss, p64 = L64.focal(x.double(), lab, C, alpha, gamma)
                _, p32 = L64.focal(x, lab, C, alpha, gamma)
                assert _excluded_ok(p64, p32) and bool(torch.isfinite(loss).all()), (P, C, gamma, alpha)
                # the one branch of the formula, x >= 0, is decided by the input itself; the gradients have the same sign in both
                a, b = L64.total_and_scale(p64)[0], L64.total_and_scale(p32)[0].double()
                assert bool(((torch.sign(a) == torch.sign(b)) | (b == 0) | (a == 0)).all())


def test_loc_grids_branch_alike_and_stay_under_the_cap():
    cases = [(G.loc_flag_grid(f, bv), f) for f in L64.LEGAL_FLAGS for bv in (False, True)]
    cases += [(G.loc_shape_grid(P, BS), f) for P, BS in G.LOC_SHAPES for f in G.LOC_SHAPE_FLAGS]
    for case, flags in cases:
        t64, p64, i64 = L64.loc_terms(case[0].double(), *case[1:], flags, 0.1, 0.5)
        _, p32, i32 = L64.loc_terms(*case, flags, 0.1, 0.5)
        assert _excluded_ok(p64, p32) and bool(torch.isfinite(t64).all())
        assert torch.equal(i64["sign"], i32["sign"].double()) and torch.equal(i64["sel"], i32["sel"])   # the same branch
        assert int((i64["sign"] == 0).sum()) >= 4 or case[0].shape[0] == 1


def test_softmax_rpn_roi_grids_branch_alike_and_stay_under_the_cap():
    for C in G.SOFTMAX_C:
        for R in G.SOFTMAX_R:
            x, tgt = G.softmax_grid(R, C)
            for gamma in G.SOFTMAX_GAMMAS:
                loss, g64, _ = L64.softmax_focal(x.double(), tgt, gamma)
                _, g32, _ = L64.softmax_focal(x, tgt, gamma)
                assert _excluded_ok(g64, g32) and bool(torch.isfinite(loss).all())
    for ws in (False, True):
        c = L64.rpn_case(G.RPN_SEED, with_scores=ws)
        o64 = L64.rpn_loss(*L64.rpn_slot_inputs(c, F64), c["anchors"], c["s"], c["gt_boxes"], c["gt_scores"], c["weights"])
        o32 = L64.rpn_loss(*L64.rpn_slot_inputs(c, F32), c["anchors"], c["s"], c["gt_boxes"], c["gt_scores"], c["weights"])
        assert all(bool(torch.isfinite(o).all()) for o in o64 + o32)
        assert torch.equal(o64[3], o32[3].double()) and int((o64[3][0, 2] == 0).sum()) == 3    # delta == target: sign 0 in both
    for R in G.ROI_R:
        c = G.roi_grid(R)
        b64, b32 = L64.roi_branches(c, F64), L64.roi_branches(c, F32)
        assert torch.equal(b64, b32)                                                            # ties, clamp bounds, touching boxes
        if R >= 255:
            assert bool((b64 == 0).any(dim=0)[[1, 3, 12, 13, 14, 15, 16]].all())              # each kind of tie is present
        for mode in range(4):
            a = (c["cls"], c["prop"], c["gtb"], c["gstd"], 80, mode, L64.ROI_W[0], L64.ROI_W[1], L64.ROI_CLAMP, 0.1, 0.5)
            loss, gd, gs = L64.roi_box_loss(c["mat"][:, :4].double(), c["mat"][:, 4:].double(), *a)
            _, gd32, gs32 = L64.roi_box_loss(c["mat"][:, :4], c["mat"][:, 4:], *a)
            assert bool(torch.isfinite(loss).all())
            if R > 1:
                assert _excluded_ok(gd, gd32) and _excluded_ok(gs, gs32), (R, mode)
