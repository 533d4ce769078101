"""MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE "giou" in the two boundary-variance ROI predictors, without a GPU: the fp64
restatement of the five box-loss modes (tests/loss_ref64_roi_beta.py) against the executed reference (tests/golden/roi_beta.npz), its
beta -> 0 limit, a GIoU known answer worked by hand, and what the configuration accepts."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_roi_beta as B64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
BV = ["FocalLoss_BoundaryVar", "CrossEntropy_BoundaryVar"]
MODE = {"nlloss": 0, "smooth_l1": 1, "pseudo": 3, "giou": 4}
K = 3
# the reference ran in fp64 (gen_golden_roi_beta.py) and so does the restatement: the two differ by the order of < 100 fp64 operations
# per element and of 48 additions in the sum - 1e4 units of fp64 roundoff is a wide margin, and 1e-5 of the fp32 resolution
RTOL, ATOL = 1e-11, 1e-13
# nl_loss's 2 log(2 pi) as the reference builds it: a float32 tensor (fast_rcnn.py:1283-1285)
NLL_CONST_REF = float((2 * torch.log(2 * torch.Tensor([math.pi])))[0])


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "roi_beta.npz")))


def T(a):
    return torch.from_numpy(np.asarray(a))


def restated(gold, lay, typ, beta):
    """loss_box_reg and its gradients by the fp64 restatement, normalised like the reference (fast_rcnn.py:1016: / number of rows)"""
    cls, prop, gtb = T(gold["cls"]), T(gold["prop"]).double(), T(gold["gtb"]).double()
    de, st = T(gold["deltas"]).double(), T(gold["std"]).double()
    Rn = float((cls >= 0).sum())
    if lay == "agn":
        loss, gd, gs = B64.roi_box_loss(de[:, :4], st[:, :4], cls, prop, gtb, None, K, MODE[typ], 10.0, 10.0, L64.ROI_CLAMP, 0.1, 0.5, beta,
                                        nll_const=NLL_CONST_REF)
    else:
        loss, gd, gs = B64.roi_box_loss_pc(de, st, cls, prop, gtb, K, MODE[typ], 10.0, 10.0, L64.ROI_CLAMP, beta, nll_const=NLL_CONST_REF)
    return loss.sum() / Rn, L64.total_and_scale(gd)[0] / Rn, L64.total_and_scale(gs)[0] / Rn


@pytest.mark.parametrize("bi", [0, 1, 2])
@pytest.mark.parametrize("typ", sorted(MODE))
@pytest.mark.parametrize("lay", ["agn", "pc"])
def test_fp64_restatement_equals_the_executed_reference(gold, lay, typ, bi):
    beta = float(gold["betas"][bi])
    loss, gd, gs = restated(gold, lay, typ, beta)
    for pred in ("focal", "ce"):                       # both predictors share box_reg_loss / box_reg_pseudo_loss
        q = "%s_%s_%s_b%d" % (pred, lay, typ, bi)
        np.testing.assert_allclose(float(loss), float(gold[q + "_loss"]), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(gd.numpy(), gold[q + "_gdeltas"], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(gs.numpy(), gold[q + "_gstd"], rtol=RTOL, atol=ATOL)
    if typ != "nlloss":
        assert not gs.any()                             # only the NLL term reaches the std head: "giou" gives it no gradient


def test_golden_covers_what_it_claims(gold):
    cls = T(gold["cls"])
    assert {-1, 0, K - 1, K} <= set(cls.tolist()) and gold["betas"].tolist() == [0.0, 0.11, 1.0]
    # beta matters: the three betas give three different losses, except for giou, which has no smooth-L1 term
    for lay in ("agn", "pc"):
        for typ in ("smooth_l1", "nlloss", "pseudo"):
            v = [float(gold["focal_%s_%s_b%d_loss" % (lay, typ, i)]) for i in range(3)]
            assert v[0] > v[1] > v[2] > 0
        v = [float(gold["focal_%s_giou_b%d_loss" % (lay, i)]) for i in range(3)]
        assert v[0] == v[1] == v[2] > 0
    # both sides of beta 0.11 occur among the foreground |d - t|
    fg = (cls >= 0) & (cls < K)
    g1 = T(gold["focal_agn_smooth_l1_b1_gdeltas"])[fg].abs() * float((cls >= 0).sum())
    assert ((g1 - 1).abs() < 1e-12).any() and ((g1 > 0) & (g1 < 0.999)).any()


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_beta_to_zero_is_the_l1_loss(mode):
    """below 1e-5 fvcore switches to plain L1; just above it the quadratic zone is 1e-5 wide and the linear branch is |d| - 0.5 beta:
    on R rows with |d - t| > beta everywhere the sum differs from the L1 sum by exactly 4 nfg * 0.5 beta, the gradients not at all"""
    c = L64.roi_case(64, 3, edge=False)
    a = (c["cls"], c["prop"], c["gtb"], None, 80, mode, 10.0, 5.0, L64.ROI_CLAMP, 0.1, 0.5)
    de, st = c["mat"][:, :4].double(), c["mat"][:, 4:].double()
    l0, gd0, gs0 = L64.roi_box_loss(de, st, *a)
    nfg = int(((c["cls"] >= 0) & (c["cls"] < 80)).sum())
    for beta in (0.0, 9e-6):                           # fvcore's L1 switch: the existing restatement, unchanged
        l, gd, gs = B64.roi_box_loss(de, st, *a, beta)
        assert torch.equal(l, l0) and all(torch.equal(x, y) for x, y in zip(gd + gs, gd0 + gs0))
    beta = 2e-5
    l, gd, gs = B64.roi_box_loss(de, st, *a, beta)
    assert abs(float(l0.sum() - l.sum()) - 4 * nfg * 0.5 * beta) < 1e-12
    assert torch.allclose(L64.total_and_scale(gd)[0], L64.total_and_scale(gd0)[0], rtol=0, atol=1e-15)
    assert torch.allclose(L64.total_and_scale(gs)[0], L64.total_and_scale(gs0)[0], rtol=0, atol=1e-15)
    # the restated modes at beta 0 (nll_const given: no delegation) are the existing restatement
    l, gd, gs = B64.roi_box_loss(de, st, *a, 0.0, nll_const=B64.NLL_CONST)
    assert torch.allclose(l, l0, rtol=1e-14, atol=0)
    assert torch.allclose(L64.total_and_scale(gd)[0], L64.total_and_scale(gd0)[0], rtol=1e-13, atol=1e-15)
    assert torch.allclose(L64.total_and_scale(gs)[0], L64.total_and_scale(gs0)[0], rtol=1e-13, atol=1e-15)


def test_smooth_l1_on_and_around_beta():
    x = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 2.0, -2.0], dtype=torch.float64, requires_grad=True)
    y = B64.smooth_l1(x, 0.5)
    assert y.tolist() == [0.0, 0.0625, 0.0625, 0.25, 0.25, 1.75, 1.75]      # |x| == beta: the linear side, 0.5 - 0.25
    g, = torch.autograd.grad(y.sum(), x)
    assert g.tolist() == [0.0, 0.5, -0.5, 1.0, -1.0, 1.0, -1.0]


def test_giou_known_answer_for_two_boxes():
    """a = (0, 0, 2, 2), b = (1, 1, 3, 3): I = 1, U = 4 + 4 - 1 = 7, enclosing box (0, 0, 3, 3): C = 9; GIoU = 1/7 - (9 - 7)/9 = -5/63,
    loss = 68/63.  Through the decode: proposal (0, 0, 2, 2), weights (10, 5), deltas (5, 5, 2.5, 2.5) move it by half a side = 1 pixel
    to (1, 1, 3, 3); against the gt (0, 0, 2, 2) the same two boxes.  d loss / d x1 of the moved box: dI = -1, dU = -2 + 1 = -1, dC = 0:
    d iou = (-1 * 7 + 1) / 49 = -6/49, d penalty = (1 * 9) / 81 = 1/9, d loss = 1/9 + 6/49 = 103/441; times d x1 / d delta = w / wx = 0.2."""
    a = torch.tensor([[0.0, 0.0, 2.0, 2.0]], dtype=torch.float64)
    b = torch.tensor([[1.0, 1.0, 3.0, 3.0]], dtype=torch.float64)
    assert abs(float(B64.giou_loss(a, b)[0]) - 68.0 / 63.0) < 1e-7           # (eps 1e-7 in both denominators)
    assert abs(float(B64.giou_loss(a, a)[0])) < 1e-7                          # identical boxes: 0
    far = torch.tensor([[4.0, 0.0, 6.0, 2.0]], dtype=torch.float64)          # disjoint: I = 0, U = 8, C = 12: 1 + 4/12
    assert abs(float(B64.giou_loss(a, far)[0]) - 4.0 / 3.0) < 1e-7
    de = torch.tensor([[5.0, 5.0, 2.5, 2.5]], dtype=torch.float64)
    cls = torch.tensor([1])
    loss, gd, gs = B64.roi_box_loss(de, torch.zeros(1, 4, dtype=torch.float64), cls, a, a, None, 3, 4, 10.0, 5.0, L64.ROI_CLAMP, 0.0, 0.0)
    assert abs(float(loss[0]) - 68.0 / 63.0) < 1e-7
    assert abs(float(gd[0][0, 0]) - 0.2 * 103.0 / 441.0) < 1e-7 and not gs[0].any()
    # a zero-area prediction (x1 == x2) inside the gt box: I = 0, U = C = the gt area: loss 1
    de0 = torch.tensor([[5.0, -5.0, 0.0, 0.0]], dtype=torch.float64)
    assert abs(float(B64.roi_box_loss(de0, de0, cls, a, a, None, 3, 4, 10.0, 5.0, L64.ROI_CLAMP, 0.0, 0.0)[0][0]) - 1.0) < 1e-6


def cfg_of(*over):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", "cpu"] + list(over))


@pytest.mark.parametrize("agnostic", [True, False])
@pytest.mark.parametrize("loss", BV)
def test_giou_builds_on_both_boundary_variance_predictors(loss, agnostic):
    from ubteacher.modeling import build_model
    m = build_model(cfg_of("MODEL.ROI_HEADS.LOSS", loss, "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou", "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", 0.11,
                           "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", agnostic, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "smooth_l1"))
    pred = m.roi_heads.box_predictor
    assert pred.box_reg_loss_type == "giou" and pred.BOX_LOSS_MODE["giou"] == 4 and pred.smooth_l1_beta == 0.11
    assert pred.nbox == (1 if agnostic else 80)
    assert pred.BOX_LOSS_MODE == {"nlloss": 0, "smooth_l1": 1, "giou": 4}


@pytest.mark.parametrize("loss", BV)
def test_invalid_box_loss_types_still_raise(loss):
    from ubteacher.modeling import build_model
    with pytest.raises(ValueError, match="Invalid bbox reg loss type 'diou'"):
        build_model(cfg_of("MODEL.ROI_HEADS.LOSS", loss, "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "diou"))
    with pytest.raises(ValueError, match="Invalid bbox pseudo reg loss type 'giou'"):      # the pseudo branch keeps its own key and values
        build_model(cfg_of("MODEL.ROI_HEADS.LOSS", loss, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "giou"))
    with pytest.raises(NotImplementedError):                                                # the per-class tsbetter refusal stays
        build_model(cfg_of("MODEL.ROI_HEADS.LOSS", loss, "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou",
                           "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "tsbetter"))


def test_binding_declares_the_new_entry_point_next_to_the_old():
    from ubteacher import hip
    assert {"utv2_roi_box_loss", "utv2_roi_box_loss_f"} <= set(hip.symbols())
    old, new = hip._SIGS["utv2_roi_box_loss"][1], hip._SIGS["utv2_roi_box_loss_f"][1]
    assert len(new) == len(old) + 1 and new[:16] == old[:16] and new[16] is hip.c_f and new[17:] == old[16:]
    for kind in ("bf16", "fp16"):                      # both libraries export it (load() binds every declared symbol)
        assert hasattr(hip.load(kind), "utv2_roi_box_loss_f")
