"""The RPN's loss, boundary and anchor-generator keys without a GPU: the fp64 restatement (tests/rpn_ref64.py) against the executed
reference (tests/golden/rpn_keys.npz), the 2 % comparator cap on the GPU tests' input grids, and what the configuration accepts."""
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import rpn_ref64 as R64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
# the reference ran in fp64 (gen_golden_rpn_keys.py) and so does the restatement: they differ by the order of < 100 fp64 operations per
# element and of < 100 additions per sum (the bound of tests/test_roi_box_beta.py)
RTOL, ATOL = 1e-11, 1e-13
HW, STRIDES = [(6, 8), (3, 4)], [16, 32]
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "rpn_keys.npz")))


def T(a):
    return torch.from_numpy(np.asarray(a))


def scene(gold):
    """the golden scene in the product's padded form: gt_boxes [2, 3, 4] / valid / scores, image sizes"""
    gt = torch.zeros((2, 3, 4))
    gt[0] = T(gold["gt0"]).float()
    valid = torch.tensor([[1, 1, 1], [0, 0, 0]], dtype=torch.uint8)
    sc = torch.zeros((2, 3))
    sc[0] = T(gold["sc0"]).float()
    return gt, valid, sc, [tuple(int(v) for v in s) for s in gold["sizes"]]


def labels_to_sample(lab):
    """labels after the subsampling [N, R] -> the samplers' padded dict (index order)"""
    N = lab.shape[0]
    npos, nneg = int((lab == 1).sum(1).max()), int((lab == 0).sum(1).max())
    s = dict(pos_idx=torch.zeros((N, npos), dtype=torch.int64), pos_valid=torch.zeros((N, npos), dtype=torch.uint8),
             neg_idx=torch.zeros((N, nneg), dtype=torch.int64), neg_valid=torch.zeros((N, nneg), dtype=torch.uint8))
    for n in range(N):
        for k, v in (("pos", 1), ("neg", 0)):
            i = torch.nonzero(lab[n] == v).squeeze(1)
            s[k + "_idx"][n, :i.numel()] = i
            s[k + "_valid"][n, :i.numel()] = 1
    return s


@pytest.mark.parametrize("ti", [0, 1, 2])
def test_labels_and_samples_equal_the_executed_reference(gold, ti):
    gt, valid, _, sizes = scene(gold)
    t = float(gold["thresholds"][ti])
    lab, _ = R64.rpn_labels(T(gold["anchors"]).float(), gt, valid, sizes, 0.3, 0.7, t)
    assert np.array_equal(lab.numpy(), gold["labels_t%d" % ti])
    s = R64.sample(lab, T(gold["keys"]).float(), int(gold["batch"]), float(gold["frac"]))
    got = torch.full_like(lab, -1)
    for n in range(2):
        got[n, s["pos_idx"][n][s["pos_valid"][n].bool()]] = 1
        got[n, s["neg_idx"][n][s["neg_valid"][n].bool()]] = 0
    assert np.array_equal(got.numpy(), gold["sampled_t%d" % ti])
    # the scene does hold what it is there for (image 0 is 80 x 104)
    a, l0 = T(gold["anchors"]), T(gold["labels_t0"])[0]
    assert np.all(gold["labels_t%d" % ti][1] == (0 if t < 0 else np.where(R64.inside_box(a, sizes[1], t), 0, -1)))   # the image without gt
    if t == 0.0:
        edge = (a[:, 2] == 104.0) & (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 3] < 80)         # x2 == W + t: outside
        zero = (a[:, 0] == 0.0) & (a[:, 1] >= 0) & (a[:, 2] < 104) & (a[:, 3] < 80)          # x1 == -t: inside
        lowq = torch.nonzero((a == torch.tensor([-8.0, -8.0, 8.0, 8.0])).all(1)).squeeze(1)
        assert edge.any() and zero.any() and lowq.numel() == 1 and int(l0[lowq]) == 1       # a low-quality match (IoU 0.19) ...
        assert np.all(gold["labels_t1"][0][edge.numpy()] == -1) and np.all(gold["labels_t1"][0][zero.numpy()] >= 0)
        assert int(gold["labels_t1"][0][int(lowq)]) == -1                                    # ... that lies outside is ignored
    if t == 8.0:
        edge = (a[:, 3] == 88.0) & (a[:, 0] >= -8) & (a[:, 1] >= -8) & (a[:, 2] < 112)       # y2 == H + t: outside
        inn = (a[:, 0] == -8.0) & (a[:, 1] >= -8) & (a[:, 2] < 112) & (a[:, 3] < 88)         # x1 == -t: inside
        assert edge.any() and inn.any()
        assert np.all(gold["labels_t2"][0][edge.numpy()] == -1) and np.all(gold["labels_t2"][0][inn.numpy()] >= 0)


@pytest.mark.parametrize("typ,bi", [("smooth_l1", 0), ("smooth_l1", 1), ("smooth_l1", 2), ("giou", 0)])
def test_fp64_loss_restatement_equals_the_executed_reference(gold, typ, bi):
    gt, valid, sc, sizes = scene(gold)
    anchors = T(gold["anchors"])
    _, matched = R64.rpn_labels(anchors.float(), gt, valid, sizes, 0.3, 0.7, -1.0)
    lab = T(gold["sampled_t0"])
    s = labels_to_sample(lab)
    s["matched32"], s["has_gt"] = matched, valid.any(dim=1, keepdim=True).to(torch.uint8)
    obj, deltas = T(gold["obj"]).double(), T(gold["deltas"]).double()
    idx = torch.cat((s["pos_idx"], s["neg_idx"]), dim=1)
    x = torch.gather(obj, 1, idx)
    dl = torch.gather(deltas, 1, s["pos_idx"][..., None].expand(-1, -1, 4))
    beta = float(gold["betas"][bi])
    cls, loc, gobj, gdl, _ = R64.rpn_loss(x, dl, anchors.double(), s, gt.double(), sc.double(), (1.0, 1.0, 1.0, 1.0),
                                       loc_mode=int(typ == "giou"), beta=beta)
    norm = float(gold["batch"]) * 2
    q = "%s_b%d" % (typ, bi)
    valid_s = torch.cat((s["pos_valid"], s["neg_valid"]), dim=1).bool()
    # loss_rpn_cls, which none of the keys touches, is the one value the reference does not form in fp64: rpn.py:207-212 casts the BCE
    # target to float32, and ATen then builds every term in the target's buffer.  Its VALUE is held to the fp64 restatement at four fp32
    # roundings per term, and to the same ATen call on the restatement's operands at the fp64 bound; its gradient is fp64 (autograd)
    np.testing.assert_allclose(float(cls.sum()) / norm, float(gold[q + "_loss_cls"]), rtol=4 * L64.U, atol=0)
    tgt32 = torch.cat((torch.ones(s["pos_idx"].shape), torch.zeros(s["neg_idx"].shape)), dim=1)
    w = torch.gather(sc.double(), 1, torch.gather(matched.long(), 1, idx)) * s["has_gt"].double()
    as_ref = torch.nn.functional.binary_cross_entropy_with_logits(x[valid_s], tgt32[valid_s], weight=w[valid_s], reduction="sum")
    np.testing.assert_allclose(float(as_ref) / norm, float(gold[q + "_loss_cls"]), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(loc.sum()) / norm, float(gold[q + "_loss_loc"]), rtol=RTOL, atol=ATOL)
    go, gd = torch.zeros_like(obj), torch.zeros_like(deltas)
    gdl = L64.total_and_scale(gdl)[0]
    for n in range(2):
        go[n, idx[n][valid_s[n]]] = gobj[n][valid_s[n]] / norm
        pv = s["pos_valid"][n].bool()
        gd[n, s["pos_idx"][n][pv]] = gdl[n][pv] / norm
    np.testing.assert_allclose(go.numpy(), gold[q + "_gobj"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gd.numpy(), gold[q + "_gdeltas"], rtol=RTOL, atol=ATOL)
    assert float(gold[q + "_loss_loc"]) > 0 and np.abs(gold[q + "_gdeltas"]).max() > 0
    if typ == "smooth_l1" and bi:                        # the golden deltas do fall on both sides of this beta
        d = np.abs(gold[q + "_gdeltas"][gold[q + "_gdeltas"] != 0]) * norm
        assert (d < 1 - 1e-9).any() and (np.abs(d - 1) < 1e-12).any()


def test_anchor_tables_equal_the_restated_generator(gold):
    from ubteacher.modeling.rcnn import AnchorGenerator
    from ubteacher.presets import get_config
    lv = [(8, 6), (4, 3)]
    for name, sizes, ratios, off, A in (("a6", [[32, 64]], [[0.5, 1.0, 2.0]], 0.0, 6), ("a1", [[32], [64]], [[1.0]], 0.0, 1),
                                        ("off", [[32], [64]], [[0.5, 1.0, 2.0]], 0.5, 3)):
        ref = R64.anchor_tables(lv, STRIDES, sizes, ratios, off)
        cfg = get_config("rcnn", 1, ["MODEL.DEVICE", "cpu", "MODEL.ANCHOR_GENERATOR.SIZES", sizes, "MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS", ratios,
                                     "MODEL.ANCHOR_GENERATOR.OFFSET", off])
        ag = AnchorGenerator(cfg, STRIDES)
        assert ag.A == A
        for l, (r, p) in enumerate(zip(ref, ag(lv, "cpu"))):
            want = gold["anc_%s_l%d" % (name, l)]
            assert want.shape == (lv[l][0] * lv[l][1] * A, 4)
            assert np.array_equal(r.numpy(), want) and np.array_equal(p.numpy(), want)
    assert float(gold["anc_off_l0"][0, 0] + gold["anc_off_l0"][0, 2]) == 16.0      # OFFSET 0.5: the first cell is centred on half a stride


# ---- the 2 % cap of the comparator on the GPU tests' grids --------------------------------------------------------------------------------
MODES = [(0, 0.0), (0, 0.11), (0, 1.0), (1, 0.0)]


@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("mode,beta", MODES)
@pytest.mark.parametrize("A", [1, 3, 6])
def test_grids_leave_the_comparator_its_two_percent(A, mode, beta, with_scores):
    """fp32 autograd against fp64 autograd alone: at most 2 % of a case may fall outside loss_ref64.grad_ratio's rule (grad_ok's cap)"""
    beta = float(torch.tensor(beta, dtype=F32))
    c = R64.rpn_key_case(77 + A, A=A, beta=beta, with_scores=with_scores, giou=mode == 1)
    ref = {}
    for dt in (F64, F32):
        x, dl = L64.rpn_slot_inputs(c, dt)
        ref[dt] = R64.rpn_loss(x, dl, c["anchors"], c["s"], c["gt_boxes"], c["gt_scores"], c["weights"], mode, beta)
    g64, s64 = L64.total_and_scale(ref[F64][3])[0], ref[F64][4]
    g32, _ = L64.total_and_scale(ref[F32][3])
    for k, r64, r32, s in ((g32, g64, g32, s64), (ref[F32][2], ref[F64][2], ref[F32][2], None)):
        res = L64.grad_ratio(k, r64, r32, s)
        assert res["excluded"] <= 0.02 and res["class_ok"], res
    assert torch.isfinite(ref[F64][1]).all() and float(ref[F64][1].sum()) > 0
    rows = c["rows"]
    x, dl = L64.rpn_slot_inputs(c, F32)
    if mode == 0 and beta:                                # |d| == beta bit for bit, one ulp below, one above: slots 3, 4, 5 of image 0
        assert torch.all(dl[0, 3].abs() == beta) and torch.all(dl[0, 4].abs() < beta) and torch.all(dl[0, 5].abs() > beta)
        assert torch.all(g64[0, 3].abs() == 1.0) and torch.all(g64[0, 4].abs() < 1.0) and torch.all(g64[0, 5].abs() == 1.0)
    if mode == 1:
        assert float(ref[F64][1][0, 3]) > 1.0 and 0 < float(ref[F64][1][0, 4]) < 1.0        # disjoint: loss > 1; contained
        assert float(g64[0, 6, 2]) == 0.0 and float(g64[0, 6, 3]) != 0.0                    # dw above SCALE_CLAMP: derivative exactly 0
    assert len(set(rows)) == 4


# ---- configuration --------------------------------------------------------------------------------------------------------------------------
def cfg_of(*over):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", "cpu"] + list(over))


def rpn_of(*over):
    from ubteacher.modeling import build_model
    return build_model(cfg_of(*over)).proposal_generator


def test_shipped_keys_build_the_sixteen_channel_head():
    from ubteacher.modeling import rcnn as R_
    rpn = rpn_of()
    assert rpn.A == 3 and rpn.ch == 16 == R_.RPN_CH == R_.rpn_channels(3)
    assert (rpn.loc_mode, rpn.smooth_l1_beta, rpn.boundary_thresh, rpn.anchor_generator.offset) == (0, 0.0, -1.0, 0.0)
    assert [R_.rpn_channels(a) for a in (1, 4, 6, 9, 15)] == [16, 32, 32, 48, 80]


def test_rpn_keys_are_read():
    rpn = rpn_of("MODEL.RPN.SMOOTH_L1_BETA", 0.11, "MODEL.RPN.BOUNDARY_THRESH", 0)
    assert (rpn.loc_mode, rpn.smooth_l1_beta, rpn.boundary_thresh) == (0, 0.11, 0.0)
    assert rpn_of("MODEL.RPN.BBOX_REG_LOSS_TYPE", "giou").loc_mode == 1
    rpn = rpn_of("MODEL.ANCHOR_GENERATOR.SIZES", [[32, 64], [64, 128], [128, 256], [256, 512], [512, 640]])
    assert rpn.A == 6 and rpn.ch == 32
    assert rpn_of("MODEL.RPN.CONV_DIMS", [256]).ch == 16


def test_refusals_name_their_keys():
    with pytest.raises(ValueError, match="Invalid dense box regression loss type 'diou'"):
        rpn_of("MODEL.RPN.BBOX_REG_LOSS_TYPE", "diou")
    with pytest.raises(NotImplementedError, match="ANCHOR_GENERATOR.SIZES"):
        rpn_of("MODEL.ANCHOR_GENERATOR.SIZES", [[16, 32, 64, 128]], "MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS", [[0.25, 0.5, 1.0, 2.0]])   # A = 16
    with pytest.raises(NotImplementedError, match="MODEL.ANCHOR_GENERATOR.NAME"):
        rpn_of("MODEL.ANCHOR_GENERATOR.NAME", "RotatedAnchorGenerator")
    with pytest.raises(NotImplementedError, match="MODEL.RPN.HEAD_NAME"):
        rpn_of("MODEL.RPN.HEAD_NAME", "MyHead")
    with pytest.raises(NotImplementedError, match="MODEL.RPN.CONV_DIMS"):
        rpn_of("MODEL.RPN.CONV_DIMS", [256, 256])
    with pytest.raises(ValueError, match="MODEL.ANCHOR_GENERATOR.SIZES.*MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS"):
        rpn_of("MODEL.ANCHOR_GENERATOR.SIZES", [[32], [64], [128, 192], [256], [512]])                 # unequal A per level
    with pytest.raises(ValueError, match="MODEL.ANCHOR_GENERATOR.OFFSET"):
        rpn_of("MODEL.ANCHOR_GENERATOR.OFFSET", 1.0)


def test_binding_declares_the_new_entry_points_next_to_the_old():
    from ubteacher import hip
    S = hip._SIGS
    for old, new in (("utv2_rpn_loss_fwd", "utv2_rpn_loss_fwd_f"), ("utv2_rpn_loss_fwd_range", "utv2_rpn_loss_fwd_range_f")):
        o, n = S[old][1], S[new][1]
        assert len(n) == len(o) + 3 and n[:len(o) - 4] == o[:-4] and n[len(o) - 4:len(o) - 1] == [hip.c_i, hip.c_f, hip.c_f] and n[-4:] == o[-4:]
    o, n = S["utv2_rpn_sample_keys"][1], S["utv2_rpn_sample_keys_b"][1]
    assert len(n) == len(o) + 3 and n[:9] == o[:9] and n[9:12] == [hip.c_p, hip.c_p, hip.c_f] and n[12:] == o[9:]
    for kind in ("bf16", "fp16"):
        for name in ("utv2_rpn_loss_fwd_f", "utv2_rpn_loss_fwd_range_f", "utv2_rpn_sample_keys_b"):
            assert hasattr(hip.load(kind), name)
