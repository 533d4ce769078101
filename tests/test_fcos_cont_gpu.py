"""The continuous FCOS regression head (MODEL.FCOS.REG_DISCRETE False) on the GPU.

Kernels (csrc/fcos.hip utv2_fcos_loc_terms_cont_*, utv2_fcos_decode_cont) element by element against the fp64 autograd reference of
tests/loss_ref64_cont.py with the rule of tests/test_loss_kernels_fp64_gpu.py: |k - r64| <= M max(|r32 - r64|, u |r64|) + M u s, s = the
loss-part addends, no absolute tolerance, M = that file's M_LOC (4); forward sums |k - sum r64| <= (L + D + 2 M) u sum |r64_i| with the
same launch geometry (at most 512 blocks x 128 threads, one row per thread and trip: L = ceil(P / 65536), D = D_BLOCK).
Each test prints its worst ratio before it asserts.

Whole path against the executed-reference goldens of tests/golden/gen_golden_fcos_cont.py with the tolerances of
tests/test_fcos_kernels_gpu.py / tests/test_fcos_step_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64_cont as C64
from tests.test_loss_kernels_fp64_gpu import COEF4, D_BLOCK, EARG, M_LOC, bits, check_grad, check_sum, dev, same_bits
from tests.loss_ref64 import LEGAL_FLAGS, LT_KLLOSS, LT_QUALITY_IOU

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE = 16                      # modeling.fcos.BOX_STRIDE_CONT
CONT_P = [0, 1, 127, 128, 129, 1000]      # the launch bound is 128: either side of a block edge, several blocks
CONT_BS = [STRIDE, 80]
SHAPE_FLAGS = [0, 7, 26]


def hip():
    from ubteacher import hip as H
    return H


def shape_grid(P, BS):
    case = C64.cont_case(max(P, 1), BS, 700 + P + BS)
    if P == 1:
        case[3][0] = 3
    return case if P > 0 else tuple(None if x is None else x[:0].contiguous() for x in case)


def flag_grid(flags, with_bvars):
    return C64.cont_case(129, STRIDE, 900 + flags, with_bvars=with_bvars)


def run(case, flags, tag, tsb=C64.TS_BETTER, tsc=C64.TS_CERT):
    H = hip()
    box, t, bv, lab = case
    P, BS = box.shape
    coef = [float(torch.tensor(c, dtype=F32)) for c in COEF4]
    t64 = C64.loc_terms_cont(box.double(), t, bv, lab, flags, tsb, tsc, coef=coef)
    t32 = C64.loc_terms_cont(box, t, bv, lab, flags, tsb, tsc, coef=coef)
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, tsb, tsc)
    s1 = H.fcos_loc_terms_cont_fwd(*args, flags=flags).cpu()
    s2 = H.fcos_loc_terms_cont_fwd(*args, flags=flags).cpu()
    assert same_bits(s1, s2)
    for col in range(7):
        check_sum("%s col%d" % (tag, col), s1[col], t64[0][:, col], math.ceil(P / 65536), D_BLOCK, M_LOC)
    assert float(s1[7]) == 0.0
    g = H.fcos_loc_terms_cont_bwd(*args, dev(torch.tensor(COEF4, dtype=F32)), flags=flags)
    g2 = H.fcos_loc_terms_cont_bwd(*args, dev(torch.tensor(COEF4, dtype=F32)), flags=flags)
    assert same_bits(g, g2)
    check_grad(tag, g, t64[1], t32[1], M_LOC)
    gc = g.cpu()
    nonpos = (lab < 0) | (lab == 80)
    assert torch.all(gc[nonpos] == 0) and torch.all(gc[:, 9:] == 0)
    return s1, gc, t64


@pytest.mark.parametrize("with_bvars", [False, True])
@pytest.mark.parametrize("flags", LEGAL_FLAGS)
def test_cont_loc_terms_all_flags_vs_fp64(flags, with_bvars):
    run(flag_grid(flags, with_bvars), flags, "cont f%d bv%d" % (flags, with_bvars))


@pytest.mark.parametrize("BS", CONT_BS)
@pytest.mark.parametrize("P", CONT_P)
def test_cont_loc_terms_shapes_vs_fp64(P, BS):
    H = hip()
    case = shape_grid(P, BS)
    if P == 0:   # sums = 0, the backward writes nothing
        box, t, bv, lab = (torch.zeros((0, BS)), torch.zeros((0, 4)), torch.zeros((0, 4)), torch.zeros(0, dtype=torch.int32))
        one = torch.full((4, BS), 7.0, device=DEV)
        st, p = H._stream(), (lambda a: a.data_ptr())
        sums = torch.full((8,), 7.0, device=DEV)
        ws = torch.zeros(4096, device=DEV)
        H.call("utv2_fcos_loc_terms_cont_fwd", p(one), p(one), BS, p(one), None, 0, 80, 0.1, 0.5, 0, p(sums), p(ws), st)
        assert torch.all(bits(sums) == 0)
        H.call("utv2_fcos_loc_terms_cont_bwd", p(one), p(one), BS, p(one), None, 0, 80, 0.1, 0.5, 0, p(sums), p(one), st)
        H.call("utv2_fcos_loc_terms_cont_bwd_acc", p(one), p(one), BS, p(one), None, 0, 80, 0.1, 0.5, 0, p(sums), None, p(one), 0, st)
        assert torch.all(one.cpu() == 7.0)
        return
    for flags in SHAPE_FLAGS:
        run(case, flags, "cont P%d BS%d f%d" % (P, BS, flags))


def rows_of(kind, P=48):
    return [r for r in range(P) if r % 12 == kind]


def test_cont_stored_zero_negative_and_minus_zero_have_no_gradient():
    """rows 1 (all 0), 2 (two sides negative), 3 (-0.0): d = 0 there in the forward, gradient exactly 0 on those columns"""
    case = C64.cont_case(48, STRIDE, 11, labels_mode="positive")
    for flags in (0, LT_KLLOSS):
        _, g, t64 = run(case, flags, "cont relu f%d" % flags)
        dead = case[0][:, 0:4] <= 0                     # 0, -0.0 and negatives
        assert int(dead.sum()) >= 30 and torch.all(g[:, 0:4][dead] == 0)
        for r in rows_of(1) + rows_of(4):
            assert bool(dead[r].all())
        for r in rows_of(3):
            assert g[r, 0] == 0 and g[r, 2] == 0 and g[r, 1] != 0 and g[r, 3] != 0
        assert torch.all(t64[2]["d"][rows_of(1)] == 0)


def test_cont_all_four_distances_dead_iou_is_one_over_target_area_plus_one():
    H = hip()
    box, t, bv, lab = C64.cont_case(48, STRIDE, 12, labels_mode="positive")
    for r in rows_of(4):
        s = H.fcos_loc_terms_cont_fwd(dev(lab[r:r + 1]), dev(box[r:r + 1].contiguous()), dev(t[r:r + 1].contiguous()), None, 80, 0.0, 0.0,
                                      flags=LT_QUALITY_IOU).cpu()
        ta = (t[r, 0].double() + t[r, 2].double()) * (t[r, 1].double() + t[r, 3].double())
        want = 1.0 / (ta + 1.0)
        assert abs(float(s[1]) - float(want)) <= 2 * 2.0 ** -24 * float(want), (float(s[1]), float(want))   # one division, one rounding of ta + 1
    run((box, t, bv, lab), LT_QUALITY_IOU, "cont dead")


@pytest.mark.parametrize("flags", [0, 4, 8, LT_KLLOSS])
def test_cont_ties_d_equals_t(flags):
    """rows 5 (all sides tie) and 6 (one side ties, the others on either side): min / max split the gradient half / half, the L1 and
    smooth-L1 terms have gradient 0 at the tie - as autograd has it"""
    case = C64.cont_case(48, STRIDE, 13, labels_mode="positive")
    _, g, t64 = run(case, flags, "cont tie f%d" % flags)
    assert int((t64[2]["sign"][rows_of(5)] == 0).sum()) == 16


def test_cont_smooth_l1_switch_at_one():
    case = C64.cont_case(48, STRIDE, 14, labels_mode="positive")
    _, _, t64 = run(case, LT_KLLOSS, "cont sl1")
    d, t = t64[2]["d"][rows_of(7)], case[1][rows_of(7)].double()
    assert int(((d - t).abs() == 1.0).sum()) >= 8


def test_cont_selection_thresholds_are_strict():
    """ct == ts_cert (bvars logit 0 -> ct = 0.5 exactly) and ct == cs + ts_better (equal logits, ts_better 0): not selected"""
    H = hip()
    case = C64.cont_case(48, STRIDE, 15, labels_mode="positive")
    s, _, t64 = run(case, 0, "cont cert")
    assert float(s[5]) == float(t64[2]["sel"].sum()) and not bool(t64[2]["sel"][rows_of(8)].any())
    box, t, bv, lab, tsb, tsc = C64.better_tie_case(STRIDE)
    s, _, t64 = run((box, t, bv, lab), 0, "cont better", tsb, tsc)
    assert float(s[5]) == 8.0 and t64[2]["sel"].sum(dim=1).tolist() == [0, 4, 0, 0, 4, 0]


@pytest.mark.parametrize("mode", ["skipped", "background", "mixed"])
def test_cont_labels_skipped_background_mixed(mode):
    H = hip()
    case = C64.cont_case(129, STRIDE, 16, labels_mode=mode)
    if mode == "mixed":
        run(case, 0, "cont labels mixed")
        return
    box, t, bv, lab = case
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, 0.1, 0.5)
    assert torch.all(bits(H.fcos_loc_terms_cont_fwd(*args)) == 0)
    assert torch.all(bits(H.fcos_loc_terms_cont_bwd(*args, dev(torch.tensor(COEF4, dtype=F32)))) == 0)


@pytest.mark.parametrize("flags", [0, 4, LT_KLLOSS])
def test_cont_small_and_large_targets(flags):
    case = C64.cont_case(48, STRIDE, 17, labels_mode="positive")
    _, g, _ = run(case, flags, "cont range f%d" % flags)
    assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("BS", CONT_BS)
def test_cont_loc_terms_bwd_acc_semantics(BS):
    H = hip()
    P = 129
    box, t, bv, lab = C64.cont_case(P, BS, 21)
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, 0.1, 0.5)
    c4 = torch.tensor(COEF4, dtype=F32)
    c8 = torch.tensor([9.0, 9.0, COEF4[0], COEF4[1], COEF4[2], 9.0, COEF4[3], 9.0], dtype=F32)
    g0 = H.fcos_loc_terms_cont_bwd(*args, dev(c4), flags=0).cpu()
    ga = H.fcos_loc_terms_cont_bwd_acc(*args, dev(c8), None, torch.full((P, BS), 7.0, device=DEV), False, flags=0).cpu()
    gb = H.fcos_loc_terms_cont_bwd_acc(*args, dev(c8), dev(torch.ones(1)), torch.full((P, BS), 7.0, device=DEV), False, flags=0).cpu()
    assert same_bits(g0, ga) and same_bits(g0, gb)            # accumulate 0 writes zeros on rows without a gradient
    pre = torch.randn((P, BS), generator=torch.Generator().manual_seed(6))
    pre[13, 0] = float("nan")                                 # a skipped row
    gc = H.fcos_loc_terms_cont_bwd_acc(*args, dev(c8), None, dev(pre.clone()), True, flags=0).cpu()
    gd = H.fcos_loc_terms_cont_bwd_acc(*args, dev(c8), None, dev(pre.clone()), True, flags=0).cpu()
    assert same_bits(gc, gd)
    nonpos = (lab < 0) | (lab == 80)
    assert int(lab[13]) == -1 and same_bits(gc[nonpos], pre[nonpos])
    assert same_bits(gc[~nonpos][:, :9], (pre + g0)[~nonpos][:, :9])
    assert same_bits(gc[:, 9:], pre[:, 9:])                   # the pad columns are untouched under accumulate


def test_cont_bad_arguments_are_refused():
    from tests.test_fcos_cont import bad_argument_rows
    H = hip()
    lib = H.load()
    one = torch.zeros(4096, device=DEV)
    for name, args in bad_argument_rows(one.data_ptr()):
        assert getattr(lib, name)(*args) == -1000, (name, args)
    torch.cuda.synchronize()
    assert torch.all(one.cpu() == 0)
    with pytest.raises(RuntimeError, match=EARG):
        H.fcos_loc_terms_cont_fwd(one[:5].int(), one[:40].view(5, 8), one[:20].view(5, 4), None, 80, 0.1, 0.5)   # box_stride 8


# ---- decode -------------------------------------------------------------------------------------
def test_decode_cont_empty_slots_two_images_two_levels():
    H = hip()
    g = torch.Generator().manual_seed(3)
    N, C, BS = 2, 5, STRIDE
    levels = [(3, 4, 8), (2, 2, 16)]          # (h, w, stride)
    K = [7, 3]
    MAXC = sum(K)
    outs = dict(boxes=torch.full((N, MAXC, 4), 9.0, device=DEV), scores=torch.full((N, MAXC), 9.0, device=DEV),
                classes=torch.full((N, MAXC), 9, dtype=torch.int32, device=DEV), locations=torch.full((N, MAXC, 2), 9.0, device=DEV),
                centerness=torch.full((N, MAXC), 9.0, device=DEV), cls_confid=torch.full((N, MAXC), 9.0, device=DEV),
                reg_pred_std=torch.full((N, MAXC, 4), 9.0, device=DEV), fpn_levels=torch.full((N, MAXC), 9, dtype=torch.int32, device=DEV),
                valid=torch.full((N, MAXC), 9, dtype=torch.uint8, device=DEV))
    slot0 = 0
    for l, (h, w, s) in enumerate(levels):
        HW = h * w
        logits = torch.randn((N * HW, C), generator=g)
        box = torch.randn((N * HW, BS), generator=g) * 2
        flat = torch.stack([torch.randperm(HW * C, generator=g)[:K[l]] for _ in range(N)])
        rank = torch.rand((N, K[l]), generator=g)
        keys = (rank.view(torch.int32).long() << 32) | (0xFFFFFFFF - flat)
        keys[0, -2:] = -1                       # empty slots
        keys[1, 0] = -1
        H.fcos_decode_cont(dev(keys), dev(logits), dev(box), N, HW, w, s, l, 1, slot0, outs)
        o = {k: v.cpu() for k, v in outs.items()}
        for n in range(N):
            for k in range(K[l]):
                sl = slot0 + k
                if int(keys[n, k]) < 0:
                    assert int(o["valid"][n, sl]) == 0 and float(o["scores"][n, sl]) == -1.0 and torch.all(o["boxes"][n, sl] == 0)
                    continue
                f = int(flat[n, k])
                hw, c = f // C, f % C
                row = box[n * HW + hw]
                x, y = float((hw % w) * s + s // 2), float((hw // w) * s + s // 2)
                d = torch.clamp(row[:4], min=0) * s
                want = torch.tensor([x - float(d[0]), y - float(d[1]), x + float(d[2]), y + float(d[3])])
                assert torch.equal(o["boxes"][n, sl], want)
                assert int(o["classes"][n, sl]) == c and int(o["fpn_levels"][n, sl]) == l and int(o["valid"][n, sl]) == 1
                assert torch.equal(o["reg_pred_std"][n, sl], row[4:8]) and o["locations"][n, sl].tolist() == [x, y]
                assert abs(float(o["scores"][n, sl]) - math.sqrt(float(rank[n, k]))) <= 1e-6
                assert abs(float(o["centerness"][n, sl]) - float(torch.sigmoid(row[8]))) <= 1e-6
                assert abs(float(o["cls_confid"][n, sl]) - float(torch.sigmoid(logits[n * HW + hw, c]))) <= 1e-6
        slot0 += K[l]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "fcos_cont_outputs.npz")))


def T(a):
    return torch.from_numpy(np.asarray(a))


def build_head_out(gold, requires_grad=False):
    from tests.test_fcos_cont import box_rows
    from ubteacher.ops import LevelMeta
    N = int(gold["N"])
    level_hw = [tuple(gold["logits%d" % l].shape[2:]) for l in range(5)]
    meta = LevelMeta(N, level_hw)
    logits_all = torch.cat([T(gold["logits%d" % l]).permute(0, 2, 3, 1).reshape(-1, 80) for l in range(5)]).to(DEV).contiguous()
    box_all = box_rows(gold, STRIDE).to(DEV)
    if requires_grad:
        logits_all.requires_grad_(True)
        box_all.requires_grad_(True)
    return {"logits": logits_all, "box": box_all, "meta": meta}, level_hw


def cont_cfg(**fcos):
    from tests.test_fcos_cont import cont_outputs_cfg
    return cont_outputs_cfg(**fcos)


def padded_gt(gold, prefix):
    from tests.test_fcos_kernels_gpu import padded_gt as pg
    return pg(gold, prefix, int(gold["N"]))


@pytest.mark.parametrize("mode", ["test", "train"])
def test_predict_proposals_cont_vs_reference_golden(gold, mode):
    """boxes / scores with the tolerances of tests/test_fcos_kernels_gpu.py::test_decode_nms; classes, levels and the kept candidates'
    location indices exact"""
    from tests.test_fcos_kernels_gpu import close
    from ubteacher.modeling.fcos import FCOSOutputs
    over = {k[len("det_cfg_"):]: (float(v) if "TH" in k else int(v)) for k, v in gold.items() if k.startswith("det_cfg_")}
    outm = FCOSOutputs(cont_cfg(**over))
    outm.training = mode == "train"
    head_out, level_hw = build_head_out(gold)
    N, H, W = int(gold["N"]), int(gold["H"]), int(gold["W"])
    det = outm.predict_proposals(head_out, level_hw, [(H, W)] * N, "cls_n_ctr")
    for i, r in enumerate(det.to_instances()):
        p = "det_%s_%d_" % (mode, i)
        assert len(r) == len(gold[p + "classes"]) and len(r) > 0
        assert np.array_equal(r.pred_classes.cpu().numpy(), gold[p + "classes"])
        assert np.array_equal(r.fpn_levels.cpu().numpy(), gold[p + "level"])
        strides = np.array([8, 16, 32, 64, 128])[gold[p + "level"]]
        loc = r.locations.cpu().numpy()
        wl = -(-W // strides)
        hw = ((loc[:, 1] - strides // 2) / strides).round().astype(np.int64) * wl + ((loc[:, 0] - strides // 2) / strides).round().astype(np.int64)
        assert np.array_equal(hw, gold[p + "hw"])
        close(r.pred_boxes.tensor, gold[p + "boxes"], rtol=1e-5, atol=2e-4)
        close(r.scores, gold[p + "scores"], rtol=2e-5)
        close(r.centerness, gold[p + "ctr"], rtol=2e-5)
        close(r.cls_confid, gold[p + "conf"], rtol=2e-5)
        close(r.reg_pred_std, gold[p + "std"])


# ---- losses through FCOSOutputs against the executed reference -----------------------------------
def level_grads(gold, case, head_out, with_std=True, with_logits=True):
    from tests.test_fcos_kernels_gpu import close
    meta = head_out["meta"]
    for l in range(5):
        if with_logits:
            close(meta.level_view(head_out["logits"].grad, l).permute(0, 3, 1, 2), gold["%s_glogits%d" % (case, l)], rtol=1e-4, atol=2e-7)
        gb = meta.level_view(head_out["box"].grad, l)
        close(gb[..., 0:4].permute(0, 3, 1, 2), gold["%s_greg%d" % (case, l)], rtol=1e-4, atol=2e-7)
        if with_std:
            close(gb[..., 4:8].permute(0, 3, 1, 2), gold["%s_gstd%d" % (case, l)], rtol=1e-4, atol=2e-7)
        else:
            assert float(gb[..., 4:8].abs().max()) == 0.0
        close(gb[..., 8:9].permute(0, 3, 1, 2), gold["%s_gctr%d" % (case, l)], rtol=1e-4, atol=2e-7)
        assert float(gb[..., 9:].abs().max()) == 0.0


SUP_CASES = {"a_sup": dict(KL_LOSS=False, CENTER_SAMPLE=True), "b_sup": dict(),
             "c_sup": dict(KL_LOSS_TYPE="klloss", LOC_FUN_ALL="weight_ctr_mean")}


@pytest.mark.parametrize("case", sorted(SUP_CASES))
def test_supervised_losses_cont_vs_reference_golden(gold, case):
    from tests.test_fcos_kernels_gpu import close
    from ubteacher.modeling.fcos import FCOSOutputs
    outm = FCOSOutputs(cont_cfg(**SUP_CASES[case]))
    head_out, level_hw = build_head_out(gold, True)
    _, losses = outm.losses(head_out, level_hw, padded_gt(gold, "gt"))
    for k in ("loss_fcos_cls", "loss_fcos_loc", "loss_fcos_ctr"):
        close(losses[k], gold["%s_%s" % (case, k)], rtol=2e-5)
    (losses["loss_fcos_cls"] + 2.0 * losses["loss_fcos_loc"] + 3.0 * losses["loss_fcos_ctr"]).backward()
    level_grads(gold, case, head_out, with_std=case != "a_sup", with_logits=case == "a_sup")


@pytest.mark.parametrize("case,over", [("b_pseudo", dict()),
                                       ("c_pseudo", dict(KL_LOSS_TYPE="klloss", LOC_FUN_ALL="weight_ctr_mean", CONSIST_REG_LOSS="mse_loss_all_raw"))])
def test_pseudo_losses_cont_vs_reference_golden(gold, case, over):
    from tests.test_fcos_kernels_gpu import close
    from ubteacher.modeling.fcos import FCOSOutputs
    outm = FCOSOutputs(cont_cfg(**over))
    head_out, level_hw = build_head_out(gold, True)
    gt = {"cls": padded_gt(gold, "pcls_gt"), "reg": padded_gt(gold, "preg_gt")}
    _, losses = outm.pseudo_losses(head_out, level_hw, gt)
    keys = [k[len(case) + 1:] for k in gold if k.startswith(case + "_loss") or k == case + "_teacher_better_student"]
    assert "loss_fcos_loc" in keys
    for k in keys:
        close(losses[k], gold["%s_%s" % (case, k)], rtol=2e-5)
    (losses["loss_fcos_cls"] + 2.0 * losses["loss_fcos_loc"] + 3.0 * losses["loss_fcos_ctr"]).backward()
    level_grads(gold, case, head_out, with_logits=case == "b_pseudo")


def test_pseudo_regression_without_kl_loss_raises(gold):
    from ubteacher.modeling.fcos import FCOSOutputs
    outm = FCOSOutputs(cont_cfg(KL_LOSS=False))
    head_out, level_hw = build_head_out(gold)
    with pytest.raises(ValueError, match="KL_LOSS"):
        outm.pseudo_losses(head_out, level_hw, {"reg": padded_gt(gold, "preg_gt")})


def test_joint_losses_cont_equal_per_branch_paths(gold):
    """FCOSOutputs.joint_losses (one autograd node, the _acc backward kernels) against losses() + pseudo_losses() on the same head
    output, compared as tests/test_fcos_kernels_gpu.py::test_joint_losses_fused_tail_equals_op_chain compares the discrete head"""
    from tests.test_fcos_kernels_gpu import close
    from ubteacher.modeling.fcos import FCOSOutputs, PaddedBoxes
    outm = FCOSOutputs(cont_cfg())
    N = int(gold["N"])
    nl = 1

    def rows(pb, a, b):
        return PaddedBoxes(list(pb.image_sizes)[a:b], **{k: v[a:b].contiguous() for k, v in pb.f.items() if k != "count"})

    gtl = rows(padded_gt(gold, "gt"), 0, nl)
    gtu = {"cls": rows(padded_gt(gold, "pcls_gt"), nl, N), "reg": rows(padded_gt(gold, "preg_gt"), nl, N)}
    act = torch.zeros(N, dtype=torch.uint8, device=DEV)
    act[:nl] = 1
    lu, lr = 4.0, 1.5
    lw = {"loss_fcos_cls": (1.0, lu + 1.0), "loss_fcos_ctr": (1.0, lu + 1.0), "loss_fcos_loc": (1.0, lr + 1.0),
          "loss_fcos_cls_pseudo": (lu, lu + 1.0), "loss_fcos_ctr_pseudo": (lu, lu + 1.0), "loss_fcos_loc_pseudo": (lr, lr + 1.0)}
    ha, level_hw = build_head_out(gold, True)
    ls, lun, total = outm.joint_losses(ha, level_hw, gtl, gtu, nl, N, lw)
    total.backward()
    hb, _ = build_head_out(gold, True)
    _, rs = outm.losses(hb, level_hw, gtl.pad_images(0, N - nl), active=act)
    _, ru = outm.pseudo_losses(hb, level_hw, {k: v.pad_images(nl, 0) for k, v in gtu.items()}, active=(1 - act))
    ref = (rs["loss_fcos_cls"] / (lu + 1.0) + rs["loss_fcos_loc"] / (lr + 1.0) + rs["loss_fcos_ctr"] / (lu + 1.0)
           + ru["loss_fcos_cls"] * lu / (lu + 1.0) + ru["loss_fcos_ctr"] * lu / (lu + 1.0) + ru["loss_fcos_loc"] * lr / (lr + 1.0))
    ref.backward()
    for k in ("loss_fcos_cls", "loss_fcos_loc", "loss_fcos_ctr"):
        close(ls[k], rs[k].detach(), rtol=1e-6)
        close(lun[k], ru[k].detach(), rtol=1e-6)
    close(lun["teacher_better_student"], ru["teacher_better_student"], rtol=0)
    close(total.detach(), ref.detach(), rtol=1e-6)
    for key in ("logits", "box"):
        ga, gb = ha[key].grad, hb[key].grad
        assert float(gb.abs().max()) > 0
        assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())


# ---- one whole semi-supervised iteration -----------------------------------------------------------
def step_cfg(amp=False):
    from ubteacher.presets import get_config
    return get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                  "SOLVER.AMP.ENABLED", amp, "MODEL.DEVICE", "cuda", "MODEL.FCOS.REG_DISCRETE", False])


def run_golden_step(amp):
    from tests.test_fcos_cont import golden_init_state_cont
    from tests.utv2_testutil import FixedLoader, golden_batches, tune_state_for_pseudo_labels
    from ubteacher.engine import UBTeacherTrainer
    d = np.load(os.path.join(GOLD, "step_fcos_cont.npz"), allow_pickle=False)
    sd0 = golden_init_state_cont(d)
    prod, orac = golden_batches(d, "cuda")
    tr = UBTeacherTrainer(step_cfg(amp), data_loader=FixedLoader(prod))
    sd_s = tune_state_for_pseudo_labels(sd0, [x["image"] for x in orac[3]])
    sd_t = dict(sd_s)
    sd_t["proposal_generator.fcos_head.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = float(d["lr"])
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    return d, tr, rec


@pytest.fixture(scope="module")
def fp32_step():
    return run_golden_step(False)


def test_fcos_cont_step_vs_reference_trainer_golden(fp32_step):
    """One full UTv2 iteration with REG_DISCRETE False against the reference's own run_step_full_semisup (step_fcos_cont.npz), with the
    tolerances of tests/test_fcos_step_gpu.py::test_fcos_step_vs_reference_trainer_golden."""
    from tests.utv2_testutil import check_state_fingerprints, cpu_state, golden_record
    d, tr, rec = fp32_step
    for k, v in golden_record(d).items():
        if k == "data_time":
            continue
        assert k in rec, k
        print("STEP %s %.7g golden %.7g" % (k, rec[k], v))
        assert abs(rec[k] - v) <= 1e-3 * max(abs(v), 1e-6), (k, rec[k], v)
    for name, pb in zip(("pcls", "preg"), tr._last_pseudo):
        for i in range(pb.n):
            m = pb["valid"][i].bool()
            assert int(m.sum()) == len(d["%s%d_boxes" % (name, i)]), (name, i)
            order = torch.argsort(pb["scores"][i][m], descending=True, stable=True).cpu()
            ref_order = np.argsort(-d["%s%d_scores" % (name, i)], kind="stable")
            assert np.array_equal(pb["classes"][i][m].long().cpu()[order].numpy(), d["%s%d_classes" % (name, i)][ref_order])
            np.testing.assert_allclose(pb["boxes"][i][m].cpu()[order].numpy(), d["%s%d_boxes" % (name, i)][ref_order], rtol=0, atol=2e-2)
            np.testing.assert_allclose(pb["scores"][i][m].cpu()[order].numpy(), d["%s%d_scores" % (name, i)][ref_order], rtol=1e-3)
    check_state_fingerprints(d, "teacher", cpu_state(tr.model_teacher), 0.0, exact=True)
    check_state_fingerprints(d, "student", cpu_state(tr.model), 1e-4, rtol_update=5e-3)


def test_fcos_cont_fp16_amp_step_vs_own_fp32_step(fp32_step, monkeypatch):
    """fp16 AMP: every first-step loss within 1e-3 of the product's OWN fp32 step on the same inputs (the bar the README states for AMP).
    The oracle cannot judge this mode (oracle/ models only the discrete head), and the reference golden is an fp32 run."""
    from ubteacher import ops
    _, _, rec32 = fp32_step
    monkeypatch.delenv("UTV2_PRECISION", raising=False)     # SOLVER.AMP.ENABLED alone selects IEEE fp16 + the dynamic loss scale
    try:
        _, _, rec16 = run_golden_step(True)
        assert ops.PRECISION[0] == "fp16"
    finally:
        ops.set_precision("fp32")
    for k, v in rec32.items():
        if k.startswith("loss") or k == "total_loss":
            print("AMP %s fp16 %.7g fp32 %.7g" % (k, rec16[k], v))
            assert abs(rec16[k] - v) <= 1e-3 * max(abs(v), 1e-6), (k, rec16[k], v)
