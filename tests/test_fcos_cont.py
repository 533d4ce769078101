"""CPU side of the continuous FCOS regression head (MODEL.FCOS.REG_DISCRETE False): the model builds with the reference's state-dict
surface, checkpoints round-trip and a mode mismatch is reported, the fp64 reference of the kernels (tests/loss_ref64_cont.py) agrees
with the executed-reference golden (tests/golden/fcos_cont_outputs.npz), its grids stay inside the exclusion cap, and the new entry
points refuse bad arguments before anything is launched (the libraries load without a GPU).  Helpers of tests/test_fcos_cont_gpu.py
live here too, so the two modules cannot drift."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_cont as C64
from tests.test_loss_ref64 import _excluded_ok, near

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64 = torch.float64


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "fcos_cont_outputs.npz")))


def cpu_cfg(*extra):
    from ubteacher.presets import get_config
    return get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                  "SOLVER.AMP.ENABLED", False, "MODEL.DEVICE", "cpu"] + list(extra))


def cont_outputs_cfg(**over):
    """the configuration of tests/golden/gen_golden_fcos_cont.py::cont_cfg as a product config"""
    from ubteacher import add_ubteacher_config
    from ubteacher.d2 import get_cfg
    cfg = get_cfg()
    add_ubteacher_config(cfg)
    f = cfg.MODEL.FCOS
    f.CENTER_SAMPLE = False; f.REG_DISCRETE = False; f.KL_LOSS = True; f.KLLOSS_WEIGHT = 0.05; f.KL_LOSS_TYPE = "nlloss"
    cfg.SEMISUPNET.CONSIST_REG_LOSS = "ts_locvar_better_nms_nll_l1"
    for k, v in over.items():
        setattr(cfg.SEMISUPNET if k == "CONSIST_REG_LOSS" else f, k, v)
    return cfg


def box_rows(gold, BS):
    """golden NCHW head tensors -> the level-first continuous box rows [P, BS]: ltrb (pre-ReLU) | std | ctr | pad"""
    rows = []
    for l in range(5):
        n = T(gold["reg%d" % l]).permute(0, 2, 3, 1).reshape(-1, 4).shape[0]
        b = torch.zeros((n, BS))
        b[:, 0:4] = T(gold["reg%d" % l]).permute(0, 2, 3, 1).reshape(-1, 4)
        b[:, 4:8] = T(gold["std%d" % l]).permute(0, 2, 3, 1).reshape(-1, 4)
        b[:, 8] = T(gold["ctr%d" % l]).permute(0, 2, 3, 1).reshape(-1)
        rows.append(b)
    return torch.cat(rows).contiguous()


def level_first(gold, fmt, ch):
    return torch.cat([T(gold[fmt % l]).reshape(-1, ch) if ch else T(gold[fmt % l]).reshape(-1) for l in range(5)])


def grads_level_first(gold, case, BS, with_std=True):
    g = []
    for l in range(5):
        r = T(gold["%s_greg%d" % (case, l)]).permute(0, 2, 3, 1).reshape(-1, 4)
        b = torch.zeros((r.shape[0], BS))
        b[:, 0:4] = r
        if with_std:
            b[:, 4:8] = T(gold["%s_gstd%d" % (case, l)]).permute(0, 2, 3, 1).reshape(-1, 4)
        b[:, 8] = T(gold["%s_gctr%d" % (case, l)]).permute(0, 2, 3, 1).reshape(-1)
        g.append(b)
    return torch.cat(g)


def golden_init_state_cont(d):
    """the initial weights step_fcos_cont.npz started from (tests/utv2_testutil.golden_init_state under REG_DISCRETE False)"""
    from tests.utv2_testutil import state_fingerprint
    from ubteacher.modeling import build_model
    torch.manual_seed(int(d["seed_state"]))
    model = build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", False))
    sd = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items()}
    keys = [str(k) for k in d["init_keys"]]
    assert keys == [k for k in sd if sd[k].dtype.is_floating_point], "state-dict surface differs from the golden's"
    assert np.array_equal(np.stack([state_fingerprint(sd[k]) for k in keys]), d["init_fp"]), "CPU initialisation is not the golden's"
    return sd


# ---- model surface ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kl", [True, False])
def test_build_model_cont_state_dict_is_the_references(gold, kl):
    from ubteacher.modeling import build_model
    model = build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", False, "MODEL.FCOS.KL_LOSS", kl))
    sd = model.state_dict()
    tag = "kl" if kl else "nokl"
    want = {str(k): tuple(int(x) for x in s if x >= 0) for k, s in zip(gold["keys_" + tag], gold["shapes_" + tag])}
    mine = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("proposal_generator.")}
    assert mine == want
    assert tuple(sd["proposal_generator.fcos_head.bbox_pred.weight"].shape) == (4, 256, 3, 3)
    assert ("proposal_generator.fcos_head.bbox_pred_std.weight" in sd) == kl
    assert "proposal_generator.fcos_outputs.integral.project" in sd      # the reference builds Integral whatever REG_DISCRETE says


def test_cont_checkpoint_round_trip_and_mode_mismatch(tmp_path):
    from ubteacher.modeling import build_model
    torch.manual_seed(3)
    a = build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", False))
    path = str(tmp_path / "cont.pth")
    torch.save({"model": a.state_dict()}, path)
    torch.manual_seed(4)
    b = build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", False))
    b.load_state_dict(torch.load(path)["model"])
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    disc = build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", True))
    with pytest.raises(Exception, match="bbox_pred"):
        disc.load_state_dict(torch.load(path)["model"])
    with pytest.raises(Exception, match="bbox_pred"):
        b.load_state_dict(disc.state_dict())


def test_discrete_default_config_still_builds_with_the_same_keys():
    """regression guard: the shipped recipe (REG_DISCRETE True) keeps its state-dict surface"""
    from ubteacher.modeling import build_model
    sd = build_model(cpu_cfg()).state_dict()
    assert tuple(sd["proposal_generator.fcos_head.bbox_pred.weight"].shape) == (68, 256, 3, 3)
    assert tuple(sd["proposal_generator.fcos_head.bbox_pred_std.weight"].shape) == (4, 256, 3, 3)
    d = np.load(os.path.join(GOLD, "step_fcos.npz"), allow_pickle=False)
    assert [str(k) for k in d["init_keys"]] == [k for k in sd if sd[k].dtype.is_floating_point]
    from ubteacher.modeling.fcos import FCOSHead  # noqa: F401
    with pytest.raises(AssertionError):
        build_model(cpu_cfg("MODEL.FCOS.REG_DISCRETE", True, "MODEL.FCOS.REG_MAX", 8))


# ---- the fp64 reference against the executed reference ------------------------------------------------
def _ref_losses(gold, labels_fmt, regt_fmt, flags, bvars_fmt=None, tsb=0.1, tsc=0.8):
    box = box_rows(gold, 16).double()
    lab = level_first(gold, labels_fmt, 0).to(torch.int32)
    t = level_first(gold, regt_fmt, 4).float()
    bv = level_first(gold, bvars_fmt, 4).float() if bvars_fmt else None
    return box, lab, t, bv


def test_ref64_cont_agrees_with_executed_reference_supervised(gold):
    """case b (nlloss) and c (klloss + weight_ctr_mean): loss_fcos_loc / loss_fcos_ctr and d total / d (reg, std, ctr) of the golden
    (total = cls + 2 loc + 3 ctr) from the fp64 terms, normalised as fcos_outputs.py:317-321,361-416 does"""
    for case, flags, kl4 in (("b_sup", 0, False), ("c_sup", L64.LT_KLLOSS | L64.LT_KL_WCTR, True), ("a_sup", 0, None)):
        box, lab, t, _ = _ref_losses(gold, case.replace("c_", "b_") + "_labels%d", case.replace("c_", "b_") + "_regt%d", flags)
        terms, _, _ = C64.loc_terms_cont(box, t, None, lab, flags, 0.0, 0.0)
        S = terms.sum(dim=0)
        npos, den = max(float(S[0]), 1.0), max(float(S[1]), 1e-6)
        w = 0.05
        if kl4 is None:
            c_nll = 0.0
            loc = S[3] / den
        elif kl4:
            c_nll = 2.0 * w * w / den            # weight_ctr_mean: the KL sum over the loss normaliser
            loc = w * w * S[4] / den + S[3] / den
        else:
            c_nll = 2.0 * w * w / npos
            loc = w * w * S[4] / npos + S[3] / den
        near(loc, gold[case + "_loss_fcos_loc"], k=256)
        near(S[2] / npos, gold[case + "_loss_fcos_ctr"], k=256)
        _, parts, _ = C64.loc_terms_cont(box, t, None, lab, flags, 0.0, 0.0, coef=(3.0 / npos, 2.0 / den, c_nll, 0.0))
        g, _ = L64.total_and_scale(parts)
        want = grads_level_first(gold, case, 16, with_std=kl4 is not None)
        assert float((g - want.double()).abs().max()) <= 1e-4 * float(want.abs().max())


def test_ref64_cont_agrees_with_executed_reference_pseudo(gold):
    """case b pseudo: the teacher-better L1 on the reg set (TS_BETTER 0.1, TS_BETTER_CERT 0.8) + centerness BCE on the cls set"""
    box, lab_c, t_c, _ = _ref_losses(gold, "b_pcls_labels%d", "b_pcls_regt%d", 0)
    _, lab_r, t_r, bv = _ref_losses(gold, "b_preg_labels%d", "b_preg_regt%d", 0, "b_preg_bvars%d")
    tc, _, _ = C64.loc_terms_cont(box, t_c, None, lab_c, 0, 0.0, 0.0)
    trm, _, info = C64.loc_terms_cont(box, t_r, bv, lab_r, 0, 0.1, 0.8)
    Sc, Sr = tc.sum(dim=0), trm.sum(dim=0)
    npc, nsel = max(float(Sc[0]), 1.0), max(float(Sr[5]), 1.0)
    assert float(Sr[5]) == float(gold["b_pseudo_teacher_better_student"]) and float(Sr[5]) > 0
    near(Sr[6] / nsel, gold["b_pseudo_loss_fcos_loc"], k=256)
    near(Sc[2] / npc, gold["b_pseudo_loss_fcos_ctr"], k=256)
    _, pc, _ = C64.loc_terms_cont(box, t_c, None, lab_c, 0, 0.0, 0.0, coef=(3.0 / npc, 0.0, 0.0, 0.0))
    _, pr, _ = C64.loc_terms_cont(box, t_r, bv, lab_r, 0, 0.1, 0.8, coef=(0.0, 0.0, 0.0, 2.0 / nsel))
    g = L64.total_and_scale(pc)[0] + L64.total_and_scale(pr)[0]
    want = grads_level_first(gold, "b_pseudo", 16)
    assert float((g - want.double()).abs().max()) <= 1e-4 * float(want.abs().max())


def test_cont_grids_branch_alike_and_stay_under_the_cap():
    from tests import test_fcos_cont_gpu as G
    cases = [(G.flag_grid(f, bv), f) for f in L64.LEGAL_FLAGS for bv in (False, True)]
    cases += [(G.shape_grid(P, BS), f) for P in G.CONT_P if P > 0 for BS in G.CONT_BS for f in G.SHAPE_FLAGS]
    cases += [(C64.cont_case(48, 16, s, labels_mode="positive"), f) for s in (11, 12, 13, 14, 15, 17) for f in (0, 4, 8, L64.LT_KLLOSS)]
    for case, flags in cases:
        t64, p64, i64 = C64.loc_terms_cont(case[0].double(), *case[1:], flags, C64.TS_BETTER, C64.TS_CERT)
        _, p32, i32 = C64.loc_terms_cont(*case, flags, C64.TS_BETTER, C64.TS_CERT)
        assert _excluded_ok(p64, p32) and bool(torch.isfinite(t64).all())
        assert torch.equal(i64["sign"], i32["sign"].double()) and torch.equal(i64["sel"], i32["sel"])
        # nothing of the reference alone is excluded: no element where fp64 autograd cancels to 0 with a non-zero addend structure
        a, s = L64.total_and_scale(p64)
        assert bool(torch.isfinite(a).all())
    box, t, bv, lab, tsb, tsc = C64.better_tie_case()
    _, _, i64 = C64.loc_terms_cont(box.double(), t, bv, lab, 0, tsb, tsc)
    _, _, i32 = C64.loc_terms_cont(box, t, bv, lab, 0, tsb, tsc)
    assert torch.equal(i64["sel"], i32["sel"]) and i64["sel"].sum(dim=1).tolist() == [0, 4, 0, 0, 4, 0]


# ---- argument checks: refused on the host, nothing launched -------------------------------------------
def bad_argument_rows(ptr):
    """(entry point, argument tuple) rows that must return UTV2_EARG; `ptr` is any non-null address (never followed)"""
    p, z = ctypes.c_void_p(ptr), ctypes.c_void_p(0)
    st = ctypes.c_void_p(0)

    def fwd(labels=p, box=p, bs=16, t=p, P=5, flags=0, sums=p, ws=p):
        return ("utv2_fcos_loc_terms_cont_fwd", (labels, box, bs, t, z, P, 80, 0.1, 0.5, flags, sums, ws, st))

    def bwd(labels=p, box=p, bs=16, t=p, P=5, flags=0, coef=p, dbox=p):
        return ("utv2_fcos_loc_terms_cont_bwd", (labels, box, bs, t, z, P, 80, 0.1, 0.5, flags, coef, dbox, st))

    def acc(labels=p, box=p, bs=16, t=p, P=5, flags=0, coef=p, dbox=p):
        return ("utv2_fcos_loc_terms_cont_bwd_acc", (labels, box, bs, t, z, P, 80, 0.1, 0.5, flags, coef, z, dbox, 1, st))

    def dec(keys=p, K=4, logits=p, box=p, bs=16, N=2, HW=12, Wl=4, C=80, stride=8, method=1, MAXC=8, slot0=4, out=p, valid=p):
        return ("utv2_fcos_decode_cont", (keys, K, logits, box, bs, N, HW, Wl, C, stride, 0, method, MAXC, slot0, out, out, out, out, out, out,
                                          out, out, valid, st))
    rows = []
    for f in (fwd, bwd, acc):
        rows += [f(labels=z), f(box=z), f(t=z), f(P=-1), f(bs=8), f(bs=18), f(bs=0), f(flags=-1), f(flags=32), f(flags=12), f(flags=13)]
    rows += [fwd(sums=z), fwd(ws=z), bwd(coef=z), bwd(dbox=z), acc(coef=z), acc(dbox=z)]
    rows += [dec(keys=z), dec(logits=z), dec(box=z), dec(out=z), dec(valid=z), dec(bs=8), dec(bs=18), dec(K=-1), dec(slot0=5), dec(slot0=-1),
             dec(K=9, slot0=0), dec(N=0), dec(HW=0), dec(Wl=0), dec(C=0), dec(stride=0), dec(method=4), dec(method=-1)]
    return rows


def test_cont_entries_refuse_bad_arguments_without_a_device():
    from ubteacher import hip as H
    for kind in ("bf16", "fp16"):
        lib = H.load(kind)
        buf = (ctypes.c_float * 16)()
        for name, args in bad_argument_rows(ctypes.addressof(buf)):
            assert getattr(lib, name)(*args) == -1000, (kind, name, args)
