"""Anchors tests/loss_tail_ref64.py on the CPU: hand-computed answers per flag bit, agreement with the ATen arithmetic of
FCOSOutputs.losses() / pseudo_losses() restated on CPU tensors, coef against central differences in fp64, the listed mutants rejected by
the comparison rules, the exclusion cap of the joint-node seeds, and the refusals of FCOSOutputs.joint_losses."""
import types

import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_tail_ref64 as T64

F32, F64 = torch.float32, torch.float64


def t64(*v):
    return torch.tensor(v, dtype=F64)


# ---- hand-computed answers ------------------------------------------------------------------------------------------------------------
def hand_inputs():
    fs, fc = t64(24.0), t64(40.0)
    S = t64(8.0, 4.0, 12.0, 6.0, 20.0, 0.0, 0.0, 0.0)
    C = t64(16.0, 2.0, 10.0, 3.0, 9.0, 0.0, 0.0, 0.0)
    R = t64(4.0, 2.0, 5.0, 7.0, 14.0, 8.0, 18.0, 0.0)
    return fs, S, fc, C, R


ONES = [1.0] * 6


def test_hand_computed_flag_bits():
    a = hand_inputs()
    # no flag: cls 24/8, loc 6/4, ctr 12/8, cls_p 40/16, ctr_p 10/16, loc_p = w * R4 / n = 0.5 * 14 / 4
    rec, coef = T64.fcos_tail(*a, None, 1.0, 0, 0.5, ONES, ONES)
    assert rec.tolist() == [3.0, 1.5, 1.5, 2.5, 0.625, 1.75, 0.0, 10.875]
    exp = [0.0] * 26
    exp[0], exp[3], exp[4], exp[9], exp[12], exp[22] = 1 / 8, 1 / 8, 1 / 4, 1 / 16, 1 / 16, 0.5 / 4
    assert coef.tolist() == exp
    # bit 1: + w * w * S4 / n = 0.25 * 20 / 8 on the supervised loc
    rec, coef = T64.fcos_tail(*a, None, 1.0, 1, 0.5, ONES, ONES)
    assert rec[1] == 1.5 + 0.625 and coef[5] == 0.25 / 8 and rec[7] == 10.875 + 0.625
    # bits 1 + 2: "klloss" divides by 4 n on both branches
    rec, coef = T64.fcos_tail(*a, None, 1.0, 3, 0.5, ONES, ONES)
    assert rec[1] == 1.5 + 0.625 / 4 and coef[5] == 0.25 / 32 and rec[5] == 1.75 / 4 and coef[22] == 0.5 / 16
    # bit 4: the pseudo centerness is value 0 with gradient 0
    rec, coef = T64.fcos_tail(*a, None, 1.0, 4, 0.5, ONES, ONES)
    assert rec[4] == 0.0 and coef[12] == 0.0 and rec[7] == 10.875 - 0.625
    # bit 8: loc_p = R6 / R5 = 18 / 8, teacher_better_student = R5
    rec, coef = T64.fcos_tail(*a, None, 1.0, 8, 0.5, ONES, ONES)
    assert rec[5] == 2.25 and rec[6] == 8.0 and coef[24] == 1 / 8 and coef[22] == 0.0
    # weights: value * mul / div
    rec, coef = T64.fcos_tail(*a, None, 1.0, 0, 0.5, [2.0] * 6, [8.0] * 6)
    assert rec[7] == 10.875 / 4 and coef[0] == 1 / 32
    # norm / world: npa = norm[0] / world = 32 / 2, den = 16 / 2; the local KL mean still divides by the local n_pos
    norm = t64(32.0, 16.0, 8.0, 1.0, 0.0, 0.0)
    rec, coef = T64.fcos_tail(*a, norm, 2.0, 1, 0.5, ONES, ONES)
    assert rec[0] == 24 / 16 and rec[1] == 6 / 8 + 0.625 and rec[3] == 40 / 4 and coef[4] == 1 / 8
    # clamps: no positive anywhere
    z = torch.zeros(8, dtype=F64)
    rec, coef = T64.fcos_tail(t64(5.0), z, t64(3.0), z, z, None, 1.0, 9, 0.5, ONES, ONES)
    assert rec.tolist() == [5.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 8.0] and coef[4] == 1.0 / T64.EPS_DEN and coef[24] == 1.0


def test_hand_computed_rcnn():
    tg = torch.tensor([3, -1, 80, 5, -1, 0, 7, 9, -2, 11], dtype=torch.int32)      # 7 sampled
    tu = torch.tensor([-1, -1], dtype=torch.int32)                                  # none: Rn clamps to 1
    wt = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 0.0]
    rec, coef, grads = T64.rcnn_tail(t64(16.0, 32.0), t64(64.0, 128.0), t64(14.0), t64(3.0), t64(21.0), t64(5.0), tg, tu, 8.0, 16.0, 0.5, 0.25,
                                     2.0, wt)
    assert rec.tolist() == [2.0, 6.0, 1.0, 1.0, 3.0, 10.0, 2.0, 2.0, 2 + 12 + 3 + 4 + 15 + 60 + 14 + 0]
    assert coef.tolist() == [1 / 7, 2 * 2 / 7, 3 * 0.5 / 8, 4 * 0.25 / 8, 5.0, 6 * 2.0, 7 * 0.5 / 16, 0.0]
    sl = T64.rcnn_node_slices(coef)
    for got, want in zip(sl, grads):
        assert torch.equal(got, want)


# ---- the ATen arithmetic of losses() / pseudo_losses(), restated ---------------------------------------------------------------------------
def product_chain(fs, S, fc, C, R, kl_type, unify, tsbetter, klw, wmul, wdiv):
    """FCOSOutputs.losses + pseudo_losses after the kernels (modeling/fcos.py), with the class's own _normalisers / _kl_mean, and the
    trainer's weighting"""
    from ubteacher.modeling.fcos import FCOSOutputs
    me = types.SimpleNamespace(kl_loss_type=kl_type, loc_fun_all="mean")
    npa, den = FCOSOutputs._normalisers(S)
    loc = S[3] / den
    w = klw
    loc = w * (w * FCOSOutputs._kl_mean(me, S, den)) + loc
    out = [fs[0] / npa, loc, S[2] / npa]
    npa, den = FCOSOutputs._normalisers(C)
    ctr = C[2] / npa
    out += [fc[0] / npa, ctr * 0 if unify else ctr]
    _, den_r = FCOSOutputs._normalisers(R)
    if tsbetter:
        out.append(R[6] / R[5].detach().clamp(min=1.0))
    else:
        out.append(klw * FCOSOutputs._kl_mean(me, R, den_r))
    total = sum(v * m / d for v, m, d in zip(out, wmul, wdiv))
    return out, total


@pytest.mark.parametrize("tsbetter", [False, True])
@pytest.mark.parametrize("unify", [False, True])
@pytest.mark.parametrize("kl_type", ["nlloss", "klloss"])
@pytest.mark.parametrize("name", ["ordinary", "npos0_all", "den_below", "r5_zero"])
def test_tail_equals_the_aten_chain(name, kl_type, unify, tsbetter):
    fs, S, fc, C, R, _ = T64.fcos_sums(name, 1.0, False)
    leaves = [t.double().requires_grad_(True) for t in (fs, S, fc, C, R)]
    klw = T64.f32(0.05)
    wmul, wdiv = [T64.f32(v) for v in T64.FCOS_WMUL], [T64.f32(v) for v in T64.FCOS_WDIV]
    out, total = product_chain(*leaves, kl_type, unify, tsbetter, klw, wmul, wdiv)
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    flags = 1 | (2 if kl_type == "klloss" else 0) | (4 if unify else 0) | (8 if tsbetter else 0)
    rec, coef = T64.fcos_tail(fs.double(), S.double(), fc.double(), C.double(), R.double(), None, 1.0, flags, klw, wmul, wdiv)
    # the chain clamps an fp64 tensor at the double 1e-6, the product an fp32 tensor at the fp32 1e-6: where that clamp decides, only to 1e-7
    tol = 1e-7 if name in ("npos0_all", "den_below") else 1e-14
    torch.testing.assert_close(rec[:6], torch.stack([v.detach() for v in out]), rtol=tol, atol=0)
    torch.testing.assert_close(rec[7], total.detach(), rtol=tol, atol=0)
    chain = torch.cat([torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)])
    torch.testing.assert_close(coef, chain, rtol=tol, atol=0)


# ---- coef against central differences ------------------------------------------------------------------------------------------------------
NORMALISERS = (1, 2, 10, 11, 18, 19, 23)     # (n_pos, sum ctr) of the three sets and R5 in the flat order of coef


@pytest.mark.parametrize("flags", range(16))
def test_fcos_coef_against_central_differences(flags):
    fs, S, fc, C, R, norm = T64.fcos_sums("ordinary", 2.0, True)
    args = [t.double() for t in (fs, S, fc, C, R)]
    rec, coef = T64.fcos_tail(*args, norm.double(), 2.0, flags, 0.05, T64.FCOS_WMUL, T64.FCOS_WDIV)
    flat = torch.cat(args)
    sizes = [1, 8, 1, 8, 8]
    for i in range(26):
        h = 1e-4 * max(1.0, abs(float(flat[i])))
        tot = []
        for sgn in (1.0, -1.0):
            f = flat.clone()
            f[i] += sgn * h
            tot.append(float(T64.fcos_tail(*torch.split(f, sizes), norm.double(), 2.0, flags, 0.05, T64.FCOS_WMUL, T64.FCOS_WDIV)[0][7]))
        fd = (tot[0] - tot[1]) / (2 * h)
        if i in NORMALISERS:
            continue      # n_pos (it feeds the KL mean's divisor), sum ctr and R5 are normalisers: no gradient by definition
        assert abs(fd - float(coef[i])) <= 1e-9 * max(1.0, abs(fd)), (i, fd, float(coef[i]))
    assert all(float(coef[i]) == 0.0 for i in NORMALISERS)


def test_rcnn_coef_against_central_differences():
    a = T64.rcnn_sums(65, 63, 5)
    consts = (512.0, 768.0, 1.21, 0.81, 1.5, T64.RCNN_WT)
    rec, coef, grads = T64.rcnn_tail(*[t.double() for t in a[:6]], a[6], a[7], *consts)
    flat = torch.cat([t.double() for t in a[:6]])
    g = torch.cat(grads)
    for i in range(8):
        tot = []
        for sgn in (1.0, -1.0):
            f = flat.clone()
            f[i] += sgn * 1e-3
            tot.append(float(T64.rcnn_tail(*torch.split(f, [2, 2, 1, 1, 1, 1]), a[6], a[7], *consts)[0][8]))
        fd = (tot[0] - tot[1]) / 2e-3
        assert abs(fd - float(g[i])) <= 1e-9 * max(1.0, abs(fd)), (i, fd, float(g[i]))


# ---- the rules: the fp32 reference passes, every mutant fails ----------------------------------------------------------------------------------
def fcos_rule(k_rec, k_coef, inputs, world, flags, klw):
    fs, S, fc, C, R, norm = inputs
    a = [t.double() for t in (fs, S, fc, C, R)]
    n64 = None if norm is None else norm.double()
    rec, coef = T64.fcos_tail(*a, n64, world, flags, klw, T64.FCOS_WMUL, T64.FCOS_WDIV)
    mrec, mcoef = T64.fcos_mag(fs, S, fc, C, R, norm, world, flags, klw, T64.FCOS_WMUL, T64.FCOS_WDIV)
    nrec, ncoef = T64.fcos_counts(flags)
    ok_r, _ = T64.tail_ok(k_rec, rec, mrec, nrec)
    ok_c, _ = T64.tail_ok(k_coef, coef, mcoef, ncoef)
    zeros = T64.is_pos_zero(k_coef.float()[T64.fcos_structural_zero(flags)])
    return ok_r and ok_c and zeros


def fcos_k(inputs, world, flags, klw, mut=None):
    """the reference itself in the kernel's place: evaluated in fp64 (a correct kernel's error is far inside the rule) and rounded to fp32"""
    fs, S, fc, C, R, norm = inputs
    rec, coef = T64.fcos_tail(*[t.double() for t in (fs, S, fc, C, R)], None if norm is None else norm.double(), world, flags, klw,
                              T64.FCOS_WMUL, T64.FCOS_WDIV, mut=mut)
    return rec.float(), coef.float()


@pytest.mark.parametrize("flags", range(16))
@pytest.mark.parametrize("name", T64.FCOS_SUM_SETS)
def test_fcos_rule_accepts_the_reference(name, flags):
    for world, with_norm in ((1.0, False), (2.0, True), (8.0, True)):
        inputs = T64.fcos_sums(name, world, with_norm)
        assert fcos_rule(*fcos_k(inputs, world, flags, 0.05), inputs, world, flags, 0.05)
        # and the fp32 evaluation of the same function: autograd spends one more rounding per coefficient than the counted kernel path
        fs, S, fc, C, R, norm = inputs
        rec32, coef32 = T64.fcos_tail(fs, S, fc, C, R, norm, world, flags, 0.05, T64.FCOS_WMUL, T64.FCOS_WDIV)
        rec, coef = T64.fcos_tail(*[t.double() for t in (fs, S, fc, C, R)], None if norm is None else norm.double(), world, flags, 0.05,
                                  T64.FCOS_WMUL, T64.FCOS_WDIV)
        mrec, mcoef = T64.fcos_mag(fs, S, fc, C, R, norm, world, flags, 0.05, T64.FCOS_WMUL, T64.FCOS_WDIV)
        nrec, ncoef = T64.fcos_counts(flags)
        assert T64.tail_ok(rec32, rec, mrec, nrec)[0]
        assert T64.tail_ok(coef32, coef, mcoef, [n + 1 if n else 0 for n in ncoef])[0]


FCOS_MUTANTS = [   # (mutant, sum set, world, with_norm, flags): a cell of the GPU grid that rejects it
    ("kl4drop", "ordinary", 1.0, False, 3),
    ("kl4drop", "ordinary", 1.0, False, 2),
    ("unifycoef", "ordinary", 1.0, False, 4),
    ("nonorm", "ordinary", 2.0, True, 0),
    ("nonorm", "ordinary", 8.0, True, 9),
    ("clamp1", "den_above", 1.0, False, 0),
    ("clamp1", "den_below", 2.0, True, 0),
    ("clamp1", "npos0_sup", 1.0, False, 1),
    ("klw1", "ordinary", 1.0, False, 1),
    ("klw1", "large", 8.0, True, 3),
]


@pytest.mark.parametrize("mut,name,world,with_norm,flags", FCOS_MUTANTS)
def test_fcos_rule_rejects_the_mutants(mut, name, world, with_norm, flags):
    inputs = T64.fcos_sums(name, world, with_norm)
    assert fcos_rule(*fcos_k(inputs, world, flags, 0.05), inputs, world, flags, 0.05)
    assert not fcos_rule(*fcos_k(inputs, world, flags, 0.05, mut=mut), inputs, world, flags, 0.05)


RCNN_CONSTS = (512.0, 768.0, 1.21, 0.81, 1.5, T64.RCNN_WT)


def rcnn_rule(k_rec, k_coef, a):
    rec, coef, _ = T64.rcnn_tail(*[t.double() for t in a[:6]], a[6], a[7], *RCNN_CONSTS)
    mrec, mcoef = T64.rcnn_mag(*a, *RCNN_CONSTS)
    return T64.tail_ok(k_rec, rec, mrec, T64.RCNN_NREC)[0] and T64.tail_ok(k_coef, coef, mcoef, T64.RCNN_NCOEF)[0]


@pytest.mark.parametrize("n", T64.RCNN_NTGT)
def test_rcnn_rule_accepts_the_reference_and_rejects_an_unclamped_count(n):
    for a in (T64.rcnn_sums(n, 1000 - n, 3 + n), T64.rcnn_sums(n, 65, 4 + n, all_empty=True)):
        rec, coef, _ = T64.rcnn_tail(*[t.double() for t in a[:6]], a[6], a[7], *RCNN_CONSTS)
        assert rcnn_rule(rec.float(), coef.float(), a)
        rec32, coef32, _ = T64.rcnn_tail(*a, *RCNN_CONSTS)
        assert rcnn_rule(rec32, coef32, a)
        if int((a[6] >= 0).sum()) == 0:
            rec, coef, _ = T64.rcnn_tail(*[t.double() for t in a[:6]], a[6], a[7], *RCNN_CONSTS, mut="rnclamp")
            assert not rcnn_rule(rec.float(), coef.float(), a)


def test_node_slice_swap_is_visible_with_distinct_weights():
    a = T64.rcnn_sums(65, 63, 5)
    rec, coef, grads = T64.rcnn_tail(*[t.double() for t in a[:6]], a[6], a[7], *RCNN_CONSTS)
    mcoef = T64.rcnn_mag(*a, *RCNN_CONSTS)[1]
    good, bad = T64.rcnn_node_slices(coef.float()), T64.rcnn_node_slices(coef.float(), mut="swap14")
    mags = T64.rcnn_node_slices(mcoef)
    assert all(T64.tail_ok(g, r, m, [3] * r.numel())[0] for g, r, m in zip(good, grads, mags))
    assert not all(T64.tail_ok(g, r, m, [3] * r.numel())[0] for g, r, m in zip(bad, grads, mags))


# ---- the joint node's reference ----------------------------------------------------------------------------------------------------------------
JOINT_CASES = [("fused", 4100), ("shared", 4200), ("empty", 4300)]


def joint_refs(layout, seed, cflags, flags_s, flags_p, cont=False, mut=None, BS=80):
    BS = 16 if cont else BS
    logits, box, sets = T64.joint_case(layout, seed, BS=BS, cont=cont)
    consts = T64.joint_consts(cflags, flags_s, flags_p, 16)
    sets64 = tuple(tuple(x for x in s) for s in sets)
    r64 = T64.fcos_joint(logits.double(), box.double(), sets64, consts, cont=cont, mut=mut)
    r32 = T64.fcos_joint(logits, box, sets, consts, cont=cont)
    return r64, r32


@pytest.mark.parametrize("head", ["BS80", "BS76", "cont"])
@pytest.mark.parametrize("layout,seed", JOINT_CASES)
def test_joint_seeds_stay_within_the_exclusion_cap(layout, seed, head):
    """the rounded fp64 reference in the kernel's place: nothing of the comparison may rest on excluded elements (cap 2 %)"""
    cont, BS = head == "cont", 76 if head == "BS76" else 80
    for cflags, fp, q in ((9, 0, 0), (3, L64.LT_KLLOSS, 0), (1, 0, L64.LT_QUALITY_IOU), (3, L64.LT_KLLOSS, L64.LT_QUALITY_IOU)):
        r64, r32 = joint_refs(layout, seed, cflags, fp | q, fp, cont=cont, BS=BS)
        assert r64["dbox"][0].shape[1] == (16 if cont else BS)
        for key, M in (("dlogits", 16), ("dbox", 4)):
            g64, s = L64.total_and_scale(r64[key])
            g32, _ = L64.total_and_scale(r32[key])
            ok, res = L64.grad_ok(g64.float(), g64, g32, s, M)
            assert ok and res["excluded"] <= 0.02, (layout, key, res)
        assert torch.isfinite(r64["rec"]).all() and torch.isfinite(r32["rec"]).all()


def test_joint_rule_rejects_an_overwriting_third_backward():
    r64, r32 = joint_refs("shared", 4200, 9, 0, 0)
    bad, _ = joint_refs("shared", 4200, 9, 0, 0, mut="noacc3")
    g64, s = L64.total_and_scale(r64["dbox"])
    g32, _ = L64.total_and_scale(r32["dbox"])
    gbad, _ = L64.total_and_scale(bad["dbox"])
    assert L64.grad_ok(g64.float(), g64, g32, s, 4)[0]
    assert not L64.grad_ok(gbad.float(), g64, g32, s, 4)[0]


# ---- the pack kernels' references ------------------------------------------------------------------------------------------------------------
def test_pack_reference_mutants_differ():
    kidx = torch.tensor([[2, 0, -1, -1], [1, 3, 0, 2]], dtype=torch.int32)
    cnt = torch.tensor([2, 4], dtype=torch.int32)
    boxes = torch.arange(2 * 4 * 4, dtype=F32).reshape(2, 4, 4)
    scores = torch.arange(8, dtype=F32).reshape(2, 4)
    ob, osc, ov = T64.nms_pack(kidx, cnt, boxes, scores)
    assert ov.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1]] and osc.tolist() == [[2.0, 0.0, 0.0, 0.0], [5.0, 7.0, 4.0, 6.0]]
    assert torch.equal(ob[0, 2], boxes[0, 0])
    assert not torch.equal(T64.nms_pack(kidx, cnt, boxes, scores, mut="cntle")[2], ov)
    K, P = 3, 4
    pb = torch.arange(2 * P * K * 4, dtype=F32).reshape(2, P, K, 4)
    flat = torch.tensor([[5, 0, 11], [7, 2, 3]])
    sc = torch.tensor([[0.9, 0.5, 0.25], [0.8, 0.5, -1.0]])
    s, rows, cls, cb, valid = T64.roi_infer_gather(flat, sc, pb, K, 0.5)
    assert rows.tolist() == [[1, 0, 3], [2, 0, 1]] and cls.tolist() == [[2, 0, 2], [1, 2, 0]] and valid.tolist() == [[1, 0, 0], [1, 0, 0]]
    assert torch.equal(cb[0, 0], pb[0, 1, 2])
    assert not torch.equal(T64.roi_infer_gather(flat, sc, pb, K, 0.5, mut="box0")[3], cb)


# ---- FCOSOutputs.joint_losses refuses what its scalar tail cannot represent ---------------------------------------------------------------------
def outputs(*opts):
    from ubteacher.modeling.fcos import FCOSOutputs
    from ubteacher.presets import get_config
    return FCOSOutputs(get_config("fcos", 1, ["MODEL.DEVICE", "cpu"] + list(opts)))


def test_joint_losses_refuses_kl_loss_off():
    fo = outputs("MODEL.FCOS.KL_LOSS", False)
    with pytest.raises(ValueError, match="pseudo regression loss needs MODEL.FCOS.KL_LOSS"):
        fo.joint_losses(None, None, None, None, 1, 2, None)


@pytest.mark.parametrize("fun", ["sum", "weight_ctr_sum", "weight_ctr_mean"])
def test_joint_losses_refuses_klloss_reductions_it_cannot_represent(fun):
    fo = outputs("MODEL.FCOS.KL_LOSS_TYPE", "klloss", "MODEL.FCOS.LOC_FUN_ALL", fun)
    with pytest.raises(ValueError, match="LOC_FUN_ALL"):
        fo.joint_losses(None, None, None, None, 1, 2, None)


@pytest.mark.parametrize("opts,fused", [((), True), (("MODEL.FCOS.KL_LOSS", False), False),
                                        (("MODEL.FCOS.KL_LOSS_TYPE", "klloss", "MODEL.FCOS.LOC_FUN_ALL", "sum"), False),
                                        (("MODEL.FCOS.KL_LOSS_TYPE", "klloss", "MODEL.FCOS.LOC_FUN_ALL", "mean"), True)])
def test_forward_joint_finish_still_takes_the_fallback(opts, fused, monkeypatch):
    from ubteacher.modeling.fcos import FCOS
    fo = outputs(*opts)
    calls = []
    monkeypatch.setattr(fo, "joint_losses", lambda *a, **k: (calls.append("joint"), ({}, {}, torch.zeros(())))[1])
    monkeypatch.setattr(fo, "losses", lambda *a, **k: (calls.append("losses"), (None, {"loss_fcos_cls": 0}))[1])
    monkeypatch.setattr(fo, "pseudo_losses", lambda *a, **k: (calls.append("pseudo"), (None, {"loss_fcos_cls": 0}))[1])
    model = FCOS.__new__(FCOS)
    model.fcos_outputs = fo

    class Gt:
        def __init__(self, n):
            self.n = n

        def pad_images(self, a, b):
            return Gt(self.n + a + b)

    ctx = dict(head_out=None, level_hw=None, n_labeled=2, N=4, gt_labeled=Gt(2), device="cpu")
    weights = {k: (1.0, 1.0) for k in fo.LOSS_KEYS}
    l_sup, l_uns = model.forward_joint_finish(ctx, {"cls": Gt(2), "reg": Gt(2)}, weights)
    assert calls == (["joint"] if fused else ["losses", "pseudo"])
    assert ("weighted_total" in l_sup) == fused
