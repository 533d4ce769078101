"""The fused loss tails on the device against the fp64 references of tests/loss_tail_ref64.py: the two combine kernels
(fcos_loss_combine_kernel, rcnn_loss_combine_kernel) called directly through ubteacher.hip, and the three autograd nodes that wrap them
(ops._FcosCombineFn, ops._FcosJointLossFn, ops._RcnnCombineFn).

Rule for every rec / coef entry: |k - r64| <= n 2^-24 sum |addends|, n = the fp32 roundings on the entry's path.  The counts
(loss_tail_ref64.fcos_counts, RCNN_NREC / RCNN_NCOEF carry the derivations; fp32 division is correctly rounded in this build):
  FCOS  sum / normaliser 2; supervised loc with KL 4; TS-better loc 1, KL pseudo loc 2; total 11; coef 3 (coef[5] 4, coef[24] 2)
  RCNN  loss_cls 1, weighted losses 2, total 10, coef 2
Every test prints the worst |k - r64| / (n u sum |addends|) of its family (<= 1 passes); DESIGN.md section 13 records them.
On a dyadic grid every operation is exact and the kernels must equal r64 bit for bit; entries the flags do not use are +0 as bits.

The joint node adds the kernels' own forward-sum bounds (test_loss_kernels_fp64_gpu.py) to the tail's; its gradients go through
loss_ref64.grad_ok with M_FOCAL / M_LOC unchanged."""
import ctypes

import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_tail_ref64 as T64
from tests.test_loss_kernels_fp64_gpu import D_BLOCK, EARG, M_FOCAL, M_LOC, dev, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
KLW = 0.05
WORLDS = ((1.0, False), (2.0, True), (8.0, True))


def hip():
    from ubteacher import hip as H
    return H


def ops():
    from ubteacher import ops as O
    return O


def d64(ts):
    return [t.double() for t in ts]


def rule(tag, k, r64, mag, n):
    ok, ratio = T64.tail_ok(k.cpu(), r64, mag, n)
    assert ok, (tag, ratio, k.cpu().tolist(), r64.tolist())
    return ratio


# =================================================================================================
# fcos_loss_combine_kernel, called directly
# =================================================================================================
def fcos_run(inputs, world, flags, klw=KLW, wmul=T64.FCOS_WMUL, wdiv=T64.FCOS_WDIV):
    fs, S, fc, C, R, norm = inputs
    rec, coef = hip().fcos_loss_combine(dev(fs), dev(S), dev(fc), dev(C), dev(R), dev(norm), world, flags, klw, wmul, wdiv)
    return rec.cpu(), coef.cpu()


def fcos_refs(inputs, world, flags, klw=KLW, wmul=T64.FCOS_WMUL, wdiv=T64.FCOS_WDIV):
    fs, S, fc, C, R, norm = inputs
    n64 = None if norm is None else norm.double()
    rec, coef = T64.fcos_tail(*d64((fs, S, fc, C, R)), n64, world, flags, klw, wmul, wdiv)
    mrec, mcoef = T64.fcos_mag(fs, S, fc, C, R, norm, world, flags, klw, wmul, wdiv)
    return rec, coef, mrec, mcoef


def structural_zeros(tag, rec, coef, flags):
    assert T64.is_pos_zero(coef[T64.fcos_structural_zero(flags)]), (tag, coef.tolist())
    if not flags & 8:
        assert T64.is_pos_zero(rec[6:7]), (tag, rec.tolist())


@pytest.mark.parametrize("name", T64.FCOS_SUM_SETS)
def test_fcos_combine_grid_vs_fp64(name):
    worst_rec, worst_coef = 0.0, 0.0
    for world, with_norm in WORLDS:
        inputs = T64.fcos_sums(name, world, with_norm)
        for flags in range(16):
            tag = "fcos tail %s world %g flags %d" % (name, world, flags)
            rec, coef = fcos_run(inputs, world, flags)
            r_rec, r_coef, mrec, mcoef = fcos_refs(inputs, world, flags)
            nrec, ncoef = T64.fcos_counts(flags)
            worst_rec = max(worst_rec, rule(tag + " rec", rec, r_rec, mrec, nrec))
            worst_coef = max(worst_coef, rule(tag + " coef", coef, r_coef, mcoef, ncoef))
            structural_zeros(tag, rec, coef, flags)
    print("RATIO fcos tail %s rec %.3f coef %.3f" % (name, worst_rec, worst_coef))


@pytest.mark.parametrize("world", [1.0, 2.0, 8.0])
def test_fcos_combine_dyadic_grid_is_bit_exact(world):
    fs, S, fc, C, R, wmul, wdiv, klw = T64.fcos_dyadic(world)
    for with_norm in (False, True):
        norm = torch.cat((S[0:2], C[0:2], R[0:2])) if with_norm else None
        S2, C2 = S.clone(), C.clone()
        if with_norm:                      # the local pair is another (dyadic) number; n_pos stays: it feeds the local KL mean
            S2[1], C2[1] = 64.0, 32.0
        for flags in range(16):
            inputs = (fs, S2, fc, C2, R, norm)
            rec, coef = fcos_run(inputs, world, flags, klw, wmul, wdiv)
            r_rec, r_coef, _, _ = fcos_refs(inputs, world, flags, klw, wmul, wdiv)
            assert same_bits(rec, r_rec.float()), (world, with_norm, flags, rec.tolist(), r_rec.tolist())
            assert same_bits(coef, r_coef.float()), (world, with_norm, flags, coef.tolist(), r_coef.tolist())
            structural_zeros("dyadic", rec, coef, flags)


def test_fcos_combine_refuses_bad_arguments():
    H = hip()
    fs, S, fc, C, R, _ = T64.fcos_sums("ordinary", 1.0, False)
    t = [dev(x) for x in (fs, S, fc, C, R)]
    rec, coef = torch.zeros(8, device=DEV), torch.zeros(26, device=DEV)
    wm = (ctypes.c_float * 6)(*T64.FCOS_WMUL)
    wd = (ctypes.c_float * 6)(*T64.FCOS_WDIV)
    good = [x.data_ptr() for x in t] + [None, 1.0, 0, KLW, ctypes.cast(wm, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p), rec.data_ptr(),
                                        coef.data_ptr(), H._stream()]
    H.call("utv2_fcos_loss_combine", *good)
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12):              # every required pointer (norm, index 5, is optional)
        bad = list(good)
        bad[i] = None
        with pytest.raises(RuntimeError, match=EARG):
            H.call("utv2_fcos_loss_combine", *bad)
    for world in (0.0, 0.5, -1.0, float("nan")):
        bad = list(good)
        bad[6] = world
        with pytest.raises(RuntimeError, match=EARG):
            H.call("utv2_fcos_loss_combine", *bad)


# =================================================================================================
# rcnn_loss_combine_kernel, called directly
# =================================================================================================
RCNN_CONSTS = (512.0, 768.0, 1.21, 0.81, 1.5, T64.RCNN_WT)


def rcnn_check(tag, a, consts=RCNN_CONSTS):
    rec, coef = hip().rcnn_loss_combine(*[dev(x) for x in a], *consts)
    r_rec, r_coef, _ = T64.rcnn_tail(*d64(a[:6]), a[6], a[7], *consts)
    mrec, mcoef = T64.rcnn_mag(*a, *consts)
    w = (rule(tag + " rec", rec, r_rec, mrec, T64.RCNN_NREC), rule(tag + " coef", coef, r_coef, mcoef, T64.RCNN_NCOEF))
    zero = [k for k in range(8) if consts[5][k] == 0]
    assert T64.is_pos_zero(coef.cpu()[zero]), (tag, coef.tolist())
    return w


@pytest.mark.parametrize("n", T64.RCNN_NTGT)
def test_rcnn_combine_grid_vs_fp64(n):
    w1 = rcnn_check("rcnn tail n %d" % n, T64.rcnn_sums(n, 1000 - n, 3 + n))
    w2 = rcnn_check("rcnn tail n %d swapped" % n, T64.rcnn_sums(1000 - n, n, 5 + n))
    w3 = rcnn_check("rcnn tail n %d all empty" % n, T64.rcnn_sums(n, 65, 4 + n, all_empty=True))      # Rn clamps to 1
    print("RATIO rcnn tail n %d rec %.3f coef %.3f" % (n, max(w1[0], w2[0], w3[0]), max(w1[1], w2[1], w3[1])))


def test_rcnn_combine_dyadic_grid_is_bit_exact():
    tg = torch.arange(64, dtype=torch.int32)
    tu = torch.cat((torch.arange(16, dtype=torch.int32), torch.full((48,), -1, dtype=torch.int32)))
    a = (torch.tensor([24.0, 40.0]), torch.tensor([12.0, 6.0]), torch.tensor([96.0]), torch.tensor([20.0]), torch.tensor([48.0]),
         torch.tensor([10.0]), tg, tu)
    consts = (512.0, 256.0, 0.25, 4.0, 2.0, [1.0, 2.0, 0.5, 4.0, 8.0, 0.25, 2.0, 0.0])
    rec, coef = hip().rcnn_loss_combine(*[dev(x) for x in a], *consts)
    r_rec, r_coef, _ = T64.rcnn_tail(*d64(a[:6]), tg, tu, *consts)
    assert same_bits(rec, r_rec.float()) and same_bits(coef, r_coef.float()), (rec.tolist(), r_rec.tolist(), coef.tolist(), r_coef.tolist())


def test_rcnn_combine_refuses_bad_arguments():
    H = hip()
    a = [dev(x) for x in T64.rcnn_sums(65, 63, 5)]
    for norm in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match=EARG):
            H.rcnn_loss_combine(*a, norm, 768.0, 1.21, 0.81, 1.5, T64.RCNN_WT)
        with pytest.raises(RuntimeError, match=EARG):
            H.rcnn_loss_combine(*a, 512.0, norm, 1.21, 0.81, 1.5, T64.RCNN_WT)
    rec, coef = torch.zeros(9, device=DEV), torch.zeros(8, device=DEV)
    wt = (ctypes.c_float * 8)(*T64.RCNN_WT)
    p = [x.data_ptr() for x in a]
    good = p[:6] + [p[6], 65, p[7], 63, 512.0, 768.0, 1.21, 0.81, 1.5, ctypes.cast(wt, ctypes.c_void_p), rec.data_ptr(), coef.data_ptr(),
                    H._stream()]
    H.call("utv2_rcnn_loss_combine", *good)
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 15, 16, 17):        # every required pointer; a target list of length > 0 needs its storage
        bad = list(good)
        bad[i] = None
        with pytest.raises(RuntimeError, match=EARG):
            H.call("utv2_rcnn_loss_combine", *bad)


# =================================================================================================
# the combine nodes: every returned slice against the fp64 autograd gradient of the matching leaf
# =================================================================================================
def backward(total, leaves, g):
    return torch.autograd.grad(total, leaves, grad_outputs=torch.tensor(g, dtype=F32, device=DEV), retain_graph=True, allow_unused=True)


@pytest.mark.parametrize("flags", [0, 3, 5, 9, 15])
def test_fcos_combine_node_backward(flags):
    world, with_norm = 2.0, True
    inputs = T64.fcos_sums("ordinary", world, with_norm)
    leaves = [dev(x).requires_grad_(True) for x in inputs[:5]]
    total, rec = ops().fcos_loss_combine(*leaves, dev(inputs[5]), world, flags, KLW, T64.FCOS_WMUL, T64.FCOS_WDIV)
    r_rec, r_coef, mrec, mcoef = fcos_refs(inputs, world, flags)
    nrec, ncoef = T64.fcos_counts(flags)
    rule("fcos node rec", rec, r_rec, mrec, nrec)
    assert same_bits(total, rec[7]) and not rec.requires_grad
    g1, g1024, g0 = (backward(total, leaves, g) for g in (1.0, 1024.0, 0.0))
    sizes = [1, 8, 1, 8, 8]
    worst = 0.0
    for got, want, mag, n in zip(g1, torch.split(r_coef, sizes), torch.split(mcoef, sizes), torch.split(torch.tensor(ncoef), sizes)):
        assert got.shape == want.shape
        worst = max(worst, rule("fcos node slice", got, want, mag, n.tolist()))      # x 1 is exact: the counted n holds
    for a, b, z in zip(g1, g1024, g0):
        assert same_bits(b, a * 1024.0) and T64.is_pos_zero(z.abs())
    print("RATIO fcos node flags %d %.3f" % (flags, worst))


def test_rcnn_combine_node_backward():
    a = T64.rcnn_sums(65, 63, 5)
    leaves = [dev(x).requires_grad_(True) for x in a[:6]]
    total, rec = ops().rcnn_loss_combine(*leaves, dev(a[6]), dev(a[7]), RCNN_CONSTS)
    r_rec, r_coef, grads = T64.rcnn_tail(*d64(a[:6]), a[6], a[7], *RCNN_CONSTS)
    mrec, mcoef = T64.rcnn_mag(*a, *RCNN_CONSTS)
    rule("rcnn node rec", rec, r_rec, mrec, T64.RCNN_NREC)
    assert same_bits(total, rec[8]) and not rec.requires_grad
    g1, g1024, g0 = (backward(total, leaves, g) for g in (1.0, 1024.0, 0.0))
    worst = 0.0
    for got, want, mag in zip(g1, grads, T64.rcnn_node_slices(mcoef)):      # the eight distinct weights make any swap of slices visible
        assert got.shape == want.shape
        worst = max(worst, rule("rcnn node slice", got, want, mag, [2] * want.numel()))
    for x, y, z in zip(g1, g1024, g0):
        assert same_bits(y, x * 1024.0) and T64.is_pos_zero(z.abs())
    print("RATIO rcnn node %.3f" % worst)


# =================================================================================================
# ops.fcos_joint_loss on synthetic target sets
# =================================================================================================
def joint_refs(layout, seed, consts, cont, BS=80):
    """BS: the row pitch of the box output - 80 and 76 (7 and 3 pad columns) for the discrete head, 16 for the continuous one"""
    logits, box, sets = T64.joint_case(layout, seed, BS=16 if cont else BS, cont=cont)
    r64 = T64.fcos_joint(logits.double(), box.double(), sets, consts, cont=cont)
    r32 = T64.fcos_joint(logits, box, sets, consts, cont=cont)
    return logits, box, sets, r64, r32


def dev_sets(sets):
    (ls, rs), (lc, rc), (lr, rr, bv) = sets
    return ((dev(ls), dev(rs)), (dev(lc), dev(rc)), (dev(lr), dev(rr), dev(bv)))


def rec_bound(r64, consts):
    """n u sum |addends| of the tail + the forward-sum bounds of the kernels that feed it, pushed through the tail: every rec entry is
    monotone in every sum (rising; falling in the loss normaliser S1), so the tail at sums + e (S1 - e) bounds what the sum errors can
    move.  focal: L = 4 ceil(P C / 2^20) = 4, loc: L = 1, D = D_BLOCK (test_loss_kernels_fp64_gpu.py); counts (columns 0, 5) are exact."""
    cflags, klw, wmul, wdiv = consts[9], consts[10], consts[11], consts[12]
    assert consts[8] == 1.0      # the node is run in a world of 1 with no `norm`: the tail below is evaluated the same way
    fl_s, t_s, fl_c, t_c, t_r = r64["terms"]
    ab = (fl_s.abs().sum().reshape(1), t_s.abs().sum(dim=0), fl_c.abs().sum().reshape(1), t_c.abs().sum(dim=0), t_r.abs().sum(dim=0))
    mrec, _ = T64.fcos_mag(*ab, None, 1.0, cflags, klw, wmul, wdiv)
    ef, el = (4 + D_BLOCK + 2 * M_FOCAL) * L64.U, (1 + D_BLOCK + 2 * M_LOC) * L64.U
    plus = []
    for s, a in zip(r64["sums"], ab):
        e = a * (ef if s.numel() == 1 else el)
        if s.numel() == 8:
            e[0], e[5], e[1] = 0.0, 0.0, -e[1]
        plus.append(s + e)
    moved, _ = T64.fcos_tail(*plus, None, 1.0, cflags, klw, wmul, wdiv)
    nrec, _ = T64.fcos_counts(cflags)
    return torch.tensor(nrec, dtype=F64) * L64.U * mrec + (moved - r64["rec"]).abs()


def check_joint(tag, rec, dlg, dbx, sets, r64, r32, consts, cont, scale=1.0):
    k = rec.cpu().double()
    err, bound = (k - r64["rec"]).abs(), rec_bound(r64, consts)
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print("RATIO joint rec %s worst %.3f" % (tag, float(ratio.max())))
    assert torch.isfinite(rec).all() and float(ratio.max()) <= 1.0, (tag, ratio.tolist(), k.tolist(), r64["rec"].tolist())
    c32 = torch.tensor(scale, dtype=F32)
    for name, g, M in (("dlogits", dlg, M_FOCAL), ("dbox", dbx, M_LOC)):
        g64, s = L64.total_and_scale(r64[name])
        g32, _ = L64.total_and_scale(r32[name])
        # Below 2^-126 fp32 has no relative precision u, only the grid 2^-149: there the rule of grad_ok asks for less than half a grid
        # step, which no fp32 result owes.  The tail's coefficients (0.05 / 4 n and smaller) carry elements of d box into that range,
        # which the per-kernel grids never reach.  Such an element is the sum of at most three branch results, each rounded once onto
        # the grid (half a step each; adding denormals is exact): one within 1.5 x 2^-149 of r64 is as good as fp32 allows and is handed
        # to grad_ok at its reference value; every other element, tiny or not, stands before the unchanged rule.
        # Measured: row 3, column 21 of klloss / quality / shared: k 2.95738716e-39, r64 2.95738861e-39, 1.03 steps (ratio 4.1 by the rule).
        kc = g.cpu()
        tiny = (g64.abs() * float(c32) < 2.0 ** -126) & (g64 != 0) & ((kc.double() - g64 * c32.double()).abs() <= 1.5 * 2.0 ** -149)
        kc = torch.where(tiny, (g64 * c32.double()).float(), kc)
        ok, res = L64.grad_ok(kc, g64 * c32.double(), g32 * c32, s * float(c32), M)
        print("RATIO joint %s %s worst %.3f excluded %.4f n %d" % (name, tag, res["ratio"], res["excluded"], res["n"]))
        assert ok, (tag, name, res)
    (ls, _), (lc, _), (lr, _, _) = sets
    pos = lambda l: (l >= 0) & (l != 80)    # noqa: E731
    nopos = ~(pos(ls) | pos(lc) | pos(lr))
    gb, gl = dbx.cpu(), dlg.cpu()
    assert T64.is_pos_zero(gb[nopos].abs()) and T64.is_pos_zero(gb[:, (9 if cont else 73):].abs()), tag
    assert T64.is_pos_zero(gl[(ls < 0) & (lc < 0)].abs()), tag


def run_joint(layout, seed, consts, cont=False, BS=80):
    O = ops()
    logits, box, sets, r64, r32 = joint_refs(layout, seed, consts, cont, BS)
    assert box.shape == (T64.JOINT_P, 16 if cont else BS)
    lg, bx = dev(logits).requires_grad_(True), dev(box).requires_grad_(True)
    total, rec = O.fcos_joint_loss(lg, bx, dev_sets(sets), consts, lambda a, b, c: None)
    assert same_bits(total, rec[7])
    for shape in (lg.shape, bx.shape):      # best effort: the node allocates its gradients with empty_like - leave NaN where they may land
        junk = torch.full(shape, float("nan"), device=DEV)
        del junk
    dlg, dbx = torch.autograd.grad(total, (lg, bx), retain_graph=True)
    return rec, dlg, dbx, (lg, bx, total), (sets, r64, r32)


def scales_by_1024(g1, gk):
    """an upstream gradient of 1024 scales the result bit for bit.  Where the result at 1 is a denormal it was rounded on a coarser grid
    than its scaled twin: there the two agree to that grid, 2^-149 x 1024.  Both gradients have such elements: d logits below the
    saturated focal logits, d box in the far bins of a sharply peaked row (measured: one element of 10320, -1.4714e-43 at 1 against
    -1.4717e-43 = its twin / 1024; up to 1.6 % of d box with the small coefficients of "klloss").  Every normal element is held bit for
    bit."""
    a, b = g1.cpu(), gk.cpu()
    normal = a.abs() >= 2.0 ** -126
    assert same_bits(b[normal], a[normal] * 1024.0)
    assert torch.all((b[~normal].double() - a[~normal].double() * 1024.0).abs() <= 1024.0 * 2.0 ** -149)


def reg_max(cont):
    return hip().REG_CONT if cont else 16


JOINT_GRID = [      # (KL type, unify, TS-better, layout, seed): the eight cells, plain supervised flags
    ("nlloss", False, True, "fused", 4100), ("nlloss", False, False, "shared", 4200),
    ("nlloss", True, True, "shared", 4200), ("nlloss", True, False, "fused", 4100),
    ("klloss", False, True, "shared", 4200), ("klloss", False, False, "fused", 4100),
    ("klloss", True, True, "fused", 4100), ("klloss", True, False, "shared", 4200),
]
# (KL type, unify, TS-better, quality IoU on the supervised flags, layout, seed, BS): every cell at both row pitches, plus LT_QUALITY_IOU on
# the supervised flags for one case of each KL type
JOINT_CONFIGS = [(k, u, t, False, lay, seed, BS) for BS in (80, 76) for (k, u, t, lay, seed) in JOINT_GRID] + [
    ("nlloss", True, False, True, "fused", 4100, 76), ("klloss", False, False, True, "shared", 4200, 80)]


def joint_flags(kl_type, unify, tsb, quality):
    cflags = 1 | (2 if kl_type == "klloss" else 0) | (4 if unify else 0) | (8 if tsb else 0)
    fp = L64.LT_KLLOSS if kl_type == "klloss" else 0
    return cflags, fp | (L64.LT_QUALITY_IOU if quality else 0), fp


@pytest.mark.parametrize("kl_type,unify,tsb,quality,layout,seed,BS", JOINT_CONFIGS)
def test_fcos_joint_loss_vs_fp64(kl_type, unify, tsb, quality, layout, seed, BS):
    consts = T64.joint_consts(*joint_flags(kl_type, unify, tsb, quality), reg_max(False))
    tag = "%s u%d ts%d q%d %s BS%d" % (kl_type, unify, tsb, quality, layout, BS)
    rec, dlg, dbx, (lg, bx, total), (sets, r64, r32) = run_joint(layout, seed, consts, BS=BS)
    check_joint(tag, rec, dlg, dbx, sets, r64, r32, consts, False)
    dlg_k, dbx_k = torch.autograd.grad(total, (lg, bx), grad_outputs=torch.tensor(1024.0, device=DEV))
    assert dbx_k.shape == (T64.JOINT_P, BS)
    scales_by_1024(dlg, dlg_k)
    scales_by_1024(dbx, dbx_k)


def test_fcos_joint_loss_continuous_head_vs_fp64():
    consts = T64.joint_consts(*joint_flags("nlloss", False, True, False), reg_max(True))
    rec, dlg, dbx, _, (sets, r64, r32) = run_joint("fused", 4100, consts, cont=True)
    check_joint("cont", rec, dlg, dbx, sets, r64, r32, consts, True)


@pytest.mark.parametrize("BS", [80, 76])
@pytest.mark.parametrize("tsb", [True, False])
def test_fcos_joint_loss_without_any_positive(tsb, BS):
    """an all-background supervised set and pseudo sets without a positive: every clamp of the tail at once"""
    consts = T64.joint_consts(*joint_flags("nlloss", False, tsb, False), reg_max(False))
    rec, dlg, dbx, _, (sets, r64, r32) = run_joint("empty", 4300, consts, BS=BS)
    assert torch.isfinite(rec).all() and torch.isfinite(dlg).all() and torch.isfinite(dbx).all()
    check_joint("empty ts%d" % tsb, rec, dlg, dbx, sets, r64, r32, consts, False)
    assert T64.is_pos_zero(dbx.cpu().abs())


@pytest.mark.parametrize("kl_type,unify", [("nlloss", False), ("klloss", True)])
@pytest.mark.parametrize("node", ["1", "0"])
def test_joint_losses_both_paths_vs_fp64(node, kl_type, unify, monkeypatch):
    """FCOSOutputs.joint_losses as one node (UTV2_JOINT_LOSS_NODE unset / 1) and as separate nodes + _FcosCombineFn (0), the target kernel
    replaced by the synthetic sets"""
    from ubteacher.modeling.fcos import FCOSOutputs
    from ubteacher.presets import get_config
    monkeypatch.setenv("UTV2_JOINT_LOSS_NODE", node)
    fo = FCOSOutputs(get_config("fcos", 1, ["MODEL.FCOS.KL_LOSS_TYPE", kl_type, "MODEL.FCOS.UNIFY_CTRCLS", unify]))
    tsb = fo.reg_unsup_loss == "ts_locvar_better_nms_nll_l1"
    cflags, flags_s, flags_p = joint_flags(kl_type, unify, tsb, fo.quality_iou)
    flags_s, flags_p = flags_s | fo.loc_flags, flags_p | fo.loc_flags
    base = T64.joint_consts(cflags, flags_s, flags_p, 16, klw=fo.kl_loss_weight)
    consts = (fo.focal_loss_alpha, fo.focal_loss_gamma, 80, 16, flags_s, flags_p, T64.f32(fo.tsbetter_reg), T64.f32(fo.tsbetter_reg_cert)) + base[8:]
    logits, box, sets, r64, r32 = joint_refs("fused", 4100, consts, False)
    dsets = dev_sets(sets)
    queue = [(dsets[0][0], dsets[0][1], None, None), (dsets[1][0], dsets[1][1], None, None), (dsets[2][0], dsets[2][1], dsets[2][2], None)]
    monkeypatch.setattr(fo, "_targets", lambda *a, **k: queue.pop(0))
    lg, bx = dev(logits).requires_grad_(True), dev(box).requires_grad_(True)
    weights = {k: (m, d) for k, m, d in zip(fo.LOSS_KEYS, consts[11], consts[12])}
    l_sup, l_uns, total = fo.joint_losses({"logits": lg, "box": bx}, None, None, {"cls": None, "reg": None}, 1, 2, weights)
    rec = torch.stack([l_sup["loss_fcos_cls"], l_sup["loss_fcos_loc"], l_sup["loss_fcos_ctr"], l_uns["loss_fcos_cls"], l_uns["loss_fcos_ctr"],
                       l_uns["loss_fcos_loc"], l_uns.get("teacher_better_student", torch.zeros((), device=DEV)), total.detach()])
    dlg, dbx = torch.autograd.grad(total, (lg, bx))
    check_joint("path %s %s" % (node, kl_type), rec, dlg, dbx, sets, r64, r32, consts, False)
