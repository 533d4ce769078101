"""The fused loss kernels (csrc/fcos.hip, csrc/rcnn.hip), called directly through ubteacher.hip, element by element against the fp64
autograd references of tests/loss_ref64.py on deterministic grids that sit ON the kernels' branch points (ties, thresholds, the
log1p series switch, clamp bounds) and in saturation.

Rule for every gradient element (loss_ref64.grad_ratio): |k - r64| <= M max(|r32 - r64|, u |r64|) + M u s, u = 2^-24, r32 = the same
reference function in fp32 on the CPU, s = the largest addend of that element in the reference.  No absolute tolerance anywhere.
Rule for every forward sum: |k - sum r64| <= (L + D + 2 M) u sum |r64_i|, L = longest serial fp32 chain of one thread, D = depth
of the reduction tree, both read off the launch geometry (derivations next to each family below).

M per family: twice the worst ratio measured on the MI355X over the whole grid, rounded up to a power of two, at most 16
(DESIGN.md "Loss-kernel accuracy against fp64" has the measured figures).  Each test prints its worst ratio before it asserts.

Measured worst ratios on the MI355X (whole grid per family, `s` = the loss-part addends only): rpn 1.0, loc terms 2.0, softmax focal 4.1,
sigmoid focal 5.2, roi box loss 11.1 (gd) / 7.5 (gs); twice 11.1 exceeds 16, so roi sits at the cap with less than the usual headroom.
Elements where fp64 autograd itself cancels to an exact 0 (r64 == r32 == 0, all addends 0) while the kernel returns the true ~1e-23
are excluded and counted against the 2 % cap (loss_ref64.grad_ratio); at most 1.6 % of a case (focal P 257, C 1, gamma 0)."""
import math

import pytest
import torch

from tests import loss_ref64 as L64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64

M_FOCAL, M_LOC, M_SOFTMAX, M_RPN, M_ROI = 16, 4, 16, 2, 16

# block_reduce_sum (csrc/common.h): six shuffle levels inside a wave, then six more over the per-wave partials = 12 dependent adds;
# sum_partials_kernel adds the per-block partials in DOUBLE and rounds once (+ 1).
D_BLOCK = 12 + 1


def hip():
    from ubteacher import hip as H
    return H


def dev(t):
    return None if t is None else t.to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check_grad(tag, k, parts64, parts32, M, scale=1.0, s=None):
    r64, s64 = L64.total_and_scale(parts64)
    r32, _ = L64.total_and_scale(parts32)
    if s is not None:
        s64 = s
    c32 = torch.tensor(scale, dtype=F32)
    ok, res = L64.grad_ok(k.cpu(), r64 * c32.double(), r32 * c32, s64 * abs(float(c32)), M)
    print("RATIO %s worst %.3f excluded %.4f n %d" % (tag, res["ratio"], res["excluded"], res["n"]))
    if not ok and res["argmax"] >= 0:
        i = res["argmax"]
        print("WORST %s at %d: k %.9g r64 %.17g r32 %.9g s %.9g" % (tag, i, float(k.cpu().reshape(-1)[i]), float((r64 * c32.double()).reshape(-1)[i]),
                                                             float((r32 * c32).reshape(-1)[i]), float(s64.reshape(-1)[i]) * abs(float(c32))))
    assert ok, (tag, res["ratio"], res["excluded"], res["class_ok"], res["argmax"])
    return res["ratio"]


def check_sum(tag, k, terms64, Lc, D, M):
    ref, bound = L64.sum_bound(terms64, Lc, D, M)
    err = abs(float(k) - ref)
    print("SUM %s k %.9g ref %.9g err %.3g bound %.3g" % (tag, float(k), ref, err, bound))
    assert math.isfinite(float(k)) and err <= bound, (tag, float(k), ref, err, bound)


# =================================================================================================
# sigmoid focal.  Forward geometry (utv2_sigmoid_focal_fwd): 1024 blocks x 256 threads; C % 4 == 0: a thread adds the 4 terms of a
# quad per trip, ceil(P C / 4 / 262144) trips -> L = 4 ceil(P C / 1048576); scalar path: L = ceil(P C / 262144).  D = D_BLOCK.
# =================================================================================================
FOCAL_SHAPES = [(1, 80), (257, 80), (3001, 80), (1, 1), (257, 1), (3001, 3), (257, 3), (1, 81), (257, 81), (2003, 81)]


FOCAL_GAMMAS, FOCAL_ALPHAS = [2.0, 1.5, 0.0], [0.25, 0.5, -1.0]


def focal_grid(P, C):
    return L64.focal_case(P, C, 1000 + P + C)


@pytest.mark.parametrize("alpha", FOCAL_ALPHAS)
@pytest.mark.parametrize("gamma", FOCAL_GAMMAS)
@pytest.mark.parametrize("P,C", FOCAL_SHAPES)
def test_focal_vs_fp64(P, C, gamma, alpha):
    H = hip()
    x, lab = focal_grid(P, C)
    loss64, p64 = L64.focal(x.double(), lab, C, alpha, gamma)
    _, p32 = L64.focal(x, lab, C, alpha, gamma)
    xd, ld = dev(x), dev(lab)
    f1 = H.sigmoid_focal_fwd(xd, ld, alpha, gamma).cpu()
    f2 = H.sigmoid_focal_fwd(xd, ld, alpha, gamma).cpu()
    assert same_bits(f1, f2)
    Lc = 4 * math.ceil(P * C / 1048576) if C % 4 == 0 else math.ceil(P * C / 262144)
    tag = "focal P%d C%d g%g a%g" % (P, C, gamma, alpha)
    check_sum(tag, f1[0], loss64, Lc, D_BLOCK, M_FOCAL)
    coef = torch.tensor([0.37], dtype=F32)
    g = H.sigmoid_focal_bwd(xd, ld, alpha, gamma, dev(coef))
    check_grad(tag, g, p64, p32, M_FOCAL, scale=0.37)
    assert torch.all(g.cpu()[lab < 0] == 0)


def test_focal_negative_alpha_is_unweighted():
    """MODEL.FCOS.LOSS_ALPHA < 0 (fvcore: no class weighting).  The kernel used to weight with alpha t + (1 - alpha)(1 - t) = -1 / 2."""
    H = hip()
    x, lab = L64.focal_case(257, 80, 7, edge=False)
    loss64, p64 = L64.focal(x.double(), lab, 80, -1.0, 2.0)
    _, p32 = L64.focal(x, lab, 80, -1.0, 2.0)
    f = H.sigmoid_focal_fwd(dev(x), dev(lab), -1.0, 2.0).cpu()
    check_sum("focal alpha -1", f[0], loss64, 4, D_BLOCK, M_FOCAL)
    one = torch.ones(1, dtype=F32)
    check_grad("focal alpha -1", H.sigmoid_focal_bwd(dev(x), dev(lab), -1.0, 2.0, dev(one)), p64, p32, M_FOCAL)


def test_focal_series_switch_has_no_bias():
    """the log1p series below e < 1e-2 (|x| > 4.605): over the 64 points across the switch the SIGNED relative error of the negative-class
    gradient must average out like rounding (|mean| <= 1 u); a truncated series shows as a one-sided error on the series side (the
    three-term series the kernel had: +2.9 u on its side, with up to 100 u of scatter from log(1 + e) on the other; log1pf: -0.1 / -0.5 u)"""
    H = hip()
    sw = torch.linspace(4.55, 4.66, 32, dtype=F32)
    x = torch.cat((sw, -sw)).reshape(64, 1).repeat(1, 4).contiguous()
    lab = torch.full((64,), 4, dtype=torch.int32)          # background: every element is a negative
    loss64, p64 = L64.focal(x.double(), lab, 4, 0.25, 2.0)
    r64, _ = L64.total_and_scale(p64)
    g = H.sigmoid_focal_bwd(dev(x), dev(lab), 0.25, 2.0, dev(torch.ones(1))).cpu().double()
    rel = ((g - r64) / r64.abs())[:, 0] / L64.U
    ser = x[:, 0].abs() > 4.6052
    print("BIAS focal series side mean %.3f u, log side mean %.3f u" % (float(rel[ser].mean()), float(rel[~ser].mean())))
    assert abs(float(rel[ser].mean())) <= 1.0 and abs(float(rel[~ser].mean())) <= 1.0


@pytest.mark.parametrize("C", [80, 3])
def test_focal_bwd_acc_semantics(C):
    H = hip()
    P = 257
    x, lab = L64.focal_case(P, C, 11)
    xd, ld = dev(x), dev(lab)
    coef = dev(torch.tensor([0.37], dtype=F32))
    g0 = H.sigmoid_focal_bwd(xd, ld, 0.25, 2.0, coef).cpu()
    ga = H.sigmoid_focal_bwd_acc(xd, ld, 0.25, 2.0, coef, None, torch.full((P, C), 7.0, device=DEV), False).cpu()
    gb = H.sigmoid_focal_bwd_acc(xd, ld, 0.25, 2.0, coef, dev(torch.ones(1)), torch.full((P, C), 7.0, device=DEV), False).cpu()
    assert same_bits(g0, ga) and same_bits(g0, gb)           # gscale absent == gscale 1; accumulate 0 overwrites, skipped rows zero
    assert torch.all(g0[lab < 0] == 0)
    pre = torch.randn((P, C), generator=torch.Generator().manual_seed(5))
    pre[1, 0] = float("nan")                                  # a skipped row: its sentinel must survive bit for bit
    gc = H.sigmoid_focal_bwd_acc(xd, ld, 0.25, 2.0, coef, None, dev(pre.clone()), True).cpu()
    skip = lab < 0
    assert same_bits(gc[skip], pre[skip])                     # untouched: the sentinel bits survive
    assert same_bits(gc[~skip], (pre + g0)[~skip])            # one fp32 add
    # a device gscale multiplies coef before the product with the derivative
    gs = torch.tensor([0.5], dtype=F32)
    gd = H.sigmoid_focal_bwd_acc(xd, ld, 0.25, 2.0, coef, dev(gs), torch.zeros((P, C), device=DEV), False).cpu()
    half = H.sigmoid_focal_bwd(xd, ld, 0.25, 2.0, dev(torch.tensor([0.37], dtype=F32) * gs)).cpu()
    assert same_bits(gd, half)


# =================================================================================================
# FCOS location terms.  Forward geometry (utv2_fcos_loc_terms_fwd): 512 blocks x 128 threads, one row per thread and trip:
# L = ceil(P / 65536) adds per column, D = D_BLOCK.
# =================================================================================================
COEF4 = (0.61, 1.3, 0.05, 0.4)


def loc_run(case, flags, P, BS, with_bvars, tag):
    H = hip()
    box, t, bv, lab = case
    t64 = L64.loc_terms(box.double(), t, bv, lab, flags, 0.1, 0.5, coef=[float(torch.tensor(c, dtype=F32)) for c in COEF4])
    t32 = L64.loc_terms(box, t, bv, lab, flags, 0.1, 0.5, coef=[float(torch.tensor(c, dtype=F32)) for c in COEF4])
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, 16, 0.1, 0.5)
    s1 = H.fcos_loc_terms_fwd(*args, flags=flags).cpu()
    s2 = H.fcos_loc_terms_fwd(*args, flags=flags).cpu()
    assert same_bits(s1, s2)
    for col in range(7):
        check_sum("%s col%d" % (tag, col), s1[col], t64[0][:, col], math.ceil(P / 65536), D_BLOCK, M_LOC)
    assert float(s1[7]) == 0.0
    g = H.fcos_loc_terms_bwd(*args, dev(torch.tensor(COEF4, dtype=F32)), flags=flags)
    check_grad(tag, g, t64[1], t32[1], M_LOC)
    gc = g.cpu()
    nonpos = (lab < 0) | (lab == 80)
    assert torch.all(gc[nonpos] == 0) and torch.all(gc[:, 73:] == 0)
    return g


LOC_SHAPES, LOC_SHAPE_FLAGS = [(1, 76), (1, 80), (129, 76), (2003, 76), (2003, 80)], [0, 7, 26]


def loc_flag_grid(flags, with_bvars):
    return L64.loc_case(129, 80, 300 + flags, with_bvars=with_bvars)


def loc_shape_grid(P, BS):
    case = L64.loc_case(P, BS, 500 + P + BS)
    if P == 1:
        case[3][0] = 3   # the single row is a positive
    return case


@pytest.mark.parametrize("with_bvars", [False, True])
@pytest.mark.parametrize("flags", L64.LEGAL_FLAGS)
def test_loc_terms_all_flags_vs_fp64(flags, with_bvars):
    loc_run(loc_flag_grid(flags, with_bvars), flags, 129, 80, with_bvars, "loc f%d bv%d" % (flags, with_bvars))


@pytest.mark.parametrize("flags", LOC_SHAPE_FLAGS)
@pytest.mark.parametrize("P,BS", LOC_SHAPES)
def test_loc_terms_shapes_vs_fp64(P, BS, flags):
    case = loc_shape_grid(P, BS)
    loc_run(case, flags, P, BS, True, "loc P%d BS%d f%d" % (P, BS, flags))


def test_loc_terms_all_background_is_exactly_zero():
    H = hip()
    box, t, bv, lab = L64.loc_case(129, 80, 9, all_background=True)
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, 16, 0.1, 0.5)
    assert torch.all(bits(H.fcos_loc_terms_fwd(*args)) == 0)
    assert torch.all(bits(H.fcos_loc_terms_bwd(*args, dev(torch.tensor(COEF4, dtype=F32)))) == 0)


@pytest.mark.parametrize("BS", [76, 80])
def test_loc_terms_bwd_acc_semantics(BS):
    H = hip()
    P = 129
    box, t, bv, lab = L64.loc_case(P, BS, 21)
    args = (dev(lab), dev(box), dev(t), dev(bv), 80, 16, 0.1, 0.5)
    c4 = torch.tensor(COEF4, dtype=F32)
    c8 = torch.tensor([9.0, 9.0, COEF4[0], COEF4[1], COEF4[2], 9.0, COEF4[3], 9.0], dtype=F32)
    g0 = H.fcos_loc_terms_bwd(*args, dev(c4), flags=0).cpu()
    ga = H.fcos_loc_terms_bwd_acc(*args, dev(c8), None, torch.full((P, BS), 7.0, device=DEV), False, flags=0).cpu()
    gb = H.fcos_loc_terms_bwd_acc(*args, dev(c8), dev(torch.ones(1)), torch.full((P, BS), 7.0, device=DEV), False, flags=0).cpu()
    assert same_bits(g0, ga) and same_bits(g0, gb)            # coef8 == coef[4] at [2], [3], [4], [6]; gscale absent == 1
    pre = torch.randn((P, BS), generator=torch.Generator().manual_seed(6))
    pre[5, 0] = float("nan")                                  # a skipped row
    gc = H.fcos_loc_terms_bwd_acc(*args, dev(c8), None, dev(pre.clone()), True, flags=0).cpu()
    nonpos = (lab < 0) | (lab == 80)
    assert same_bits(gc[nonpos], pre[nonpos])
    assert same_bits(gc[~nonpos][:, :73], (pre + g0)[~nonpos][:, :73])
    assert same_bits(gc[:, 73:], pre[:, 73:])                 # the pad columns are untouched under accumulate


# =================================================================================================
# softmax focal.  Forward geometry (utv2_softmax_focal_fwd): 256 blocks x 4 waves, one wave per row and trip, lane 0 adds:
# L = ceil(R / 1024); the 4 wave partials are added in a chain (3), the block partials serially in double (+ 1): D = 4.
# =================================================================================================
SOFTMAX_C, SOFTMAX_R, SOFTMAX_GAMMAS = [2, 64, 65, 81, 129], [67, 1023], [1.5, 2.0]


def softmax_grid(R, C):
    return L64.softmax_case(R, C, 40 + C + R)


@pytest.mark.parametrize("gamma", SOFTMAX_GAMMAS)
@pytest.mark.parametrize("R", SOFTMAX_R)
@pytest.mark.parametrize("C", SOFTMAX_C)
def test_softmax_focal_vs_fp64(C, R, gamma):
    H = hip()
    x, tgt = softmax_grid(R, C)
    l64, g64, s64 = L64.softmax_focal(x.double(), tgt, gamma)
    _, g32, _ = L64.softmax_focal(x, tgt, gamma)
    xd, td = dev(x), dev(tgt)
    f1, f2 = H.softmax_focal_fwd(xd, td, gamma).cpu(), H.softmax_focal_fwd(xd, td, gamma).cpu()
    assert same_bits(f1, f2)
    tag = "softmax C%d R%d g%g" % (C, R, gamma)
    check_sum(tag, f1[0], l64, math.ceil(R / 1024), 4, M_SOFTMAX)
    g = H.softmax_focal_bwd(xd, td, gamma, dev(torch.tensor([0.37], dtype=F32)))
    check_grad(tag, g, g64, g32, M_SOFTMAX, scale=0.37, s=s64)
    assert torch.all(g.cpu()[tgt < 0] == 0)


# =================================================================================================
# RPN losses.  Forward geometry (utv2_rpn_loss_fwd): ONE block of 256 threads, thread t adds slots t, t + 256, ...: L = ceil(N S / 256)
# (x 4 for the location sum: four |d - t| per slot), then an 8-level LDS tree: D = 8.
# =================================================================================================
@pytest.mark.parametrize("with_scores", [False, True])
def test_rpn_loss_dense_and_head_vs_fp64(with_scores):
    H = hip()
    c = L64.rpn_case(RPN_SEED, with_scores=with_scores)
    N, A, R, ch, hw = c["N"], c["A"], c["R"], c["ch"], c["hw"]
    sd = {k: dev(v) for k, v in c["s"].items()}
    ref = {}
    for dt in (F64, F32):
        x, dl = L64.rpn_slot_inputs(c, dt)
        ref[dt] = L64.rpn_loss(x, dl, c["anchors"], c["s"], c["gt_boxes"], c["gt_scores"], c["weights"])
    common = (N, A, R, dev(c["anchors"]), sd, dev(c["gt_boxes"]), dev(c["gt_scores"]), c["weights"])
    dense = H.rpn_loss_fwd(dev(c["obj"]), dev(c["deltas"]), None, *common)
    dense2 = H.rpn_loss_fwd(dev(c["obj"]), dev(c["deltas"]), None, *common)
    hd = dev(c["head"])
    head = H.rpn_loss_fwd(hd, hd, hw, *common)
    for a, b, b2 in zip(dense, head, dense2):
        assert same_bits(a, b) and same_bits(a, b2)           # the two layouts and two runs give the same bits
    sums, gobj, gdl = [t.cpu() for t in dense]
    S = gobj.shape[1]
    tag = "rpn scores%d" % with_scores
    check_sum(tag + " cls", sums[0], ref[F64][0], math.ceil(N * S / 256), 8, M_RPN)
    check_sum(tag + " loc", sums[1], ref[F64][1], 4 * math.ceil(N * S / 256), 8, M_RPN)
    check_grad(tag + " gobj", gobj, [ref[F64][2]], [ref[F32][2]], M_RPN)
    assert torch.equal(gdl.double(), ref[F64][3])             # signs: exact (a delta equal to its target gives 0)
    valid = torch.cat((c["s"]["pos_valid"], c["s"]["neg_valid"]), dim=1).bool()
    assert torch.all(gobj[~valid] == 0) and torch.all(gdl[N - 1] == 0)   # empty slots and the image without gt: nothing, although their
    if with_scores:                                                       # indices name NaN / inf logits; the pseudo branch weights
        assert torch.all(gobj[N - 1] == 0)                                # an image without boxes by 0
    # backward: a pure scatter of gout * per-slot derivative to the sampled anchors; everything else keeps the caller's zero
    gc, gl = torch.tensor([0.7], dtype=F32), torch.tensor([1.9], dtype=F32)
    go, gd = torch.zeros((N, R), device=DEV), torch.zeros((N, R, 4), device=DEV)
    H.rpn_loss_bwd(dense[1], dense[2], dev(gc), dev(gl), None, N, A, 0, R, sd, go, gd)
    gh = torch.zeros_like(hd)
    H.rpn_loss_bwd(dense[1], dense[2], dev(gc), dev(gl), hw, N, A, ch, R, sd, gh, gh)
    eo, ed, eh = torch.zeros((N, R)), torch.zeros((N, R, 4)), torch.zeros(c["head"].numel())
    idx = torch.cat((c["s"]["pos_idx"], c["s"]["neg_idx"]), dim=1)
    npos = c["s"]["pos_idx"].shape[1]
    for n in range(N):
        for j in range(S):
            if not valid[n, j]:
                continue
            r = int(idx[n, j])
            oo, od = L64.rpn_head_offsets(hw, N, A, ch, n, r)
            eo[n, r] = eh[oo] = gobj[n, j] * gc[0]
            if j < npos:
                ed[n, r] = gdl[n, j] * gl[0]
                eh[od:od + 4] = ed[n, r]
    assert same_bits(go, eo) and same_bits(gd, ed) and same_bits(gh.reshape(-1), eh)


# =================================================================================================
# ROI box losses.  Forward geometry (utv2_roi_box_loss): ONE block of 256 threads, thread t takes rows t, t + 256, ... and adds at
# most 5 terms per row (four |d - t|, one NLL * IoU): L = 5 ceil(R / 256), 8-level LDS tree: D = 8.
# =================================================================================================
ROI_R = [1, 255, 600]
RPN_SEED = 77


def roi_grid(R):
    c = L64.roi_case(R, 60 + R)
    if R == 1:
        c["cls"][0] = 5
    return c


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("R", ROI_R)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_roi_box_loss_vs_fp64(mode, R, ld):
    H = hip()
    c = roi_grid(R)
    wx, wy = L64.ROI_W
    a = (c["cls"], c["prop"], c["gtb"], c["gstd"], 80, mode, wx, wy, L64.ROI_CLAMP, 0.1, 0.5)
    l64, gd64, gs64 = L64.roi_box_loss(c["mat"][:, :4].double(), c["mat"][:, 4:].double(), *a)
    _, gd32, gs32 = L64.roi_box_loss(c["mat"][:, :4], c["mat"][:, 4:], *a)
    m = dev(c["mat"])
    de, st = (m[:, :4], m[:, 4:]) if ld == 8 else (m[:, :4].clone(memory_format=torch.contiguous_format), m[:, 4:].clone(memory_format=torch.contiguous_format))
    assert R == 1 or de.stride(0) == ld
    k = (dev(c["cls"]), dev(c["prop"]), dev(c["gtb"]), dev(c["gstd"]), 80, mode, wx, wy, L64.ROI_CLAMP, 0.1, 0.5)
    o1, o2 = H.roi_box_loss(de, st, *k), H.roi_box_loss(de, st, *k)
    for x1, x2 in zip(o1, o2):
        assert same_bits(x1, x2)
    tag = "roi m%d R%d ld%d" % (mode, R, ld)
    check_sum(tag, o1[0].cpu()[0], l64, 5 * math.ceil(R / 256), 8, M_ROI)
    check_grad(tag + " gd", o1[1], gd64, gd32, M_ROI)
    check_grad(tag + " gs", o1[2], gs64, gs32, M_ROI)
    bg = (c["cls"] < 0) | (c["cls"] >= 80)
    assert torch.all(o1[1].cpu()[bg] == 0) and torch.all(o1[2].cpu()[bg] == 0)
    if mode != 0:
        assert torch.all(o1[2].cpu() == 0)


# =================================================================================================
# the defects these tests found, each kept as a named case
# =================================================================================================
def test_focal_gamma0_negative_below_minus_17_has_a_gradient():
    """1 - p_t was formed as 1 - (1 - p): below x = -17 the fp32 1 - p is 1 and the gradient of a negative at gamma 0 (alpha p) was exactly 0"""
    H = hip()
    x = torch.tensor([-17.5, -20.0, -30.0, -50.0, -80.0], dtype=F32).reshape(5, 1).repeat(1, 4).contiguous()
    lab = torch.full((5,), 4, dtype=torch.int32)
    _, p64 = L64.focal(x.double(), lab, 4, 0.25, 0.0)
    _, p32 = L64.focal(x, lab, 4, 0.25, 0.0)
    g = H.sigmoid_focal_bwd(dev(x), dev(lab), 0.25, 0.0, dev(torch.ones(1)))
    assert torch.all(g.cpu() > 0)
    check_grad("focal gamma 0 below -17", g, p64, p32, M_FOCAL)


def test_focal_saturated_positive_gradient_is_not_lost():
    """a positive at x = 50 / 87 (gamma 0): the true gradient -alpha (1 - p) ~ 1e-23 / 1e-39 is what the kernel returns; fp64 autograd
    cancels sigmoid(x) - 1 to an exact 0 there (the degenerate elements of loss_ref64.grad_ratio), so this is checked against exp(-x)"""
    H = hip()
    x = torch.tensor([50.0, 87.0], dtype=F32).reshape(2, 1).repeat(1, 4).contiguous()
    lab = torch.zeros(2, dtype=torch.int32)
    g = H.sigmoid_focal_bwd(dev(x), dev(lab), 0.25, 0.0, dev(torch.ones(1))).cpu().double()[:, 0]
    ref = -0.25 * torch.exp(-x[:, 0].double()) / (1 + torch.exp(-x[:, 0].double()))
    print("RATIO focal saturated positive rel err / u", ((g - ref).abs() / ref.abs() / L64.U).tolist())
    assert torch.all((g - ref).abs() <= M_FOCAL * L64.U * ref.abs())


def test_loc_terms_sharply_peaked_rows_keep_j_minus_d():
    """one bin 12 above the rest: d = jm + 1e-4.  (j - d) at the mode and (t - d) lost up to 9e-2 of their value to the rounding of
    d = sum p_j j in the fp32 backward; the Integral around the mode, in double, keeps them"""
    P = 64
    box, t, bv, lab = L64.loc_case(P, 80, 91, edge=False)
    g = torch.Generator().manual_seed(92)
    jm = torch.randint(1, 16, (P, 4), generator=g)
    for r in range(P):
        for b in range(4):
            box[r, b * 17 + int(jm[r, b])] += 12.0
    t = jm.float() + 0.375
    lab[:] = 3
    for flags in (0, 2, 7):
        loc_run((box, t, bv, lab), flags, P, 80, True, "loc peaked f%d" % flags)


def test_softmax_focal_logits_of_order_1e4():
    """CE was (log s + m) - x_t: with m ~ 1e4 the sum rounds at 1e-3 before x_t is taken off; now log s + (m - x_t)"""
    H = hip()
    x, tgt = L64.softmax_case(64, 81, 5, edge=False)
    x = (x + 1e4).contiguous()
    l64, g64, s64 = L64.softmax_focal(x.double(), tgt, 1.5)
    _, g32, _ = L64.softmax_focal(x, tgt, 1.5)
    check_sum("softmax 1e4", H.softmax_focal_fwd(dev(x), dev(tgt), 1.5).cpu()[0], l64, 1, 4, M_SOFTMAX)
    check_grad("softmax 1e4", H.softmax_focal_bwd(dev(x), dev(tgt), 1.5, dev(torch.ones(1))), g64, g32, M_SOFTMAX, s=s64)


# =================================================================================================
# argument combinations the entry points do not implement are refused with UTV2_EARG (-1000), not computed wrongly
# =================================================================================================
EARG = "failed with code -1000"


def test_unsupported_arguments_are_refused():
    H = hip()
    box, t, bv, lab = L64.loc_case(5, 80, 1)
    bx, lb, tt, bb = dev(box), dev(lab), dev(t), dev(bv)
    with pytest.raises(RuntimeError, match=EARG):
        H.fcos_loc_terms_fwd(lb, bx, tt, bb, 80, 8, 0.1, 0.5)                                  # reg_max != 16
    with pytest.raises(RuntimeError, match=EARG):
        H.fcos_loc_terms_fwd(lb, bx, tt, bb, 80, 16, 0.1, 0.5, flags=12)                       # loc type 3
    with pytest.raises(RuntimeError, match=EARG):
        H.fcos_loc_terms_fwd(lb, bx[:, :72].contiguous(), tt, bb, 80, 16, 0.1, 0.5)            # box_stride < 73
    out, sums, ws, one4 = torch.full((5, 80), 7.0, device=DEV), torch.full((8,), 7.0, device=DEV), torch.zeros(4096, device=DEV), dev(torch.ones(4))
    st = H._stream()
    p = lambda a: a.data_ptr()   # noqa: E731
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_sigmoid_focal_fwd", p(bx), p(lb), 5, 0, 0.25, 2.0, p(sums), p(ws), st)                      # C == 0
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_sigmoid_focal_fwd", p(bx), p(lb), -1, 80, 0.25, 2.0, p(sums), p(ws), st)                    # P < 0
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_sigmoid_focal_bwd", p(bx), p(lb), -1, 80, 0.25, 2.0, p(one4), p(out), st)
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_fcos_loc_terms_bwd", p(lb), p(bx), 80, p(tt), None, -1, 80, 16, 0.1, 0.5, 0, p(one4), p(out), st)
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_softmax_focal_fwd", p(bx), p(lb), -1, 80, 1.5, p(sums), p(ws), st)                          # R < 0
    with pytest.raises(RuntimeError, match=EARG):
        H.call("utv2_softmax_focal_bwd", p(bx), p(lb), 5, 0, 1.5, p(one4), p(out), st)                           # C == 0
    # an empty batch is legal: the backward writes nothing, the forward sums are zero
    H.call("utv2_fcos_loc_terms_bwd", p(lb), p(bx), 80, p(tt), None, 0, 80, 16, 0.1, 0.5, 0, p(one4), p(out), st)
    assert torch.all(out.cpu() == 7.0)
    H.call("utv2_fcos_loc_terms_fwd", p(lb), p(bx), 80, p(tt), None, 0, 80, 16, 0.1, 0.5, 0, p(sums), p(ws), st)
    assert torch.all(sums.cpu() == 0.0)
    H.call("utv2_softmax_focal_fwd", p(bx), p(lb), 0, 80, 1.5, p(sums), p(ws), st)
    assert float(sums.cpu()[0]) == 0.0
    cls = torch.zeros(1, dtype=torch.int64, device=DEV)
    H.call("utv2_roi_box_loss", p(bx), p(bx), 8, p(cls), p(bx), p(bx), None, 0, 80, 1, 0, 10.0, 5.0, 62.5, 0.1, 0.5, p(sums), p(out), p(out), st)
    assert float(sums.cpu()[0]) == 0.0                                                                            # R == 0: sum 0
