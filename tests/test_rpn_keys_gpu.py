"""The RPN's loss, boundary and anchor-generator keys on the GPU: utv2_rpn_loss_fwd_f (csrc/rcnn.hip) in both modes against fp64 autograd
(tests/rpn_ref64.py) on rows that sit on the branch points, dense and head-indexed forms bit for bit, the old entry points against the new,
the refused arguments, utv2_rpn_sample_keys_b through both sampler paths against the executed reference (tests/golden/rpn_keys.npz), an
RPN built at A = 6, and one small Faster-RCNN step per key.

Bounds: the gradient rule and the sum bound of tests/test_loss_kernels_fp64_gpu.py (DESIGN "Loss-kernel accuracy against fp64").  The
beta-0 row keeps M_RPN = 2 and its exact signs; M of the new modes = the smallest power of two that is at least twice the worst ratio
measured on the MI355X, at most 16 (M_NEW below; DESIGN 23 has the figures).  Each test prints its ratios before it asserts."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import rpn_ref64 as R64
from tests.test_loss_kernels_fp64_gpu import M_RPN, check_grad, check_sum, same_bits

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
EARG = "failed with code -1000"
F32, F64 = torch.float32, torch.float64
MODES = [(0, 0.0), (0, 0.11), (0, 1.0), (1, 0.0)]
# measured worst gdl ratios on the MI355X over A in {1, 3, 6} x scores: smooth-L1 at beta 0.11 and at 1: 1.39 -> M = 4; giou: 5.74 -> M = 16
M_NEW = {(0, 0.0): M_RPN, (0, 0.11): 4, (0, 1.0): 4, (1, 0.0): 16}
f32 = lambda b: float(torch.tensor(b, dtype=F32))   # noqa: E731


def T(a):
    return torch.from_numpy(np.asarray(a))


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "rpn_keys.npz")))


# ---- the loss kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_scores", [False, True])
@pytest.mark.parametrize("mode,beta", MODES)
@pytest.mark.parametrize("A", [1, 3, 6])
def test_rpn_loss_f_dense_and_head_vs_fp64(A, mode, beta, with_scores):
    from ubteacher import hip as H
    beta = f32(beta)
    c = R64.rpn_key_case(77 + A, A=A, beta=beta, with_scores=with_scores, giou=mode == 1)
    N, R, hw = c["N"], c["R"], c["hw"]
    sd = {k: dev(v) for k, v in c["s"].items()}
    ref = {}
    for dt in (F64, F32):
        x, dl = L64.rpn_slot_inputs(c, dt)
        ref[dt] = R64.rpn_loss(x, dl, c["anchors"], c["s"], c["gt_boxes"], c["gt_scores"], c["weights"], mode, beta)
    common = (N, A, R, dev(c["anchors"]), sd, dev(c["gt_boxes"]), dev(c["gt_scores"]), c["weights"])
    kw = dict(loc_mode=mode, smooth_l1_beta=beta, scale_clamp=R64.SCALE_CLAMP)
    dense = H.rpn_loss_fwd(dev(c["obj"]), dev(c["deltas"]), None, *common, **kw)
    dense2 = H.rpn_loss_fwd(dev(c["obj"]), dev(c["deltas"]), None, *common, **kw)
    hd = dev(c["head"])
    head = H.rpn_loss_fwd(hd, hd, hw, *common, **kw)
    for a, b, b2 in zip(dense, head, dense2):
        assert same_bits(a, b) and same_bits(a, b2)           # the two layouts and two runs give the same bits
    sums, gobj, gdl = [t.cpu() for t in dense]
    S = gobj.shape[1]
    M = M_NEW[(mode, round(beta, 2))]
    tag = "rpn_f A%d m%d b%g scores%d" % (A, mode, beta, with_scores)
    check_sum(tag + " cls", sums[0], ref[F64][0], math.ceil(N * S / 256), 8, M_RPN)
    check_sum(tag + " loc", sums[1], ref[F64][1], 4 * math.ceil(N * S / 256), 8, M)
    check_grad(tag + " gobj", gobj, [ref[F64][2]], [ref[F32][2]], M_RPN)
    check_grad(tag + " gdl", gdl, ref[F64][3], ref[F32][3], M, s=ref[F64][4])
    g64 = L64.total_and_scale(ref[F64][3])[0]
    if mode == 0 and not beta:
        assert torch.equal(gdl.double(), g64)                 # signs: exact (a delta equal to its target gives 0)
    if mode == 0 and beta:
        # |d| == beta bit for bit is on the linear side: +-1 exactly; one ulp below: d / beta, short of 1; one ulp above: +-1
        assert torch.all(gdl[0, 3].abs() == 1.0) and torch.all(gdl[0, 4].abs() < 1.0) and torch.all(gdl[0, 5].abs() == 1.0)
        assert torch.equal(torch.sign(gdl[0, 3:6]).double(), torch.sign(g64[0, 3:6]))
    if mode == 1:
        assert float(gdl[0, 6, 2]) == 0.0 and float(gdl[0, 6, 3]) != 0.0     # dw above SCALE_CLAMP: exactly 0
    valid = torch.cat((c["s"]["pos_valid"], c["s"]["neg_valid"]), dim=1).bool()
    assert torch.all(gobj[~valid] == 0) and torch.all(gdl[N - 1] == 0) and torch.all(gdl[~c["s"]["pos_valid"].bool()] == 0)
    assert not torch.isnan(gdl).any() and not torch.isnan(gobj).any()        # (the empty slots name NaN / inf logits and -inf deltas)


def raw_loss(H, name, c, extra, head=False):
    """the C entry point `name` on NaN-filled outputs: every element must be written by the launch itself"""
    N, A, R, s = c["N"], c["A"], c["R"], c["s"]
    npos, nneg = s["pos_idx"].shape[1], s["neg_idx"].shape[1]
    out = [torch.full(sh, float("nan"), device=DEV) for sh in ((2,), (N, npos + nneg), (N, npos, 4))]
    t = {k: dev(v) for k, v in s.items()}
    keep = [dev(c["head"]) if head else dev(c["obj"]), dev(c["deltas"]), dev(c["anchors"]), dev(c["gt_boxes"]), dev(c["gt_scores"])]
    import ctypes
    hw = (ctypes.c_int * len(c["hw"]))(*c["hw"])
    wt = (ctypes.c_float * 4)(*c["weights"])
    rng = (N, 0) if "range" in name else ()
    H.call(name, keep[0].data_ptr(), (keep[0] if head else keep[1]).data_ptr(), int(head), len(c["hw"]), ctypes.cast(hw, ctypes.c_void_p), N, *rng,
           A, c["ch"] if head else 0, R, keep[2].data_ptr(), t["pos_idx"].data_ptr(), t["pos_valid"].data_ptr(), npos, t["neg_idx"].data_ptr(),
           t["neg_valid"].data_ptr(), nneg, t["matched32"].data_ptr(), t["has_gt"].data_ptr(), keep[3].data_ptr(),
           None if keep[4] is None else keep[4].data_ptr(), c["gt_boxes"].shape[1], ctypes.cast(wt, ctypes.c_void_p), *extra,
           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), H._stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("head", [False, True])
def test_old_loss_entry_points_are_the_new_ones_at_beta_zero(head):
    from ubteacher import hip as H
    c = L64.rpn_case(77)
    outs = [raw_loss(H, "utv2_rpn_loss_fwd", c, (), head), raw_loss(H, "utv2_rpn_loss_fwd_f", c, (0, 0.0, R64.SCALE_CLAMP), head),
            raw_loss(H, "utv2_rpn_loss_fwd_range", c, (), head), raw_loss(H, "utv2_rpn_loss_fwd_range_f", c, (0, 0.0, 0.0), head),
            raw_loss(H, "utv2_rpn_loss_fwd_f", c, (0, 9e-6, 0.0), head)]          # below fvcore's 1e-5: still plain L1
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert same_bits(a, b) and not torch.isnan(a).any()
    assert float(outs[0][0][1]) > 0


def test_refused_arguments():
    from ubteacher import hip as H
    c = L64.rpn_case(77)
    for extra in ((2, 0.0, 4.0), (-1, 0.0, 4.0), (0, -1.0, 4.0), (1, float("nan"), 4.0), (1, 0.0, float("nan"))):
        for name in ("utv2_rpn_loss_fwd_f", "utv2_rpn_loss_fwd_range_f"):
            with pytest.raises(RuntimeError, match=EARG):
                raw_loss(H, name, c, extra)
    N, R, Gn = 2, 300, 3
    mx, lq, gv, keys = torch.rand(N, R, device=DEV), torch.zeros(N, R, dtype=torch.uint8, device=DEV), torch.ones(N, Gn, dtype=torch.uint8, device=DEV), \
        torch.rand(N, R, device=DEV)
    an, ihw, out = torch.zeros(R, 4, device=DEV), torch.ones(N, 2, device=DEV), torch.zeros(2 * N, R, dtype=torch.int64, device=DEV)
    args = lambda a, h, t: (mx.data_ptr(), lq.data_ptr(), gv.data_ptr(), Gn, keys.data_ptr(), N, R, 0.3, 0.7, a, h, t, out.data_ptr(), H._stream())   # noqa: E731
    for a, h, t in ((None, ihw.data_ptr(), 0.0), (an.data_ptr(), None, 8.0), (an.data_ptr(), ihw.data_ptr(), float("nan"))):
        with pytest.raises(RuntimeError, match=EARG):
            H.call("utv2_rpn_sample_keys_b", *args(a, h, t))
    # the old entry point is the new one at threshold -1 (null tables)
    o1, o2 = torch.full_like(out, 7), torch.full_like(out, 9)
    H.call("utv2_rpn_sample_keys", mx.data_ptr(), lq.data_ptr(), gv.data_ptr(), Gn, keys.data_ptr(), N, R, 0.3, 0.7, o1.data_ptr(), H._stream())
    H.call("utv2_rpn_sample_keys_b", mx.data_ptr(), lq.data_ptr(), gv.data_ptr(), Gn, keys.data_ptr(), N, R, 0.3, 0.7, None, None, -1.0, o2.data_ptr(),
           H._stream())
    assert torch.equal(o1, o2) and int((o1 >= 0).sum()) > 0


# ---- MODEL.RPN.BOUNDARY_THRESH --------------------------------------------------------------------------------------------------------------
def golden_rpn(gold, thresh, *over):
    from ubteacher.modeling.fcos import PaddedBoxes
    from ubteacher.modeling.rcnn import PseudoLabRPN
    from ubteacher.params import ParamStore
    from ubteacher.presets import get_config
    cfg = get_config("rcnn", 1, ["MODEL.DEVICE", DEV, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", int(gold["batch"]), "MODEL.RPN.POSITIVE_FRACTION",
                                 float(gold["frac"]), "MODEL.RPN.BOUNDARY_THRESH", int(thresh)] + list(over))
    rpn = PseudoLabRPN(cfg, ParamStore(), 256)
    gb, gv, gs = torch.zeros(2, 4, 4), torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(2, 4)
    gb[0, :3], gv[0, :3], gs[0, :3] = T(gold["gt0"]).float(), 1, T(gold["sc0"]).float()
    sizes = [tuple(int(v) for v in s) for s in gold["sizes"]]
    gt = PaddedBoxes(sizes, boxes=gb.to(DEV), scores=gs.to(DEV), valid=gv.to(DEV), classes=torch.zeros(2, 4, dtype=torch.int32, device=DEV))
    rpn.sample_keys = T(gold["keys"]).float().to(DEV)
    return rpn, gt, sizes


@pytest.mark.parametrize("ti", [0, 1, 2])
def test_boundary_labels_and_samples_equal_the_executed_reference(gold, ti, monkeypatch):
    """fused (utv2_rpn_sample_keys_b) and ATen sampler paths: the indices the reference's labels give under the same keys, exactly"""
    t = float(gold["thresholds"][ti])
    rpn, gt, sizes = golden_rpn(gold, t)
    anchors = T(gold["anchors"]).float().to(DEV)
    want = R64.sample(T(gold["labels_t%d" % ti]), T(gold["keys"]).float(), int(gold["batch"]), float(gold["frac"]))
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("UTV2_FUSED_SAMPLERS", fused)
        s = rpn.label_and_sample(anchors, gt, sizes)
        got[fused] = s
        for k in ("pos", "neg"):
            v = s[k + "_valid"].bool().cpu()
            assert torch.equal(v, want[k + "_valid"].bool()), (fused, k)
            assert torch.equal(s[k + "_idx"].cpu()[v], want[k + "_idx"][v]), (fused, k)
        lab = torch.full((2, anchors.shape[0]), -1, dtype=torch.int8)
        for n in range(2):
            lab[n, s["pos_idx"][n].cpu()[s["pos_valid"][n].bool().cpu()]] = 1
            lab[n, s["neg_idx"][n].cpu()[s["neg_valid"][n].bool().cpu()]] = 0
        assert np.array_equal(lab.numpy(), gold["sampled_t%d" % ti])
    assert int(want["pos_valid"].sum()) == (2 if t == 0.0 else 3)          # the low-quality match outside the image is ignored at 0
    if t >= 0:
        with pytest.raises(ValueError, match="BOUNDARY_THRESH"):
            rpn.label_and_sample(anchors, gt)


@pytest.mark.parametrize("typ,bi", [("smooth_l1", 1), ("smooth_l1", 2), ("giou", 0)])
def test_rpn_losses_vs_reference_golden(gold, typ, bi):
    """config -> PseudoLabRPN.losses -> autograd node -> kernel against the executed reference, at the bounds of
    tests/test_rcnn_kernels_gpu.py::test_rpn_pseudo_losses_vs_reference_golden"""
    from tests.test_rcnn_percls_gpu import close
    rpn, gt, sizes = golden_rpn(gold, -1, "MODEL.RPN.BBOX_REG_LOSS_TYPE", typ, "MODEL.RPN.SMOOTH_L1_BETA", float(gold["betas"][bi]))
    obj = T(gold["obj"]).float().to(DEV).requires_grad_(True)
    dl = T(gold["deltas"]).float().to(DEV).requires_grad_(True)
    ls = rpn.losses(T(gold["anchors"]).float().to(DEV), obj, dl, gt)
    q = "%s_b%d" % (typ, bi)
    close(ls["loss_rpn_cls"], gold[q + "_loss_cls"], rtol=2e-5); close(ls["loss_rpn_loc"], gold[q + "_loss_loc"], rtol=2e-5)
    (ls["loss_rpn_cls"] + ls["loss_rpn_loc"]).backward()
    close(obj.grad, gold[q + "_gobj"], rtol=1e-4, atol=1e-8); close(dl.grad, gold[q + "_gdeltas"], rtol=1e-4, atol=1e-8)


# ---- anchors and head at A = 6 ----------------------------------------------------------------------------------------------------------------
def test_generated_anchors_equal_the_golden_tables(gold):
    from ubteacher.modeling.rcnn import AnchorGenerator
    from ubteacher.presets import get_config
    lv = [(8, 6), (4, 3)]
    for name, sizes, ratios, off in (("a6", [[32, 64]], [[0.5, 1.0, 2.0]], 0.0), ("a1", [[32], [64]], [[1.0]], 0.0),
                                     ("off", [[32], [64]], [[0.5, 1.0, 2.0]], 0.5)):
        cfg = get_config("rcnn", 1, ["MODEL.DEVICE", DEV, "MODEL.ANCHOR_GENERATOR.SIZES", sizes, "MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS", ratios,
                                     "MODEL.ANCHOR_GENERATOR.OFFSET", off])
        for l, p in enumerate(AnchorGenerator(cfg, [16, 32])(lv, torch.device(DEV))):
            assert p.is_cuda and np.array_equal(p.cpu().numpy(), gold["anc_%s_l%d" % (name, l)])


def test_rpn_at_six_anchors_per_cell(tmp_path):
    """A = 6 on a 2-level 8 x 6 / 4 x 3 pyramid, N = 2: the fused proposal chain against the ATen path, the loss against the fp64
    restatement on the RPN's own sample, the exported state dict in Detectron2's shapes through a checkpoint file"""
    from ubteacher import ops
    from ubteacher.modeling.fcos import PaddedBoxes
    from ubteacher.modeling.rcnn import PseudoLabRPN
    from ubteacher.params import ParamStore
    from ubteacher.presets import get_config
    cfg = get_config("rcnn", 1, ["MODEL.DEVICE", DEV, "MODEL.RPN.IN_FEATURES", ["p4", "p5"], "MODEL.ANCHOR_GENERATOR.SIZES", [[32, 64]],
                                 "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 32, "MODEL.RPN.SMOOTH_L1_BETA", 0.11])
    torch.manual_seed(0)
    store = ParamStore()
    rpn = PseudoLabRPN(cfg, store, 256)
    A, C, N, hw = 6, 256, 2, [(8, 6), (4, 3)]
    assert rpn.A == A and rpn.ch == 32 and rpn.strides == [16, 32]
    sizes = [(128, 96), (120, 90)]
    meta = ops.LevelMeta(N, hw)
    g = torch.Generator(device=DEV).manual_seed(5)
    big = torch.zeros(meta.P, rpn.ch, device=DEV)
    big[:, :5 * A] = torch.randn(meta.P, 5 * A, device=DEV, generator=g)
    anchors = rpn.anchor_generator(hw, big.device)
    R = sum(a.shape[0] for a in anchors)
    assert R == (48 + 12) * A
    # proposals: rank_keys + topk_rows + decode against predict_proposals
    rpn.train(False)
    sel = rpn._pre_nms_topk(big, N, hw)
    assert sel is not None
    pf = rpn._proposals_fused(big, anchors, sel, hw, N, sizes)
    obj, dl = rpn._per_image_views(big, N, hw)
    pa = rpn.predict_proposals(anchors, obj, dl, sizes)
    assert torch.equal(pf["count"], pa["count"]) and int(pf["count"].min()) > 0
    assert torch.equal(pf["valid"], pa["valid"]) and torch.equal(pf["boxes"], pa["boxes"])
    assert torch.equal(pf["objectness_logits"], pa["objectness_logits"])
    rpn.train(True)
    # loss on the head output against the restatement on the RPN's own sample
    gb = torch.zeros(N, 4, 4, device=DEV); gv = torch.zeros(N, 4, dtype=torch.uint8, device=DEV)
    gb[0, :2] = torch.tensor([[10., 12., 70., 60.], [40., 50., 90., 120.]], device=DEV); gv[0, :2] = 1
    gb[1, :1] = torch.tensor([[8., 30., 60., 100.]], device=DEV); gv[1, :1] = 1
    gt = PaddedBoxes(sizes, boxes=gb, valid=gv, classes=torch.zeros(N, 4, dtype=torch.int32, device=DEV))
    rpn.sample_keys = torch.rand(N, R, device=DEV, generator=g)
    acat = torch.cat(anchors)
    ba = big.clone().requires_grad_(True)
    la = rpn.losses(acat, ba, None, gt, head_hw=hw)
    s = {k: v.cpu() for k, v in rpn._last_sample.items()}
    assert int(s["pos_valid"].sum()) >= 3
    idx = torch.cat((s["pos_idx"], s["neg_idx"]), dim=1)
    ob, de = torch.cat(obj, 1).cpu().double(), torch.cat(dl, 1).cpu().double()
    x = torch.gather(ob, 1, idx)
    d = torch.gather(de, 1, s["pos_idx"][..., None].expand(-1, -1, 4))
    cls, loc, _, _, _ = R64.rpn_loss(x, d, acat.cpu().double(), s, gb.cpu().double(), None, rpn.box_weights, 0, f32(0.11))
    norm = 32.0 * N
    S = idx.shape[1]
    for k, terms, Lc in (("loss_rpn_cls", cls, math.ceil(N * S / 256)), ("loss_rpn_loc", loc, 4 * math.ceil(N * S / 256))):
        ref, bound = L64.sum_bound(terms, Lc, 8, 2)
        print("A6 %s k %.9g ref %.9g bound %.3g" % (k, float(la[k].detach()), ref / norm, (bound + L64.U * abs(ref)) / norm))
        assert abs(float(la[k].detach()) - ref / norm) <= (bound + L64.U * abs(ref)) / norm       # (+ the division's own rounding)
    (la["loss_rpn_cls"] + la["loss_rpn_loc"]).backward()
    assert torch.all(ba.grad[:, 5 * A:] == 0) and float(ba.grad[:, :A].abs().sum()) > 0 and float(ba.grad[:, A:5 * A].abs().sum()) > 0
    # checkpoint: Detectron2's shapes, and a round trip
    store.finalize(DEV)
    sd = store.state_dict()
    pre = "proposal_generator.rpn_head."
    assert tuple(sd[pre + "objectness_logits.weight"].shape) == (A, C, 1, 1) and tuple(sd[pre + "anchor_deltas.weight"].shape) == (4 * A, C, 1, 1)
    assert tuple(sd[pre + "objectness_logits.bias"].shape) == (A,) and tuple(sd[pre + "anchor_deltas.bias"].shape) == (4 * A,)
    path = os.path.join(str(tmp_path), "rpn_a6.pth")
    torch.save({k: v.cpu() for k, v in sd.items()}, path)
    store2 = ParamStore()
    PseudoLabRPN(cfg, store2, 256)
    store2.finalize(DEV)
    assert not torch.equal(store2.state_dict()[pre + "anchor_deltas.weight"], sd[pre + "anchor_deltas.weight"])      # its own random init
    store2.load_state_dict(torch.load(path))
    sd2 = store2.state_dict()
    for k, v in sd.items():
        assert torch.equal(v.cpu(), sd2[k].cpu()), k
    assert float(sd[pre + "anchor_deltas.weight"].abs().sum()) > 0 and float(sd[pre + "objectness_logits.weight"].abs().sum()) > 0


# ---- one small Faster-RCNN step per key -------------------------------------------------------------------------------------------------------
KEYS = {"beta": ["MODEL.RPN.SMOOTH_L1_BETA", 0.11], "giou": ["MODEL.RPN.BBOX_REG_LOSS_TYPE", "giou"], "thresh": ["MODEL.RPN.BOUNDARY_THRESH", 0],
        "a6": ["MODEL.ANCHOR_GENERATOR.SIZES", [[32, 64], [64, 128], [128, 256], [256, 512], [512, 640]]]}


@pytest.mark.parametrize("key", sorted(KEYS))
def test_small_step_honours_the_key_with_both_loss_tails(key, monkeypatch):
    """One 2 + 2 step at 96 x 128 (tests/test_roi_box_beta_gpu.py::small_step): the fused scalar tail and the ATen tail agree on every loss
    to its 1e-5, every loss is finite, and the labeled branch's location sum equals the fp64 restatement on the step's own sample."""
    from tests import test_roi_box_beta_gpu as B
    from ubteacher.modeling.rcnn import PseudoLabRPN
    seen = []
    orig = PseudoLabRPN.losses

    def spy(self, anchors, obj, deltas, gt, **kw):
        out = orig(self, anchors, obj, deltas, gt, **kw)
        if kw.get("img0", 0) == 0 and not seen and self.training:
            seen.append((self, anchors.detach().cpu(), obj.detach().cpu(), gt["boxes"].cpu(), kw, {k: v.cpu() for k, v in self._last_sample.items()}, out))
        return out
    monkeypatch.setattr(PseudoLabRPN, "losses", spy)
    monkeypatch.setattr(B, "_TUNED", {})                  # (a6 has its own head shape: no tuned state is shared between the keys)
    if key == "a6":
        # the helper's head tuning knows three anchors per cell: tune those, then give the second size of every cell a scaled copy
        from tests import utv2_testutil as U
        tune3, q = U.rcnn_tune, "proposal_generator.rpn_head."

        def tune6(sd, *a, **k):
            sd = dict(sd)
            sd[q + "objectness_logits.bias"], sd[q + "anchor_deltas.bias"] = torch.zeros(3), torch.zeros(12)
            out = tune3(sd, *a, **k)
            out[q + "objectness_logits.weight"] = torch.cat((out[q + "objectness_logits.weight"], out[q + "objectness_logits.weight"] * 0.75))
            out[q + "anchor_deltas.weight"] = torch.cat((out[q + "anchor_deltas.weight"], out[q + "anchor_deltas.weight"] * 0.75))
            out[q + "objectness_logits.bias"], out[q + "anchor_deltas.bias"] = torch.zeros(6), torch.zeros(24)
            return out
        monkeypatch.setattr(U, "rcnn_tune", tune6)
    ra = B.small_step(KEYS[key], True, monkeypatch)
    first = list(seen)
    rb = B.small_step(KEYS[key], False, monkeypatch)
    for k in rb:
        if k.startswith("loss") or k == "total_loss":
            print("STEP %s %s fused %.9g aten %.9g" % (key, k, ra[k], rb[k]))
            assert math.isfinite(ra[k]) and abs(ra[k] - rb[k]) <= 1e-5 * max(abs(rb[k]), 1e-6), (k, ra[k], rb[k])
    rpn, acat, big, gb, kw, s, out = first[0]
    assert kw.get("raw") and rpn.ch == (32 if key == "a6" else 16)
    N, hw = gb.shape[0], kw["head_hw"]
    obj, dl = rpn._per_image_views(big, kw["batch"], hw)
    ob, de = torch.cat(obj, 1)[:N].double(), torch.cat(dl, 1)[:N].double()
    idx = torch.cat((s["pos_idx"], s["neg_idx"]), dim=1)
    x = torch.where(torch.cat((s["pos_valid"], s["neg_valid"]), dim=1).bool(), torch.gather(ob, 1, idx), torch.zeros((), dtype=F64))
    d = torch.gather(de, 1, s["pos_idx"][..., None].expand(-1, -1, 4))
    d = torch.where((s["pos_valid"].bool() & s["has_gt"].bool())[..., None], d, torch.zeros((), dtype=F64))
    _, loc, _, _, _ = R64.rpn_loss(x, d, acat.double(), s, gb.double(), None, rpn.box_weights, rpn.loc_mode, f32(rpn.smooth_l1_beta))
    ref, bound = L64.sum_bound(loc, 4 * math.ceil(N * idx.shape[1] / 256), 8, M_NEW[(rpn.loc_mode, 0.0)] if rpn.loc_mode else 2)
    k = float(out["raw_sums"].detach()[1])
    print("STEP %s loc sum k %.9g ref %.9g bound %.3g npos %d" % (key, k, ref, bound, int(s["pos_valid"].sum())))
    assert int(s["pos_valid"].sum()) > 0 and abs(k - ref) <= bound
