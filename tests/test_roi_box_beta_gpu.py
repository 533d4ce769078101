"""MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE "giou" on the GPU: utv2_roi_box_loss_f (csrc/rcnn.hip) in every mode x beta
against fp64 autograd (tests/loss_ref64_roi_beta.py) on rows that sit on the branch points, both box layouts against each other bit for
bit, the old entry point against the new one at beta 0, the refused arguments, the two boundary-variance predictors against the executed
reference (tests/golden/roi_beta.npz), and one small Faster-RCNN step per key with the fused loss tail and with the ATen tail.

Bounds: those of this kernel's modes 0-3 in tests/test_loss_kernels_fp64_gpu.py (M_ROI = 16, the sum at L = 5 ceil(R / 256), D = 8) and of
tests/test_rcnn_percls_gpu.py::test_predictor_losses_vs_reference_golden (loss 2e-5, gradients 1e-4 + 2e-7) - none of its own."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_percls as P64
from tests import loss_ref64_roi_beta as B64
from tests.test_loss_kernels_fp64_gpu import M_ROI, check_grad, check_sum, same_bits
from tests.test_rcnn_percls_gpu import close

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
EARG = "failed with code -1000"
BETAS = [0.0, 0.11, 1.0]
F32 = lambda b: float(torch.tensor(b, dtype=torch.float32))   # noqa: E731  (the beta the kernel receives: the reference gets the same number)


def T(a):
    return torch.from_numpy(np.asarray(a))


def raw(H, name, de, st, cls, prop, gtb, K, nbox, mode, beta=None, R=None, gstd=None):
    """the C entry point `name` on output buffers pre-filled with NaN: every element must be written by the launch itself"""
    R = de.shape[0] if R is None else R
    out = torch.full((1,), float("nan"), device=DEV)
    gd = torch.full((max(R, 1), 4 * nbox), float("nan"), device=DEV)
    gs = torch.full((max(R, 1), 4 * nbox), float("nan"), device=DEV)
    wx, wy = L64.ROI_W
    tail = (out.data_ptr(), gd.data_ptr(), gs.data_ptr(), H._stream())
    H.call(name, de.data_ptr(), st.data_ptr(), de.stride(0), cls.data_ptr(), prop.data_ptr(), gtb.data_ptr(),
           None if gstd is None else gstd.data_ptr(), R, K, nbox, mode, wx, wy, L64.ROI_CLAMP, 0.1, 0.5, *(() if beta is None else (beta,)), *tail)
    return out, gd, gs


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("mode", [0, 1, 3, 4])
@pytest.mark.parametrize("K,R", [(3, 48), (80, 64)])
def test_roi_box_loss_f_vs_fp64_and_layout_equality(K, R, mode, beta):
    """Per-class (nbox = K) on the full matrix: the sum and both gradient tensors against fp64 autograd; every unselected element exactly
    0.0 (the buffers start as NaN); gstd_out all zero outside mode 0; and nbox = 1 on the gathered columns gives the same bits."""
    from ubteacher import hip as H
    beta = F32(beta)
    c = B64.branch_case(R, K, 700 + K, beta if beta else F32(0.11))
    fgm = (c["cls"] >= 0) & (c["cls"] < K)
    assert {-1, 0, K - 1, K} <= set(c["cls"].tolist()) and int(fgm[:12].sum()) == 12
    wx, wy = L64.ROI_W
    a = (c["cls"], c["prop"], c["gtb"], K, mode, wx, wy, L64.ROI_CLAMP, beta)
    l64, gd64, gs64 = B64.roi_box_loss_pc(c["deltas"].double(), c["std"].double(), *a)
    _, gd32, gs32 = B64.roi_box_loss_pc(c["deltas"], c["std"], *a)
    if beta and mode != 4:                                   # the case does sit on the branch point: |d - t| == beta bit for bit on row 0
        d0 = torch.gather(c["deltas"], 1, c["col"])[0] - c["t"][0]
        assert (d0.abs() == beta).any() and ((d0.abs() < beta) & (d0 != 0)).any() and (torch.gather(c["deltas"], 1, c["col"])[5] - c["t"][5]).abs().max() > beta
    de, st, cls, prop, gtb = (c[k].to(DEV) for k in ("deltas", "std", "cls", "prop", "gtb"))
    o1 = raw(H, "utv2_roi_box_loss_f", de, st, cls, prop, gtb, K, K, mode, beta)
    o2 = H.roi_box_loss(de, st, cls, prop, gtb, None, K, mode, wx, wy, L64.ROI_CLAMP, 0.1, 0.5, nbox=K, smooth_l1_beta=beta)
    for x1, x2 in zip(o1, o2):
        assert same_bits(x1, x2)
    tag = "roi_f m%d K%d b%g" % (mode, K, beta)
    check_sum(tag, o1[0].cpu()[0], l64, 5 * math.ceil(R / 256), 8, M_ROI)
    check_grad(tag + " gd", o1[1], gd64, gd32, M_ROI)
    check_grad(tag + " gs", o1[2], gs64, gs32, M_ROI)
    sel = torch.zeros(R, 4 * K, dtype=torch.bool).scatter_(1, c["col"], fgm[:, None].expand(R, 4))
    for gk in (o1[1].cpu(), o1[2].cpu()):
        assert torch.all(gk[~sel] == 0.0) and not torch.isnan(gk).any()
    if mode != 0:
        assert torch.all(o1[2].cpu() == 0.0)               # "giou" too: the std head gets no gradient from it
    col = c["col"].to(DEV)
    ag = H.roi_box_loss(torch.gather(de, 1, col).contiguous(), torch.gather(st, 1, col).contiguous(), cls, prop, gtb, None, K, mode, wx, wy,
                        L64.ROI_CLAMP, 0.1, 0.5, smooth_l1_beta=beta)
    assert same_bits(ag[0], o1[0])
    fg = fgm.to(DEV)
    for a_, p_ in ((ag[1], torch.gather(o1[1], 1, col)), (ag[2], torch.gather(o1[2], 1, col))):
        assert same_bits(a_[fg], p_[fg])
        assert torch.all(a_[~fg] == 0.0) and torch.all(p_[~fg] == 0.0)


def test_giou_known_answer_on_the_device():
    """tests/test_roi_box_beta.py::test_giou_known_answer_for_two_boxes through the kernel: loss 68/63, d / d delta_x1 = 0.2 * 103/441;
    the zero-area prediction inside its gt box: loss 1.  Inputs and the decode are exact in fp32; the quotients are a few roundings."""
    from ubteacher import hip as H
    box = torch.tensor([[0.0, 0.0, 2.0, 2.0], [0.0, 0.0, 2.0, 2.0]], device=DEV)
    de = torch.tensor([[5.0, 5.0, 2.5, 2.5], [5.0, -5.0, 0.0, 0.0]], device=DEV)
    cls = torch.tensor([1, 0], device=DEV)
    u = 2.0 ** -24
    for r, want in ((0, 68.0 / 63.0), (1, 1.0)):
        out, gd, gs = H.roi_box_loss(de[r:r + 1], de[r:r + 1], cls[r:r + 1], box[r:r + 1], box[r:r + 1], None, 3, 4, 10.0, 5.0, L64.ROI_CLAMP, 0.0, 0.0)
        assert abs(float(out[0]) - want) <= 8 * u * want + 1e-7       # (fvcore's eps 1e-7 in both denominators)
        assert torch.all(gs == 0)
        if r == 0:
            assert abs(float(gd[0, 0]) - 0.2 * 103.0 / 441.0) <= 16 * u * 0.2 * 103.0 / 441.0 + 1e-7


@pytest.mark.parametrize("mode,nbox_k", [(0, False), (1, False), (2, False), (3, False), (0, True), (1, True), (3, True)])
def test_old_entry_point_is_the_new_one_at_beta_zero(mode, nbox_k):
    """(tsbetter, mode 2, has no per-class form: refused by both entry points, see the arguments test)"""
    from ubteacher import hip as H
    K, R = 3, 300                                          # more than one trip of the 256-thread row loop
    c = P64.percls_case(R, K, 41)
    gstd = torch.tensor([0.0, -3.0, 3.0, -8.0])[torch.randint(0, 4, (R, 4), generator=torch.Generator().manual_seed(3))].to(DEV)
    de, st, cls, prop, gtb = (c[k].to(DEV) for k in ("deltas", "std", "cls", "prop", "gtb"))
    if not nbox_k:
        de, st = de[:, :4].contiguous(), st[:, :4].contiguous()
    nbox = K if nbox_k else 1
    old = raw(H, "utv2_roi_box_loss", de, st, cls, prop, gtb, K, nbox, mode, gstd=gstd)
    new = raw(H, "utv2_roi_box_loss_f", de, st, cls, prop, gtb, K, nbox, mode, 0.0, gstd=gstd)
    tiny = raw(H, "utv2_roi_box_loss_f", de, st, cls, prop, gtb, K, nbox, mode, 9e-6, gstd=gstd)      # below fvcore's 1e-5: still plain L1
    for x1, x2, x3 in zip(old, new, tiny):
        assert same_bits(x1, x2) and same_bits(x1, x3) and not torch.isnan(x1).any()
    assert float(old[0].cpu()[0]) > 0
    if mode == 2:                                           # the reference calls tsbetter's smooth-L1 at 0.0: beta has no effect
        b1 = raw(H, "utv2_roi_box_loss_f", de, st, cls, prop, gtb, K, nbox, mode, 1.0, gstd=gstd)
        for x1, x2 in zip(old, b1):
            assert same_bits(x1, x2)


def test_roi_box_loss_f_arguments():
    from ubteacher import hip as H
    K, R = 3, 5
    c = P64.percls_case(R, K, 31)
    de, st, cls, prop, gtb = (c[k].to(DEV) for k in ("deltas", "std", "cls", "prop", "gtb"))
    f = "utv2_roi_box_loss_f"
    for mode in (0, 1, 3, 4):
        out, _, _ = raw(H, f, de, st, cls, prop, gtb, K, K, mode, 0.11, R=0)
        assert float(out.cpu()[0]) == 0.0                                    # R == 0: sum 0
    for bad in (dict(mode=5, beta=0.0), dict(mode=-1, beta=0.0), dict(mode=1, beta=-0.5), dict(mode=4, beta=-1e-9),
                dict(mode=1, beta=float("nan")), dict(mode=2, beta=0.0)):   # the last: tsbetter with nbox = K
        with pytest.raises(RuntimeError, match=EARG):
            raw(H, f, de, st, cls, prop, gtb, K, K, bad["mode"], bad["beta"])
    with pytest.raises(RuntimeError, match=EARG):
        raw(H, "utv2_roi_box_loss", de, st, cls, prop, gtb, K, K, 4)         # the old entry point keeps its modes 0..3
    with pytest.raises(RuntimeError, match=EARG):
        H.roi_box_loss(de, st, cls, prop, gtb, None, K, 5, 10.0, 5.0, L64.ROI_CLAMP, 0.0, 0.0, nbox=K)
    raw(H, f, de[:, :4].contiguous(), st[:, :4].contiguous(), cls, prop, gtb, K, 1, 2, 0.0)      # tsbetter, class-agnostic: accepted


# ---- the predictors against the executed reference ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "roi_beta.npz")))


TYPES = {"smooth_l1": ("supervised", "smooth_l1"), "nlloss": ("supervised", "nlloss"), "giou": ("supervised", "giou"),
         "pseudo": ("unsup_data_train", "nlloss")}


@pytest.mark.parametrize("bi", [0, 1, 2])
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("lay", ["agn", "pc"])
@pytest.mark.parametrize("pred_kind", ["focal", "ce"])
def test_predictor_box_loss_vs_reference_golden(gold, pred_kind, lay, typ, bi):
    """config -> predictor -> autograd node -> kernel: loss_box_reg and its gradients w.r.t. the deltas and the std logits, and the raw sum
    the fused scalar tail (utv2_rcnn_loss_combine) is handed: the same number before the division"""
    from ubteacher.modeling import rcnn as R_
    from ubteacher.params import ParamStore
    from ubteacher.presets import get_config
    K = 3
    branch, sup_type = TYPES[typ]
    beta = float(gold["betas"][bi])
    cfg = get_config("rcnn", 1, ["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.NUM_CLASSES", K, "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", lay == "agn",
                                 "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "smooth_l1", "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", sup_type,
                                 "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", beta])
    klass = R_.FastRCNNCrossEntropyBoundaryVarOutputLayers if pred_kind == "ce" else R_.FastRCNNFocaltLossBoundaryVarOutputLayers
    pred = klass(cfg, ParamStore(), 1024, "roi_heads.box_predictor")
    assert tuple(pred.box2box_transform.weights[:2]) == (10.0, 10.0)
    ncol = 4 if lay == "agn" else 4 * K
    cls = T(gold["cls"]).long()
    R = cls.shape[0]
    scores = torch.zeros(R, K + 1, device=DEV)
    deltas, std = (T(gold[k])[:, :ncol].float().contiguous().to(DEV).requires_grad_(True) for k in ("deltas", "std"))
    sampled = dict(gt_classes=cls.to(DEV)[None], proposal_boxes=T(gold["prop"]).float().to(DEV)[None], gt_boxes=T(gold["gtb"]).float().to(DEV)[None])
    ls = pred.losses((scores, deltas, std), sampled, branch)
    q = "%s_%s_%s_b%d" % (pred_kind, lay, typ, bi)
    close(ls["loss_box_reg"], gold[q + "_loss"], rtol=2e-5)
    ls["loss_box_reg"].backward()
    for k, v in (("deltas", deltas), ("std", std)):
        gv = v.grad if v.grad is not None else torch.zeros_like(v)
        close(gv, gold[q + "_g" + k], rtol=1e-4, atol=2e-7)
        assert float(gv[cls.to(DEV) < 0].abs().max()) == 0.0
    rawd = pred.losses((scores, deltas.detach(), std.detach()), sampled, branch, raw=True)
    n = int((cls >= 0).sum())
    close(rawd["box"][0] / n, gold[q + "_loss"], rtol=2e-5)
    assert int((rawd["tgt"] >= 0).sum()) == n


# ---- one small Faster-RCNN step per key ------------------------------------------------------------------------------------------------
_TUNED = {}


def small_step(over, fuse_tail, monkeypatch):
    """one 2 + 2 image semi-supervised step at 96 x 128 like tests/test_rcnn_step_gpu.py's (tuned heads, fixed sampling keys) -> metrics"""
    from tests.utv2_testutil import FixedLoader, cpu_state, make_batch, rcnn_tune
    from ubteacher.engine import UBRCNNTeacherTrainer
    from ubteacher.presets import get_config
    monkeypatch.setenv("UTV2_FUSE_LOSS_TAIL", "1" if fuse_tail else "0")       # read by every run_step
    cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "MODEL.DEVICE", DEV] + list(over))
    torch.manual_seed(0)
    prod, orac = make_batch(31, 2, 2, 96, 128, DEV)
    tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    if "s" not in _TUNED:                                                      # the keys change no parameter: one tuned state for all
        mean, pstd = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1), torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
        _TUNED["s"] = rcnn_tune(cpu_state(tr.model), [d["image"] for d in orac[3]], mean, pstd)
    sd_s = _TUNED["s"]
    sd_t = dict(sd_s)
    sd_t["roi_heads.box_predictor.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    src = lambda n, m, device: torch.rand(n, m, generator=torch.Generator().manual_seed(1000 * n + m)).to(device)   # noqa: E731
    tr.model.proposal_generator.sample_keys = src
    tr.model.roi_heads.sample_keys = src
    seen = []
    orig = tr.model.forward_joint_begin
    tr.model.forward_joint_begin = lambda *a, **k: (seen.append(k.get("loss_weights") is not None), orig(*a, **k))[1]
    tr.run_step_full_semisup()
    torch.cuda.synchronize()
    assert seen == [fuse_tail]                                                 # the fused student pass ran, with / without the fused tail
    rec = tr.flush_metrics()
    assert all(torch.isfinite(v).all() for v in cpu_state(tr.model).values())
    return rec


@pytest.fixture(scope="module")
def baseline_step():
    mp = pytest.MonkeyPatch()
    try:
        return small_step([], True, mp)                                        # the shipped keys: "nlloss", beta 0
    finally:
        mp.undo()


@pytest.mark.parametrize("key", ["giou", "beta"])
def test_small_step_honours_the_key_with_both_loss_tails(key, baseline_step, monkeypatch):
    """The fused scalar tail and the ATen tail agree on every loss to the 1e-5 of
    tests/test_rcnn_step_gpu.py::test_rcnn_fused_student_pass_equals_two_passes, and loss_box_reg is NOT the value of the shipped keys:
    before this, SMOOTH_L1_BETA was stored and ignored (the same number came out) and "giou" did not build."""
    over = ["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou"] if key == "giou" else ["MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", 0.11]
    ra, rb = small_step(over, True, monkeypatch), small_step(over, False, monkeypatch)
    for k in rb:
        if k.startswith("loss") or k == "total_loss":
            print("STEP %s %s fused %.9g aten %.9g shipped %.9g" % (key, k, ra[k], rb[k], baseline_step.get(k, float("nan"))))
    for k in rb:
        if k.startswith("loss") or k == "total_loss":
            assert abs(ra[k] - rb[k]) <= 1e-5 * max(abs(rb[k]), 1e-6), (k, ra[k], rb[k])
    base = baseline_step["loss_box_reg"]
    assert rb["loss_box_reg"] > 0 and base > 0
    assert abs(ra["loss_box_reg"] - base) > 1e-3 * base, (ra["loss_box_reg"], base)
    for k in ("loss_cls", "loss_rpn_cls", "loss_rpn_loc"):                     # the forward pass is the same one: only the box loss moved
        assert abs(ra[k] - baseline_step[k]) <= 1e-5 * max(abs(baseline_step[k]), 1e-6), (k, ra[k], baseline_step[k])
