"""Per-class box regression of the boundary-variance ROI predictor (MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False) on the GPU: the
utv2_roi_box_loss kernel with nbox = K against fp64 autograd (tests/loss_ref64_percls.py) and against itself with nbox = 1 on the
pre-gathered columns, the predictor's losses / head gradients / inference against the executed reference (tests/golden/rcnn_percls.npz), the fused
inference kernels against the ATen chain, and whole semi-supervised steps (fp16 AMP, hipGraph replay)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref64 as L64
from tests import loss_ref64_percls as P64
from tests.test_loss_kernels_fp64_gpu import M_ROI, check_grad, check_sum, same_bits

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
PC = ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "smooth_l1"]
EARG = "failed with code"


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(a, b, rtol=1e-5, atol=1e-6):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    a, b = a.astype(np.float64), b.astype(np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (float(np.abs(a - b).max()), float(np.abs(b).max()))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "rcnn_percls.npz")))


def cfg_of(K=80, *over):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.NUM_CLASSES", K] + PC + list(over))


def raw_loss_pc(H, de, st, cls, prop, gtb, K, nbox, mode, ld=None, R=None):
    """utv2_roi_box_loss (gstd null) on output buffers pre-filled with NaN: every element must be written by the launch itself"""
    R = de.shape[0] if R is None else R
    out = torch.full((1,), float("nan"), device=DEV)
    gd = torch.full((max(R, 1), 4 * nbox), float("nan"), device=DEV)
    gs = torch.full((max(R, 1), 4 * nbox), float("nan"), device=DEV)
    wx, wy = L64.ROI_W
    H.call("utv2_roi_box_loss", de.data_ptr(), st.data_ptr(), de.stride(0) if ld is None else ld, cls.data_ptr(), prop.data_ptr(),
           gtb.data_ptr(), None, R, K, nbox, mode, wx, wy, L64.ROI_CLAMP, 0.0, 0.0, out.data_ptr(), gd.data_ptr(), gs.data_ptr(), H._stream())
    return out, gd, gs


@pytest.mark.parametrize("pitch", ["packed", "wide"])
@pytest.mark.parametrize("K", [3, 80])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_roi_box_loss_pc_vs_fp64_and_vs_the_agnostic_kernel(mode, K, pitch):
    """R = 37 rows (no multiple of a wave).  Bound: the ROI box loss's of test_loss_kernels_fp64_gpu.py (M (max(|r32 - r64|, u |r64|) + u s),
    M = 16, no absolute tolerance; the sum: (L + D + 2 M) u sum |terms|, L = 5 ceil(R / 256), D = 8).  Outside the selected columns every
    gradient element is exactly 0.0 (the buffers start as NaN).  nbox = 1 on the pre-gathered columns gives the same bits - the sum, and
    the gradients of every foreground row: the reduction order is fixed and the row body is the same - the check of the column selection."""
    from ubteacher import hip as H
    R = 37
    c = P64.percls_case(R, K, 900 + K)
    assert {-1, 0, K - 1, K} <= set(c["cls"].tolist())
    wx, wy = L64.ROI_W
    a = (c["cls"], c["prop"], c["gtb"], K, mode, wx, wy, L64.ROI_CLAMP)
    l64, gd64, gs64 = P64.roi_box_loss_pc(c["deltas"].double(), c["std"].double(), *a)
    _, gd32, gs32 = P64.roi_box_loss_pc(c["deltas"], c["std"], *a)
    if pitch == "packed":
        de, st = c["deltas"].to(DEV), c["std"].to(DEV)
        assert de.stride(0) == 4 * K
    else:                                              # column slices of one wider matrix, as the predictor's output is: odd offset, larger pitch
        m = torch.zeros(R, 8 * K + 5)
        m[:, 1:1 + 4 * K], m[:, 1 + 4 * K:1 + 8 * K] = c["deltas"], c["std"]
        m = m.to(DEV)
        de, st = m[:, 1:1 + 4 * K], m[:, 1 + 4 * K:1 + 8 * K]
        assert de.stride(0) == 8 * K + 5
    cls, prop, gtb = c["cls"].to(DEV), c["prop"].to(DEV), c["gtb"].to(DEV)
    o1 = raw_loss_pc(H, de, st, cls, prop, gtb, K, K, mode)
    o2 = H.roi_box_loss(de, st, cls, prop, gtb, None, K, mode, wx, wy, L64.ROI_CLAMP, 0.0, 0.0, nbox=K)
    for x1, x2 in zip(o1, o2):
        assert same_bits(x1, x2)
    tag = "roi_pc m%d K%d %s" % (mode, K, pitch)
    check_sum(tag, o1[0].cpu()[0], l64, 5 * math.ceil(R / 256), 8, M_ROI)
    check_grad(tag + " gd", o1[1], gd64, gd32, M_ROI)
    check_grad(tag + " gs", o1[2], gs64, gs32, M_ROI)
    sel = torch.zeros(R, 4 * K, dtype=torch.bool).scatter_(1, c["col"], ((c["cls"] >= 0) & (c["cls"] < K))[:, None].expand(R, 4))
    for gk in (o1[1].cpu(), o1[2].cpu()):
        assert torch.all(gk[~sel] == 0.0) and not torch.isnan(gk).any()
    if mode != 0:
        assert torch.all(o1[2].cpu() == 0.0)
    # nbox = 1 on the gathered four columns
    col = c["col"].to(DEV)
    ag = H.roi_box_loss(torch.gather(de, 1, col).contiguous(), torch.gather(st, 1, col).contiguous(), cls, prop, gtb, None, K, mode, wx, wy,
                        L64.ROI_CLAMP, 0.0, 0.0)
    assert same_bits(ag[0], o1[0])
    # the selected columns exist on foreground rows: same bits there.  A background / empty row has none - both layouts give zeros, the
    # class-agnostic one signed ones (-0.0 = sign(d - t) * 0), the per-class one the +0.0 its zero-filling workgroups write
    fg = ((c["cls"] >= 0) & (c["cls"] < K)).to(DEV)
    for a_, p_ in ((ag[1], torch.gather(o1[1], 1, col)), (ag[2], torch.gather(o1[2], 1, col))):
        assert same_bits(a_[fg], p_[fg])
        assert torch.all(a_[~fg] == 0.0) and torch.all(p_[~fg] == 0.0)


def test_roi_box_loss_pc_zero_fill_grid_stride():
    """R * K = 3300 * 80 = 264 000 groups of four > 1024 workgroups x 256 threads: the zero-filling workgroups take more than one group
    each (the 4 + 4 training step has 4096 x 80).  Outputs start as NaN: every element is written, the unselected ones 0.0, the selected
    ones with the bits of nbox = 1 on the gathered columns."""
    from ubteacher import hip as H
    R, K = 3300, 80
    assert R * K > 1024 * 256
    g = torch.Generator().manual_seed(5)
    cls = torch.randint(-1, K + 1, (R,), generator=g)
    cls[0], cls[R - 1], cls[R - 2] = K - 1, 0, K - 1
    xy = torch.rand(R, 2, generator=g) * 100
    prop = torch.cat((xy, xy + torch.rand(R, 2, generator=g) * 60 + 4), 1)
    gtb = prop + torch.randn(R, 4, generator=g) * 3
    de, st = torch.randn(R, 4 * K, generator=g).to(DEV), torch.randn(R, 4 * K, generator=g).to(DEV)
    cls, prop, gtb = cls.to(DEV), prop.to(DEV), gtb.to(DEV)
    out, gd, gs = raw_loss_pc(H, de, st, cls, prop, gtb, K, K, 0)
    fg = (cls >= 0) & (cls < K)
    col = P64.select_columns(cls.cpu(), K).to(DEV)
    sel = torch.zeros(R, 4 * K, dtype=torch.bool, device=DEV).scatter_(1, col, fg[:, None].expand(R, 4))
    assert int(fg.sum()) > 3000 and int((~fg).sum()) > 20
    for gk in (gd, gs):
        assert not torch.isnan(gk).any() and torch.all(gk[~sel] == 0.0)
    assert float(gd[sel].abs().min()) > 0.0             # an L1 derivative is +-1 plus the NLL term: never 0 on a selected element
    wx, wy = L64.ROI_W
    ag = H.roi_box_loss(torch.gather(de, 1, col).contiguous(), torch.gather(st, 1, col).contiguous(), cls, prop, gtb, None, K, 0, wx, wy,
                        L64.ROI_CLAMP, 0.0, 0.0)
    assert same_bits(ag[0], out)
    assert same_bits(ag[1][fg], torch.gather(gd, 1, col)[fg]) and same_bits(ag[2][fg], torch.gather(gs, 1, col)[fg])


def test_roi_box_loss_pc_arguments():
    from ubteacher import hip as H
    K, R = 3, 5
    c = P64.percls_case(R, K, 31)
    de, st, cls, prop, gtb = (c[k].to(DEV) for k in ("deltas", "std", "cls", "prop", "gtb"))
    out, _, _ = raw_loss_pc(H, de, st, cls, prop, gtb, K, K, 1, R=0)
    assert float(out.cpu()[0]) == 0.0                                        # R == 0: sum 0
    with pytest.raises(RuntimeError, match=EARG):
        raw_loss_pc(H, de, st, cls, prop, gtb, K, K, 2)                      # tsbetter has no per-class form
    with pytest.raises(RuntimeError, match=EARG):
        raw_loss_pc(H, de, st, cls, prop, gtb, K, 2, 1)                      # nbox is neither num_classes nor 1
    with pytest.raises(RuntimeError, match=EARG):
        raw_loss_pc(H, de, st, cls, prop, gtb, K, K, 1, ld=4 * K - 1)        # pitch below 4 * nbox
    with pytest.raises(RuntimeError, match=EARG):
        raw_loss_pc(H, de, st, cls, prop, gtb, K, K, 1, R=-1)
    # nbox == 1: the raw call and the wrapper's default
    o = raw_loss_pc(H, de[:, :4].contiguous(), st[:, :4].contiguous(), cls, prop, gtb, K, 1, 0)
    wx, wy = L64.ROI_W
    ag = H.roi_box_loss(de[:, :4].contiguous(), st[:, :4].contiguous(), cls, prop, gtb, None, K, 0, wx, wy, L64.ROI_CLAMP, 0.0, 0.0)
    for x1, x2 in zip(o, ag):
        assert same_bits(x1, x2)


MODES = {"sup_nlloss": ("supervised", "nlloss"), "sup_smooth_l1": ("supervised", "smooth_l1"), "pseudo_smooth_l1": ("unsup_data_train", "nlloss")}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("pred_kind", ["focal", "ce"])
@pytest.mark.parametrize("K", [80, 3])
def test_predictor_losses_vs_reference_golden(gold, K, pred_kind, mode):
    """the tolerances of tests/test_rcnn_kernels_gpu.py::test_predictor_losses_vs_reference_golden; the fixture's rows hold empty slots
    (cls -1: zero gradient), background, class 0, class K - 1 and an image without ground truth"""
    from ubteacher.modeling import rcnn as R_
    from ubteacher.params import ParamStore
    branch, sup_type = MODES[mode]
    klass = R_.FastRCNNCrossEntropyBoundaryVarOutputLayers if pred_kind == "ce" else R_.FastRCNNFocaltLossBoundaryVarOutputLayers
    pred = klass(cfg_of(K, "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", sup_type), ParamStore(), 1024, "roi_heads.box_predictor")
    p = "k%d_" % K
    cls = T(gold[p + "cls"]).long()
    scores, deltas, std = (T(gold[p + mode + "_" + k]).float().to(DEV).requires_grad_(True) for k in ("scores", "deltas", "std"))
    sampled = dict(gt_classes=cls.to(DEV)[None], proposal_boxes=T(gold[p + "prop"]).float().to(DEV)[None],
                   gt_boxes=T(gold[p + "gtb"]).float().to(DEV)[None])
    ls = pred.losses((scores, deltas, std), sampled, branch)
    q = p + pred_kind + "_" + mode
    close(ls["loss_cls"], gold[q + "_loss_cls"], rtol=2e-5)
    close(ls["loss_box_reg"], gold[q + "_loss_box_reg"], rtol=2e-5)
    (ls["loss_cls"] + 2.0 * ls["loss_box_reg"]).backward()
    for k, v in (("scores", scores), ("deltas", deltas), ("std", std)):
        gv = v.grad if v.grad is not None else torch.zeros_like(v)
        close(gv, gold[q + "_g" + k], rtol=1e-4, atol=2e-7)
        assert float(gv[cls.to(DEV) < 0].abs().max()) == 0.0
    raw = pred.losses((scores.detach(), deltas.detach(), std.detach()), sampled, branch, raw=True)       # the fused scalar tail's inputs
    n = int((cls >= 0).sum())
    close(raw["box"][0] / n, gold[q + "_loss_box_reg"], rtol=2e-5)
    assert int((raw["tgt"] >= 0).sum()) == n


@pytest.mark.parametrize("K", [3, 80])
def test_inference_fused_equals_aten_and_the_reference(gold, K, monkeypatch):
    """N = 2, P = 50: one proposal whose decoded box is NaN for a single class (the row goes, D2 filters rows) and one invalid slot, both
    with a confident score.  Fused kernels == ATen chain bit for bit; both == the executed reference under the existing golden's tolerance."""
    from ubteacher.modeling.fcos import PaddedBoxes
    from ubteacher.modeling.rcnn import FastRCNNFocaltLossBoundaryVarOutputLayers
    from ubteacher.params import ParamStore
    pred = FastRCNNFocaltLossBoundaryVarOutputLayers(cfg_of(K), ParamStore(), 1024, "roi_heads.box_predictor")
    p = "k%d_inf" % K
    sizes = [tuple(int(x) for x in s) for s in gold[p + "_sizes"]]
    props = PaddedBoxes(sizes, boxes=T(gold[p + "_prop"]).float().to(DEV), valid=T(gold[p + "_valid"]).to(DEV))
    preds = tuple(T(gold[p + "_" + k]).float().to(DEV) for k in ("scores", "deltas", "std"))
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("UTV2_FUSED_ROI_INFERENCE", fused)
        outs.append(pred.inference(preds, props))
    (da, ra), (db, rb) = outs
    assert tuple(da["pred_boxes_std"].shape) == (2, pred.test_topk_per_image, 4 * K)
    assert torch.equal(da["count"], db["count"])
    for i in range(2):
        n = int(da["count"][i])
        assert torch.equal(ra[i, :n], rb[i, :n]) and torch.equal(da["classes"][i, :n], db["classes"][i, :n])
        for k in ("boxes", "scores", "pred_boxes_std"):
            assert same_bits(da[k][i, :n], db[k][i, :n]), k
        assert torch.equal(da["valid"][i], db["valid"][i])
        q = p + "%d_" % i
        assert n == len(gold[q + "keep"])
        assert np.array_equal(ra[i, :n].cpu().numpy(), gold[q + "keep"])
        assert np.array_equal(da["classes"][i, :n].cpu().numpy(), gold[q + "cls"])
        close(da["boxes"][i, :n], gold[q + "boxes"], atol=2e-4); close(da["scores"][i, :n], gold[q + "sc"], rtol=2e-5)
        close(da["pred_boxes_std"][i, :n], gold[q + "bstd"])
    assert int(gold[p + "_bad_row"]) not in ra[0, :int(da["count"][0])].tolist()
    assert 49 not in ra[1, :int(da["count"][1])].tolist()


@pytest.mark.parametrize("nbox", [1, 70])
def test_roi_infer_keys_both_layouts_vs_torch_ops(nbox):
    """hip.roi_infer_keys alone, N = 2, P = 5 (10 waves: a partially filled last workgroup of four), K = 70 (a second lane trip of 6
    classes), class-agnostic and per-class deltas, against the ATen chain's ops on the same device: keys and boxes equal bit for bit.
    Injected: a NaN probability at class 69 of row (0, 1), written into probs; a NaN delta in the box of class 65 (nbox = 1: in the only
    box) of row (1, 2); the invalid slot (1, 4); a probability exactly thr at (0, 3), class 10.  One bad box or probability drops the
    whole row: all 70 keys of the three bad rows are the key of -1, and so is the one of the probability equal to thr.  Where the
    expected box is NaN - only in the row with the NaN delta - the stored box is unspecified and left out of the comparison."""
    from ubteacher import hip as H
    from ubteacher.modeling.rcnn import Box2BoxXYXYTransform, float_order_key
    N, P, K, thr = 2, 5, 70, 0.015625                             # (2^-6: the same number in fp32 and in Python)
    g = torch.Generator().manual_seed(700 + nbox)
    probs = torch.softmax(torch.randn(N * P, K + 1, generator=g) * 2, dim=1)
    deltas = torch.randn(N * P, 4 * nbox, generator=g) * 3
    deltas[4] *= 40.0                                            # beyond the clamp
    xy = torch.rand(N, P, 2, generator=g) * 150
    prop = torch.cat((xy, xy + torch.rand(N, P, 2, generator=g) * 80 + 2), 2)
    valid = torch.ones(N, P, dtype=torch.uint8)
    whwh = torch.tensor([[200.0, 150.0, 200.0, 150.0], [120.0, 180.0, 120.0, 180.0]])
    probs[0 * P + 1, 69] = float("nan")
    deltas[1 * P + 2, 4 * (65 if nbox > 1 else 0) + 2] = float("nan")
    valid[1, 4] = 0
    probs[0 * P + 3, 10] = thr
    bad = [(0, 1), (1, 2), (1, 4)]
    probs, deltas, prop, valid, whwh = (t.to(DEV) for t in (probs, deltas, prop, valid, whwh))
    wx, wy = L64.ROI_W
    boxes, keys = H.roi_infer_keys(probs, deltas, prop, valid, whwh, K, wx, wy, L64.ROI_CLAMP, thr, nbox=nbox)
    assert tuple(boxes.shape) == ((N, P, 4) if nbox == 1 else (N, P, nbox, 4)) and tuple(keys.shape) == (N, P * K)
    eb = Box2BoxXYXYTransform((wx, wy), L64.ROI_CLAMP).apply_deltas(deltas.view(N, P, nbox, 4), prop[:, :, None, :])
    pk = probs.view(N, P, K + 1)[:, :, :K]
    ok = valid.bool() & torch.isfinite(eb).all(dim=3).all(dim=2) & torch.isfinite(pk).all(dim=2)
    eb = torch.minimum(eb.clamp(min=0), whwh[:, None, None, :])
    flat = torch.where((pk > thr) & ok[:, :, None], pk, torch.full_like(pk, -1.0)).reshape(N, P * K)
    assert torch.equal(keys, float_order_key(flat))
    minus1 = float_order_key(torch.full((1, P * K), -1.0, device=DEV)).view(P, K)
    kv = keys.view(N, P, K)
    for n, p in bad:
        assert torch.equal(kv[n, p], minus1[p])
    assert int(kv[0, 3, 10]) == int(minus1[3, 10]) and float(probs[3, 10]) == thr
    assert int((kv != minus1[None]).sum()) > 20                  # the good rows hold real candidates
    keep = ~torch.isnan(eb).any(dim=3)                           # [N, P, nbox]
    dropped = (~keep).any(dim=2).nonzero().tolist()
    assert len(dropped) <= 2 and all(tuple(x) in [(1, 2)] for x in dropped)
    assert torch.equal(boxes.view(N, P, nbox, 4)[keep], eb[keep])


def _fixed_keys(seed):
    """sampling keys per (rows, slots) shape, drawn once: every step, eager or replayed, labels and samples the same anchors / proposals"""
    g = torch.Generator().manual_seed(seed)
    cache = {}

    def src(n, m, device):
        if (n, m) not in cache:
            cache[(n, m)] = torch.rand(n, m, generator=g).to(device)
        return cache[(n, m)]
    return src


def _trainer(amp, seed=0, fixed_keys=False):
    import bench
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBRCNNTeacherTrainer
    from ubteacher.presets import get_config
    cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "SOLVER.AMP.ENABLED", amp, "MODEL.DEVICE", DEV] + PC)
    torch.manual_seed(seed)
    tr = UBRCNNTeacherTrainer(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=96, width=128))
    bench.tune_rcnn_for_pseudo_labels(tr, tr._data_loader.batches[0])
    tr.iter, tr.log_period = 1, 10 ** 9
    tr.optimizer.param_groups[0]["lr"] = 1e-12      # a random-init R50 only stays finite at a vanishing rate (as in bench.py)
    if fixed_keys:
        tr.model.proposal_generator.sample_keys = _fixed_keys(41)
        tr.model.roi_heads.sample_keys = _fixed_keys(43)
    return tr


def test_per_class_step_fp16_amp_is_finite():
    tr = _trainer(True)
    assert tr.model.roi_heads.box_predictor.nbox == 80
    tr.run_step_full_semisup()
    rec = dict(tr.flush_metrics())
    torch.cuda.synchronize()
    losses = {k: v for k, v in rec.items() if k.startswith("loss")}
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses.values()), losses
    assert "pred_boxes_std" not in tr._last_pseudo            # the [., 4K] std has no reader
    assert torch.isfinite(tr.model.flat_state()).all()


def test_per_class_step_as_hipgraph_replays_the_eager_step(monkeypatch):
    """run_step_graph in per-class mode: two eager steps, capture, replays - against eager steps of a second trainer with the same
    weights and batch.  The existing Faster-RCNN graph test compares statistically because the sampling keys come from the device RNG,
    whose Philox offsets differ between eager and replay; here the keys are injected (fixed per shape), so the two run the same
    arithmetic on the same samples: every loss within 1e-3 (bf16 step; the replay may order fp32 atomics differently), and a wrong
    per-class kernel inside the captured graph shows."""
    monkeypatch.setenv("UTV2_PRECISION", "bf16")
    from ubteacher import ops
    outs = []
    try:
        for graph in (False, True):
            tr = _trainer(True, fixed_keys=True)
            recs = []
            for _ in range(4):
                (tr.run_step_graph if graph else tr.run_step_full_semisup)()
                tr.iter += 1
                recs.append(dict(tr.flush_metrics()))
            torch.cuda.synchronize()
            if graph:
                assert tr._step_graphs and all(st["graph"] is not None for st in tr._step_graphs.values())
            outs.append((recs, tr.model.flat_state().clone()))
    finally:
        ops.STEP_GRAPH[0] = False
    (ra, sa), (rb, sb) = outs
    for i, (a, b) in enumerate(zip(ra, rb)):
        for k, v in a.items():
            if k.startswith("loss"):
                print("GRAPH step %d %s eager %.7g graph %.7g" % (i, k, v, b[k]))
    for a, b in zip(ra, rb):
        for k, v in a.items():
            if k.startswith("loss"):
                assert v == v and abs(b[k] - v) <= 1e-3 * max(abs(v), 1e-3), (k, v, b[k])
    assert ra[0]["loss_box_reg_pseudo"] > 0.0                 # the pseudo branch did real per-class work
    assert torch.isfinite(sa).all() and torch.isfinite(sb).all()


def _step_golden_setup():
    """tests/test_rcnn_step_gpu.py::_golden_setup for step_rcnn_percls.npz: the product's per-class CPU initialisation (verified against
    the stored fingerprints), the tuned student / teacher of the generator, the stored batch and sampling keys"""
    from tests import rcnn_percls_util as U
    from tests.utv2_testutil import FixedLoader, golden_batches, rcnn_tune, state_fingerprint
    from ubteacher.engine import UBRCNNTeacherTrainer
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    d = np.load(os.path.join(G, "step_rcnn_percls.npz"), allow_pickle=False)
    base = ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0, "SOLVER.AMP.ENABLED", False] + PC
    torch.manual_seed(int(d["seed_state"]))
    sd0 = {k: v.detach().clone().contiguous() for k, v in build_model(get_config("rcnn", 1, base + ["MODEL.DEVICE", "cpu"])).state_dict().items()}
    keys = [str(k) for k in d["init_keys"]]
    assert keys == [k for k in sd0 if sd0[k].dtype.is_floating_point], "state-dict surface differs from the golden's"
    assert np.array_equal(np.stack([state_fingerprint(sd0[k]) for k in keys]), d["init_fp"]), "CPU initialisation is not the golden's"
    prod, orac = golden_batches(d, "cuda")
    cfg = get_config("rcnn", 1, base + ["MODEL.DEVICE", DEV])
    tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1)
    pstd = torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
    sd4 = dict(sd0)                                   # the recipe draws as many bbox_pred rows as it finds: four, as in the generator
    sd4[U.P + "bbox_pred.weight"] = sd0[U.P + "bbox_pred.weight"][:4]
    sd_s = U.percls_tuned(rcnn_tune(sd4, [x["image"] for x in orac[3]], mean, pstd))
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(U.teacher_of(sd_s))
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = float(d["lr"])
    K = {k: torch.from_numpy(d["keys_" + k]) for k in ("rpn_sup", "roi_sup", "rpn_unsup", "roi_unsup")}
    calls = {"rpn": 0, "roi": 0}

    def rpn_src(n, m, device):
        k = K["rpn_sup" if calls["rpn"] == 0 else "rpn_unsup"]
        calls["rpn"] += 1
        assert tuple(k.shape) == (n, m), (tuple(k.shape), n, m)
        return k.to(device)

    def roi_src(n, m, device):
        k = K["roi_sup" if calls["roi"] == 0 else "roi_unsup"]
        calls["roi"] += 1
        assert k.shape[0] == n and k.shape[1] >= m
        return k[:, :m].contiguous().to(device)

    tr.model.proposal_generator.sample_keys = rpn_src
    tr.model.roi_heads.sample_keys = roi_src
    return d, tr


def test_per_class_step_vs_reference_trainer_golden():
    """One full per-class Faster-RCNN UTv2 iteration in fp32 - the 1024 -> 728 Linear forward and backward, utv2_roi_box_loss (nbox = K) in both
    branches, the per-class teacher inference - against the reference's own UBRCNNTeacherTrainer.run_step_full_semisup around the
    reference's executed predictor (tests/golden/gen_golden_rcnn_percls.py).  The bounds of test_rcnn_step_vs_reference_trainer_golden:
    record_dict within 1e-3 (2e-2 for the weight-0 loss_rpn_loc_pseudo), the same pseudo-label set, teacher after EMA bit exact,
    student after SGD."""
    from tests.utv2_testutil import check_state_fingerprints, cpu_state, golden_record
    d, tr = _step_golden_setup()
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    ref = golden_record(d)
    for k, v in ref.items():
        if k not in ("data_time", "total_loss"):
            print("STEP %s product %.7g reference %.7g" % (k, rec[k], v))
    for k, v in ref.items():
        if k in ("data_time", "total_loss"):
            continue
        tol = 2e-2 if k == "loss_rpn_loc_pseudo" else 1e-3
        assert abs(rec[k] - v) <= tol * max(abs(v), 1e-6), (k, rec[k], v)
    assert abs(rec["total_loss"] - ref["total_loss"]) <= 1e-3 * ref["total_loss"]
    gl = tr._last_pseudo
    i = 0
    while "pseudo%d_boxes" % i in d:
        m = gl["valid"][i].bool()
        assert int(m.sum()) == len(d["pseudo%d_boxes" % i])
        assert np.array_equal(gl["classes"][i][m].long().cpu().numpy(), d["pseudo%d_classes" % i])
        np.testing.assert_allclose(gl["boxes"][i][m].cpu().numpy(), d["pseudo%d_boxes" % i], rtol=0, atol=2e-2)
        np.testing.assert_allclose(gl["scores"][i][m].cpu().numpy(), d["pseudo%d_scores" % i], rtol=1e-3)
        i += 1
    assert i == 2 and sum(len(d["pseudo%d_boxes" % j]) for j in range(2)) > 0
    check_state_fingerprints(d, "teacher", cpu_state(tr.model_teacher), 0.0, exact=True)
    check_state_fingerprints(d, "student", cpu_state(tr.model), 1e-4, rtol_update=4e-2)
