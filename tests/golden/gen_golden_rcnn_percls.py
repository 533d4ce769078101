"""Golden vectors of the boundary-variance ROI predictor with PER-CLASS box regression (MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False,
the config default): the reference's own `FastRCNNFocaltLossBoundaryVarOutputLayers` / `FastRCNNCrossEntropyBoundaryVarOutputLayers`
(roi_heads/fast_rcnn.py:214-1225) executed here (CPU, build container only; the shims of gen_golden.py, which this script imports and
does not edit).  Detectron2's `fast_rcnn_inference` is the oracle's restatement with per-class boxes.

  rcnn_percls.npz, for K = 80 ("k80_") and K = 3 ("k3_"):
      *_cls / _prop / _gtb          R sampled rows of two images in the PRODUCT's slot form: classes -1 (empty slot), K (background), 0,
                                    K-1 (the last four columns) and others; image 1 has no ground truth (background and empty slots only).
                                    The reference is given the rows with cls >= 0 (it has no empty slots; image 1 without gt_boxes).
      *_<mode>_scores/_deltas/_std  head outputs [R, K+1], [R, 4K], [R, 4K]; mode = sup_nlloss | sup_smooth_l1 | pseudo_smooth_l1
      *_<pred>_<mode>_loss_cls / _loss_box_reg / _gscores / _gdeltas / _gstd   pred = focal | ce; gradients of loss_cls + 2 loss_box_reg
                                    (rows of empty slots: zero)
      *_inf_*                       inference on N = 2 images x P = 50 proposal slots: one proposal whose decoded box is non-finite for a
                                    single class, one invalid slot (the last of image 1: the reference gets 49 rows there); per image the
                                    kept boxes, scores, classes, rows and the [., 4K] std (fast_rcnn.py:1123)
      *_keys / *_shapes             state-dict keys and shapes of the reference module
  step_rcnn_percls.npz              one whole run_step_full_semisup of the reference trainer in per-class mode (see gen_step below)

    python tests/golden/gen_golden_rcnn_percls.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gen_golden as G  # noqa: E402
from oracle import utv2_oracle as O  # noqa: E402

MODES = {"sup_nlloss": ("supervised", "nlloss", "smooth_l1"), "sup_smooth_l1": ("supervised", "smooth_l1", "smooth_l1"),
         "pseudo_smooth_l1": ("unsup_data_train", "nlloss", "smooth_l1")}


def d2_inference_per_class(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image):
    res, keeps = [], []
    for b, s, shp in zip(boxes, scores, image_shapes):
        d, rows = O.fast_rcnn_inference_per_class(b, s, shp, score_thresh, nms_thresh, topk_per_image)
        x = G_STRUCT.Instances(shp)
        x.pred_boxes = G_STRUCT.Boxes(d["boxes"]); x.scores = d["scores"]; x.pred_classes = d["classes"]
        res.append(x); keeps.append(rows)
    return res, keeps


def quant(t):
    """multiples of 1/64: exact in fp32, and the archive stays small (random mantissas do not compress)"""
    return torch.round(t * 64.0) / 64.0


def gen(K, seed, fr, br, structures, d):
    p = "k%d_" % K
    g = torch.Generator().manual_seed(seed)
    Boxes, Instances = structures.Boxes, structures.Instances
    tf = br.Box2BoxXYXYTransform(weights=(10.0, 10.0, 5.0, 5.0))
    R0, R1 = 18, 8                                    # slots of image 0 / image 1 (no ground truth)
    R = R0 + R1
    cls = torch.randint(0, K, (R,), generator=g)
    cls[0], cls[1], cls[2], cls[3] = 0, K - 1, -1, K
    cls[8:13] = K
    cls[16:R0] = -1
    cls[R0:] = K
    cls[R - 3:] = -1
    pxy = torch.rand(R, 2, generator=g) * 150
    prop = torch.cat([pxy, pxy + torch.rand(R, 2, generator=g) * 80 + 4], 1)
    gtb = prop + torch.randn(R, 4, generator=g) * 4
    fgm = (cls >= 0) & (cls < K)
    gtb[~fgm] = 0.0                                   # the product's samplers leave zeros there
    d.update({p + "cls": G.npy(cls), p + "prop": G.npy(prop), p + "gtb": G.npy(gtb), p + "R0": np.int64(R0)})
    live = cls >= 0
    l0, l1 = live.clone(), live.clone()
    l0[R0:] = False; l1[:R0] = False
    i0 = Instances((300, 300)); i0.proposal_boxes = Boxes(prop[l0]); i0.gt_boxes = Boxes(gtb[l0]); i0.gt_classes = cls[l0]
    i1 = Instances((300, 300)); i1.proposal_boxes = Boxes(prop[l1]); i1.gt_classes = cls[l1]       # no gt_boxes: fast_rcnn.py:876-882
    for mode, (branch, sup_type, pseudo_type) in MODES.items():
        scores = quant(torch.randn(R, K + 1, generator=g) * 2)
        deltas = quant(torch.randn(R, 4 * K, generator=g) * 0.5)
        std = quant(torch.randn(R, 4 * K, generator=g) * 1.5)
        d[p + mode + "_scores"], d[p + mode + "_deltas"], d[p + mode + "_std"] = G.npy(scores), G.npy(deltas), G.npy(std)
        for pred, klass in (("focal", fr.FastRCNNFocaltLossBoundaryVarOutputLayers), ("ce", fr.FastRCNNCrossEntropyBoundaryVarOutputLayers)):
            duck = types.SimpleNamespace(num_classes=K, box2box_transform=tf, smooth_l1_beta=0.0, box_reg_loss_type=sup_type,
                                         box_pseudo_reg_loss_type=pseudo_type, loss_weight={"loss_box_reg": 1.0}, ts_better=0.1, t_cert=0.5)
            for name in ("comput_focal_loss", "box_reg_loss", "box_reg_pseudo_loss"):
                if hasattr(klass, name):
                    setattr(duck, name, types.MethodType(getattr(klass, name), duck))
            leaves = [v[live].clone().requires_grad_(True) for v in (scores, deltas, std)]
            ls = klass.losses(duck, tuple(leaves), [i0, i1], branch)
            (ls["loss_cls"] + 2.0 * ls["loss_box_reg"]).backward()
            q = p + pred + "_" + mode
            d[q + "_loss_cls"], d[q + "_loss_box_reg"] = G.npy(ls["loss_cls"]), G.npy(ls["loss_box_reg"])
            for nm, full, leaf in zip(("scores", "deltas", "std"), (scores, deltas, std), leaves):
                gr = torch.zeros_like(full)
                if leaf.grad is not None:
                    gr[live] = leaf.grad
                d[q + "_g" + nm] = G.npy(gr)
    # ---- inference ------------------------------------------------------------------------------------------------------
    N, P = 2, 50
    sizes = [(300, 280), (250, 300)]
    p0 = torch.rand(N, P, 2, generator=g) * 200
    ip = torch.cat([p0, p0 + torch.rand(N, P, 2, generator=g) * 90 + 4], -1)
    sc = quant(torch.randn(N * P, K + 1, generator=g) * 3)
    de = quant(torch.randn(N * P, 4 * K, generator=g) * 2)
    sd = quant(torch.randn(N * P, 4 * K, generator=g))
    bad_row, bad_cls = 7, K - 2
    de[bad_row, 4 * bad_cls + 1] = float("nan")       # one class of one proposal decodes to a non-finite box (the clamp keeps a NaN): the whole row goes
    sc[bad_row, :] = -5.0
    sc[bad_row, 0] = 9.0                               # ... although its class-0 candidate would be kept
    valid = torch.ones(N, P, dtype=torch.uint8)
    valid[1, P - 1] = 0
    sc[N * P - 1, :] = -5.0
    sc[N * P - 1, 1 % K] = 9.0                         # the invalid slot would be a confident detection
    duck = types.SimpleNamespace(num_classes=K, box2box_transform=tf, test_score_thresh=0.05, test_nms_thresh=0.5, test_topk_per_image=100)
    klass = fr.FastRCNNFocaltLossBoundaryVarOutputLayers
    for name in ("predict_boxes", "predict_boxes_std", "predict_probs"):
        setattr(duck, name, types.MethodType(getattr(klass, name), duck))
    rows_in = [torch.arange(P), torch.arange(P - 1)]
    pis = []
    for i in range(N):
        x = Instances(sizes[i]); x.proposal_boxes = Boxes(ip[i][rows_in[i]])
        pis.append(x)
    sel = torch.cat([rows_in[0], P + rows_in[1]])
    res, keep = klass.inference(duck, (sc[sel], de[sel], sd[sel]), pis)
    d.update({p + "inf_prop": G.npy(ip), p + "inf_valid": G.npy(valid), p + "inf_scores": G.npy(sc), p + "inf_deltas": G.npy(de),
              p + "inf_std": G.npy(sd), p + "inf_sizes": np.array(sizes), p + "inf_bad_row": np.int64(bad_row)})
    for i in range(N):
        q = p + "inf%d_" % i
        assert tuple(res[i].pred_boxes_std.shape) == (len(keep[i]), 4 * K)
        assert len(keep[i]) > 5 and not (i == 0 and bad_row in keep[i].tolist())
        d[q + "boxes"], d[q + "sc"], d[q + "cls"] = G.npy(res[i].pred_boxes.tensor), G.npy(res[i].scores), G.npy(res[i].pred_classes)
        d[q + "bstd"], d[q + "keep"] = G.npy(res[i].pred_boxes_std), G.npy(keep[i])
    # ---- state dict ------------------------------------------------------------------------------------------------------
    m = klass.__new__(klass)
    torch.nn.Module.__init__(m)
    m.cls_score = torch.nn.Linear(1024, K + 1)          # fast_rcnn.py:760-766, cls_agnostic_bbox_reg False
    nbr = K
    m.bbox_pred = torch.nn.Linear(1024, nbr * len(tf.weights))
    m.bbox_pred_std = torch.nn.Linear(1024, nbr * len(tf.weights))
    sdict = m.state_dict()
    keys = ["roi_heads.box_predictor." + k for k in sdict]
    shp = np.full((len(keys), 2), -1, dtype=np.int64)
    for i, v in enumerate(sdict.values()):
        shp[i, :v.dim()] = list(v.shape)
    d[p + "keys"], d[p + "shapes"] = np.array(keys), shp


# ---------------------------------------------------------------------------------------------------------------------
# one whole run_step_full_semisup of the reference's UBRCNNTeacherTrainer in per-class mode (pseudo smooth_l1), 96 x 128, the arrays of
# step_rcnn.npz -> step_rcnn_percls.npz.  gen_golden_step.gen_step_rcnn is run as it is; what it takes from its module / the oracle by
# name is swapped for the call: the product configuration and initial state are built per-class, the tuned state gets [4K, in]
# bbox_pred / bbox_pred_std (tests/rcnn_percls_util.py), and the teacher pass / student losses are the oracle's backbone, RPN, proposal
# sampling and box head (all shape-generic) around the REFERENCE's executed predictor (losses / inference of
# FastRCNNFocaltLossBoundaryVarOutputLayers) instead of the oracle's class-agnostic restatement.
OVERRIDES = ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "smooth_l1"]


def gen_step(structures, tr, fr, br):
    import gen_golden_step as S
    from tests import rcnn_percls_util as U
    K = 80
    klass = fr.FastRCNNFocaltLossBoundaryVarOutputLayers
    duck = types.SimpleNamespace(num_classes=K, box2box_transform=br.Box2BoxXYXYTransform(weights=(10.0, 10.0, 5.0, 5.0)), smooth_l1_beta=0.0,
                                 box_reg_loss_type="nlloss", box_pseudo_reg_loss_type="smooth_l1", loss_weight={"loss_box_reg": 1.0},
                                 ts_better=0.1, t_cert=0.5, test_score_thresh=0.05, test_nms_thresh=0.5, test_topk_per_image=100)
    for name in ("comput_focal_loss", "box_reg_loss", "box_reg_pseudo_loss", "predict_boxes", "predict_boxes_std", "predict_probs"):
        setattr(duck, name, types.MethodType(getattr(klass, name), duck))
    Boxes, Instances = structures.Boxes, structures.Instances

    def product_cfg_and_state(kind, seed):
        saved = {k: v for k, v in sys.modules.items() if k == "ubteacher" or k.startswith("ubteacher.")}
        for k in saved:
            del sys.modules[k]
        pkg = os.path.join(ROOT, "unbiased-teacher-v2_amd")
        sys.path.insert(0, pkg)
        try:
            from ubteacher.modeling import build_model
            from ubteacher.presets import get_config
            cfg = get_config(kind, 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                       "SOLVER.AMP.ENABLED", False, "MODEL.DEVICE", "cpu"] + OVERRIDES)
            torch.manual_seed(seed)
            model = build_model(cfg)
            sd = S.OrderedDict((k, v.detach().clone().contiguous()) for k, v in model.state_dict().items())
        finally:
            sys.path.remove(pkg)
            for k in [k for k in sys.modules if k == "ubteacher" or k.startswith("ubteacher.")]:
                del sys.modules[k]
            sys.modules.update(saved)
        return cfg, sd

    orig_tune, orig_net = S.rcnn_tune, S.ParamNet

    def tune(sd, images, mean, pstd, seed=0):
        return S.OrderedDict(U.percls_tuned(orig_tune(sd, images, mean, pstd, seed), K))

    def param_net(sd, frozen):
        b = sd[U.P + "bbox_pred_std.bias"]
        if b.numel() == 4:                             # gen_step_rcnn's teacher: the four-column std bias of -3, widened to 4K
            sd = S.OrderedDict(sd)
            sd[U.P + "bbox_pred_std.bias"] = b.repeat(K)
        return orig_net(sd, frozen)

    def head(sd, images, mean, pix_std):
        p, sizes = O.rcnn_backbone(sd, images, mean, pix_std)
        feats = [p[k] for k in ("p2", "p3", "p4", "p5", "p6")]
        anchors = O.make_anchors([(f.shape[2], f.shape[3]) for f in feats], [4, 8, 16, 32, 64])
        obj, dl = O.rpn_head(sd, feats)
        return feats, sizes, anchors, obj, dl

    def rcnn_teacher(sd, images, mean, pix_std, pre_topk=2000, post_topk=1000, thr=0.7):
        feats, sizes, anchors, obj, dl = head(sd, images, mean, pix_std)
        props = O.find_top_rpn_proposals(anchors, obj, dl, sizes, pre_topk, post_topk)
        preds = O.box_head(sd, O.roi_pool(feats[:4], [q["boxes"] for q in props]))
        assert preds[1].shape[1] == 4 * K == preds[2].shape[1]
        pis = []
        for q, size in zip(props, sizes):
            x = Instances(tuple(size)); x.proposal_boxes = Boxes(q["boxes"])
            pis.append(x)
        res, _ = klass.inference(duck, preds, pis)
        out = []
        for r in res:
            m = r.scores > thr
            out.append(dict(boxes=r.pred_boxes.tensor[m], scores=r.scores[m], classes=r.pred_classes[m], pred_boxes_std=r.pred_boxes_std[m]))
        return out, props

    def rcnn_student_losses(sd, images, gts, rpn_keys, roi_keys, pseudo, mean, pix_std, pre_topk=2000, post_topk=1000, props_override=None):
        feats, sizes, anchors, obj, dl = head(sd, images, mean, pix_std)
        rl, _ = O.rpn_losses(torch.cat(anchors), torch.cat(obj, 1), torch.cat(dl, 1), gts, rpn_keys, pseudo)
        with torch.no_grad():
            props = O.find_top_rpn_proposals(anchors, obj, dl, sizes, pre_topk, post_topk)
        gts4 = [{k: v for k, v in g.items() if k != "pred_boxes_std"} for g in gts]      # [., 4K]: read by nothing in this mode
        sampled = [O.roi_label_and_sample(q["boxes"], g, k(len(q["boxes"]), len(g["boxes"])) if callable(k) else k, pseudo)
                   for q, g, k in zip(props, gts4, roi_keys)]
        preds = O.box_head(sd, O.roi_pool(feats[:4], [s["proposal_boxes"] for s in sampled]))
        insts = []
        for s, size in zip(sampled, sizes):
            x = Instances(tuple(size))
            x.proposal_boxes, x.gt_boxes, x.gt_classes = Boxes(s["proposal_boxes"]), Boxes(s["gt_boxes"]), s["gt_classes"]
            insts.append(x)
        losses = dict(klass.losses(duck, preds, insts, "unsup_data_train" if pseudo else "supervised"))
        losses.update(rl)
        return losses, props, sampled

    saved = (S.product_cfg_and_state, S.rcnn_tune, S.ParamNet, O.rcnn_teacher, O.rcnn_student_losses, np.savez_compressed)
    orig_save = np.savez_compressed

    def save(path, **d):
        assert os.path.basename(path) == "step_rcnn.npz"
        for i in range(2):                              # the [n, 4K] std of the pseudo boxes: a checksum per box keeps the file small
            d["pseudo%d_std" % i] = d["pseudo%d_std" % i].astype(np.float64).sum(axis=1)
        orig_save(os.path.join(HERE, "step_rcnn_percls.npz"), **d)
    S.product_cfg_and_state, S.rcnn_tune, S.ParamNet, O.rcnn_teacher, O.rcnn_student_losses, np.savez_compressed = (
        product_cfg_and_state, tune, param_net, rcnn_teacher, rcnn_student_losses, save)
    try:
        S.gen_step_rcnn(structures, tr)
    finally:
        S.product_cfg_and_state, S.rcnn_tune, S.ParamNet, O.rcnn_teacher, O.rcnn_student_losses, np.savez_compressed = saved


if __name__ == "__main__":
    structures, fo, pg, tr = G.install_shims()
    G_STRUCT = structures
    br = G._load("ubteacher.modeling.box_regression", G.REF + "/ubteacher/modeling/box_regression.py")
    fr = G._load("ubteacher.modeling.roi_heads.fast_rcnn", G.REF + "/ubteacher/modeling/roi_heads/fast_rcnn.py")
    fr.fast_rcnn_inference = d2_inference_per_class
    d = {}
    gen(80, 4101, fr, br, structures, d)
    gen(3, 4103, fr, br, structures, d)
    out = os.path.join(HERE, "rcnn_percls.npz")
    np.savez_compressed(out, **{k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in d.items()})
    print("rcnn_percls.npz:", len(d), "arrays,", os.path.getsize(out), "bytes")
    gen_step(structures, tr, fr, br)
