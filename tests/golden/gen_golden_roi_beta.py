"""Golden vectors of the boundary-variance ROI predictors' box losses under MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE
"giou": the reference's own `FastRCNNFocaltLossBoundaryVarOutputLayers` / `FastRCNNCrossEntropyBoundaryVarOutputLayers`
(roi_heads/fast_rcnn.py:214-1092) `losses()` executed here (CPU, build container only; the Detectron2 / fvcore shims of gen_golden.py,
which this script imports and does not edit - fvcore's smooth_l1_loss and giou_loss are its restatements, Detectron2 is absent).

The reference is run in FLOAT64 on inputs that are exact in fp32 (multiples of 1/64), so the arrays are the reference's arithmetic
to ~1e-15; the one fp32 step left is nl_loss's constant 2 log(2 pi), which the reference builds as a float32 tensor (:1283-1285).

  roi_beta.npz (K = 3, R = 48 slots of two images; image 1 has no ground truth)
      cls / prop / gtb / gstd       the slots in the PRODUCT's form: classes -1 (empty slot), K (background), 0 .. K-1; the reference is
                                    given the rows with cls >= 0 (it has no empty slots; image 1 without gt_boxes)
      deltas / std                  head outputs [R, 4K]; the class-agnostic runs ("agn") read their columns 0..3
      betas                         the SMOOTH_L1_BETA values
      <pred>_<lay>_<type>_b<i>_loss / _gdeltas / _gstd    pred = focal | ce, lay = agn | pc, type = smooth_l1 | nlloss | giou (supervised
                                    branch) | pseudo (unsup_data_train, BBOX_PSEUDO_REG_LOSS_TYPE smooth_l1), i = index into betas:
                                    loss_box_reg and its gradients w.r.t. deltas / std ([R, 4] or [R, 4K]; rows of empty slots: zero)

    python tests/golden/gen_golden_roi_beta.py
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

K, R0, R1 = 3, 36, 12
BETAS = (0.0, 0.11, 1.0)
TYPES = {"smooth_l1": ("supervised", "smooth_l1"), "nlloss": ("supervised", "nlloss"), "giou": ("supervised", "giou"),
         "pseudo": ("unsup_data_train", "nlloss")}


def quant(t):
    return torch.round(t * 64.0) / 64.0


def inputs():
    g = torch.Generator().manual_seed(5207)
    R = R0 + R1
    cls = torch.randint(0, K, (R,), generator=g)
    cls[0], cls[1], cls[2], cls[3] = 0, K - 1, -1, K
    cls[20:30] = K
    cls[32:R0] = -1
    cls[R0:] = K
    cls[R - 4:] = -1
    pxy = torch.round(torch.rand(R, 2, generator=g) * 150)
    prop = torch.cat([pxy, pxy + torch.round(torch.rand(R, 2, generator=g) * 80 + 4)], 1)
    gtb = prop + quant(torch.randn(R, 4, generator=g) * 4)
    fgm = (cls >= 0) & (cls < K)
    gtb[~fgm] = 0.0                                   # the product's samplers leave zeros there
    tf_w = 10.0
    deltas = quant(torch.randn(R, 4 * K, generator=g) * 0.5)
    std = quant(torch.randn(R, 4 * K, generator=g) * 1.5)
    gstd = quant(torch.randn(R, 4, generator=g) * 2)
    # the selected columns of the foreground rows, per-class AND class-agnostic (columns 0..3): around the regression target, so that
    # |d - t| falls on both sides of 0.11 and of 1.0; then four GIoU geometries
    sw, sh = prop[:, 2] - prop[:, 0] + 1.0, prop[:, 3] - prop[:, 1] + 1.0
    t = torch.stack((tf_w * (gtb[:, 0] - prop[:, 0]) / sw, tf_w * (gtb[:, 2] - prop[:, 2]) / sw, tf_w * (gtb[:, 1] - prop[:, 1]) / sh,
                     tf_w * (gtb[:, 3] - prop[:, 3]) / sh), dim=1)
    near = quant(t + (torch.rand(R, 4, generator=g) * 2 - 1) * torch.tensor([0.06, 0.2, 0.6, 2.0])[torch.randint(0, 4, (R, 4), generator=g)])
    fg = torch.nonzero(fgm).squeeze(1).tolist()
    near[fg[1]] = torch.tensor([2 * tf_w, 2 * tf_w, 0.0, 0.0])                 # disjoint: moved two widths to the right
    near[fg[2]] = torch.tensor([tf_w / 4, -tf_w / 4, tf_w / 4, -tf_w / 4])     # shrunk by a quarter side ...
    gtb[fg[2]] = prop[fg[2]] + torch.tensor([-2.0, -2.0, 2.0, 2.0])            # ... inside a gt box that contains the proposal
    near[fg[3]] = torch.tensor([tf_w / 2, -tf_w / 2, 0.0, 0.0])                # zero area: x1 == x2
    for r in fg:
        c = int(cls[r])
        deltas[r, 4 * c:4 * c + 4] = near[r]
        if c != 0:
            deltas[r, 0:4] = near[r]
    return cls, prop, gtb, gstd, deltas, std


def main():
    structures, fo, pg, tr = G.install_shims()
    br = G._load("ubteacher.modeling.box_regression", G.REF + "/ubteacher/modeling/box_regression.py")
    fr = G._load("ubteacher.modeling.roi_heads.fast_rcnn", G.REF + "/ubteacher/modeling/roi_heads/fast_rcnn.py")
    Boxes, Instances = structures.Boxes, structures.Instances
    cls, prop, gtb, gstd, deltas, std = inputs()
    R = R0 + R1
    d = {"cls": G.npy(cls), "prop": G.npy(prop), "gtb": G.npy(gtb), "gstd": G.npy(gstd), "deltas": G.npy(deltas), "std": G.npy(std),
         "betas": np.array(BETAS, dtype=np.float64), "R0": np.int64(R0)}
    live = cls >= 0
    l0, l1 = live.clone(), live.clone()
    l0[R0:] = False
    l1[:R0] = False
    f64 = torch.float64
    i0 = Instances((300, 300)); i0.proposal_boxes = Boxes(prop[l0].to(f64)); i0.gt_boxes = Boxes(gtb[l0].to(f64)); i0.gt_classes = cls[l0]
    i0.gt_loc_std = gstd[l0].to(f64)
    i1 = Instances((300, 300)); i1.proposal_boxes = Boxes(prop[l1].to(f64)); i1.gt_classes = cls[l1]      # no gt_boxes: fast_rcnn.py:876-882
    tf = br.Box2BoxXYXYTransform(weights=(10.0, 10.0, 5.0, 5.0))
    scores = torch.zeros(R, K + 1, dtype=f64)
    for pred, klass in (("focal", fr.FastRCNNFocaltLossBoundaryVarOutputLayers), ("ce", fr.FastRCNNCrossEntropyBoundaryVarOutputLayers)):
        for lay, ncol in (("agn", 4), ("pc", 4 * K)):
            for typ, (branch, sup_type) in TYPES.items():
                for bi, beta in enumerate(BETAS):
                    duck = types.SimpleNamespace(num_classes=K, box2box_transform=tf, smooth_l1_beta=beta, box_reg_loss_type=sup_type,
                                                 box_pseudo_reg_loss_type="smooth_l1", loss_weight={"loss_box_reg": 1.0}, ts_better=0.1,
                                                 t_cert=0.5)
                    for name in ("comput_focal_loss", "box_reg_loss", "box_reg_pseudo_loss"):
                        if hasattr(klass, name):
                            setattr(duck, name, types.MethodType(getattr(klass, name), duck))
                    leaves = [v[live].to(f64).clone().requires_grad_(True) for v in (scores, deltas[:, :ncol], std[:, :ncol])]
                    ls = klass.losses(duck, tuple(leaves), [i0, i1], branch)
                    ls["loss_box_reg"].backward()
                    q = "%s_%s_%s_b%d" % (pred, lay, typ, bi)
                    d[q + "_loss"] = G.npy(ls["loss_box_reg"])
                    for nm, leaf in (("deltas", leaves[1]), ("std", leaves[2])):
                        gr = torch.zeros(R, ncol, dtype=f64)
                        if leaf.grad is not None:
                            gr[live] = leaf.grad
                        d[q + "_g" + nm] = G.npy(gr)
    out = os.path.join(HERE, "roi_beta.npz")
    np.savez_compressed(out, **d)
    print("roi_beta.npz:", len(d), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
