"""Golden vectors of the CONTINUOUS FCOS regression head (MODEL.FCOS.REG_DISCRETE False, the config default): the reference's own
modules executed here (CPU, build container only; same shims as gen_golden.py / gen_golden_step.py, which this script imports and
does not edit).

  fcos_cont_outputs.npz   the reference's FCOSOutputs with REG_DISCRETE False on seeded head outputs of a 2-image 96 x 128 batch.  The
                          stored `reg*` arrays are the values BEFORE the ReLU (what the product's box buffer holds); the reference is
                          given F.relu of them, as its head does (fcos/fcos.py:364), and the gradients are taken w.r.t. the stored values.
      a_*   reference defaults: KL_LOSS False, CENTER_SAMPLE True, supervised branch
      b_*   KL_LOSS True / nlloss, supervised + pseudo branches (CONSIST_REG_LOSS ts_locvar_better_nms_nll_l1)
      c_*   KL_LOSS True / klloss + LOC_FUN_ALL weight_ctr_mean, supervised + pseudo (CONSIST_REG_LOSS mse_loss_all_raw: the KL term)
      det_{test,train}_*  predict_proposals in eval / train mode (the train thresholds differ from the test ones)
      keys_kl / shapes_kl, keys_nokl / shapes_nokl: state-dict key -> shape of the reference's FCOS module for this head
  step_fcos_cont.npz      gen_golden_step.gen_step_fcos as it is, under REG_DISCRETE False (KL_LOSS True / nlloss, the shipped recipe
                          otherwise): one whole run_step_full_semisup iteration; the arrays of step_fcos.npz.

    python tests/golden/gen_golden_fcos_cont.py
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gen_golden as G  # noqa: E402
import gen_golden_step as S  # noqa: E402
from oracle import utv2_oracle as O  # noqa: E402

STRIDES = [8, 16, 32, 64, 128]
OVERRIDES = ["MODEL.FCOS.REG_DISCRETE", False]


def cont_cfg(**over):
    cfg = G.fcos_cfg()
    cfg.MODEL.FCOS.REG_DISCRETE = False
    for k, v in over.items():
        setattr(cfg.SEMISUPNET if k in ("CONSIST_REG_LOSS",) else cfg.MODEL.FCOS, k, v)
    return cfg


def make_head_outputs(g, N, H, W):
    logits, reg, std, ctr, locs = [], [], [], [], []
    for s in STRIDES:
        h, w = -(-H // s), -(-W // s)
        logits.append(torch.randn(N, 80, h, w, generator=g) * 1.5 - 2.0)
        r = torch.randn(N, 4, h, w, generator=g) * 2.0 + 1.5      # about a quarter of the stored distances are below 0: dead ReLUs
        reg.append(r)
        std.append(torch.randn(N, 4, h, w, generator=g) * 1.5)
        ctr.append(torch.randn(N, 1, h, w, generator=g))
        locs.append(O.compute_locations(h, w, s))
    flat = reg[0].view(-1)
    flat[::37] = 0.0          # exactly 0 and -0.0: no gradient (torch's ReLU)
    flat[5::41] = -0.0
    return logits, reg, std, ctr, locs


def run(d, case, fn, logits, reg, std, ctr, with_std, keep_logit_grads):
    leaves = [[t.clone().requires_grad_(True) for t in lst] for lst in (logits, reg, std, ctr)]
    losses = fn(leaves[0], [F.relu(r) for r in leaves[1]], leaves[3], leaves[2] if with_std else None)
    tot = losses["loss_fcos_cls"] + 2.0 * losses["loss_fcos_loc"] + 3.0 * losses["loss_fcos_ctr"]
    tot.backward()
    for k, v in losses.items():
        d["%s_%s" % (case, k)] = G.npy(v.float() if torch.is_tensor(v) else torch.tensor(float(v)))
    for nm, lst in zip(("logits", "reg", "std", "ctr"), leaves):
        if (nm == "logits" and not keep_logit_grads) or (nm == "std" and not with_std):
            continue
        for l in range(5):
            d["%s_g%s%d" % (case, nm, l)] = G.npy(lst[l].grad if lst[l].grad is not None else torch.zeros_like(lst[l]))


def store_targets(d, case, outm, locs, gts, bvars=False):
    tt = outm._get_ground_truth(locs, gts)
    for l in range(5):
        d["%s_labels%d" % (case, l)] = G.npy(tt["labels"][l])
        d["%s_regt%d" % (case, l)] = G.npy(tt["reg_targets"][l])
        if bvars:
            d["%s_bvars%d" % (case, l)] = G.npy(tt["boundary_vars"][l])


def ref_state_shapes(fcos_mod, cfg):
    shapes = {f: types.SimpleNamespace(channels=256, stride=s) for f, s in zip(cfg.MODEL.FCOS.IN_FEATURES, cfg.MODEL.FCOS.FPN_STRIDES)}
    m = fcos_mod.FCOS(cfg, shapes)
    sd = m.state_dict()
    keys = ["proposal_generator." + k for k in sd]
    shp = np.full((len(keys), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shp[i, :v.dim()] = list(v.shape)
    return np.array(keys), shp


def gen_outputs(structures, fo, pg):
    g = torch.Generator().manual_seed(97531)
    N, H, W = 2, 96, 128
    d = {"N": N, "H": H, "W": W}
    logits, reg, std, ctr, locs = make_head_outputs(g, N, H, W)
    for l in range(5):
        d["logits%d" % l], d["reg%d" % l], d["std%d" % l], d["ctr%d" % l] = map(G.npy, (logits[l], reg[l], std[l], ctr[l]))
    gts = G.make_gts(g, N, H, W, structures)
    gcls = G.make_gts(g, N, H, W, structures, with_scores=True)
    greg = G.make_gts(g, N, H, W, structures, with_scores=True)
    for x in greg:   # some confident teacher boundaries: a non-empty teacher-better selection
        x.reg_pred_std[:, :2] = -4.0
    G.gts_to_arrays("gt", gts, d)
    G.gts_to_arrays("pcls_gt", gcls, d)
    G.gts_to_arrays("preg_gt", greg, d)

    # (a) the reference defaults
    outm = fo.FCOSOutputs(cont_cfg(KL_LOSS=False, CENTER_SAMPLE=True))
    run(d, "a_sup", lambda lg, rg, ct, sd: outm.losses(lg, rg, ct, locs, gts, sd, [], False, branch="labeled")[1],
        logits, reg, std, ctr, False, True)
    store_targets(d, "a_sup", outm, locs, gts)
    # (b) nlloss, supervised + pseudo with the teacher-better selection
    outm = fo.FCOSOutputs(cont_cfg())
    run(d, "b_sup", lambda lg, rg, ct, sd: outm.losses(lg, rg, ct, locs, gts, sd, [], False, branch="labeled")[1],
        logits, reg, std, ctr, True, False)
    store_targets(d, "b_sup", outm, locs, gts)
    run(d, "b_pseudo", lambda lg, rg, ct, sd: outm.pseudo_losses(lg, rg, ct, locs, {"cls": gcls, "reg": greg}, sd, [], False, branch="unlabeled")[1],
        logits, reg, std, ctr, True, True)
    store_targets(d, "b_pcls", outm, locs, gcls)
    store_targets(d, "b_preg", outm, locs, greg, bvars=True)
    # (c) klloss + weight_ctr_mean
    outm = fo.FCOSOutputs(cont_cfg(KL_LOSS_TYPE="klloss", LOC_FUN_ALL="weight_ctr_mean", CONSIST_REG_LOSS="mse_loss_all_raw"))
    run(d, "c_sup", lambda lg, rg, ct, sd: outm.losses(lg, rg, ct, locs, gts, sd, [], False, branch="labeled")[1],
        logits, reg, std, ctr, True, False)
    run(d, "c_pseudo", lambda lg, rg, ct, sd: outm.pseudo_losses(lg, rg, ct, locs, {"cls": gcls, "reg": greg}, sd, [], False, branch="unlabeled")[1],
        logits, reg, std, ctr, True, False)

    # decode + NMS, eval and train mode (different thresholds / top-k so that the two are told apart)
    over = dict(INFERENCE_TH_TRAIN=0.3, PRE_NMS_TOPK_TRAIN=60, POST_NMS_TOPK_TRAIN=20, INFERENCE_TH_TEST=0.05, PRE_NMS_TOPK_TEST=1000,
                POST_NMS_TOPK_TEST=100)
    for k, v in over.items():
        d["det_cfg_" + k] = np.float64(v)
    outm = fo.FCOSOutputs(cont_cfg(**over))
    relu_reg = [F.relu(r) for r in reg]
    with torch.no_grad():
        for mode in ("test", "train"):
            outm.train(mode == "train")
            res = outm.predict_proposals(logits, relu_reg, ctr, locs, [(H, W)] * N, std, [], "cls_n_ctr")
            for i, r in enumerate(res):
                p = "det_%s_%d_" % (mode, i)
                d[p + "boxes"], d[p + "scores"], d[p + "classes"] = G.npy(r.pred_boxes.tensor), G.npy(r.scores), G.npy(r.pred_classes)
                d[p + "ctr"], d[p + "conf"], d[p + "std"] = G.npy(r.centerness), G.npy(r.cls_confid), G.npy(r.reg_pred_std)
                # the kept candidates named by (level, location index inside the level): with the class, the flat index the top-k ranked
                lev = r.fpn_levels.long().reshape(-1)
                hw = torch.zeros_like(lev)
                for j in range(len(lev)):
                    s = STRIDES[int(lev[j])]
                    wl = -(-W // s)
                    x, y = (r.locations[j] - s // 2) / s
                    hw[j] = int(round(float(y))) * wl + int(round(float(x)))
                d[p + "level"], d[p + "hw"] = G.npy(lev), G.npy(hw)
    return d


def gen_step(structures, tr, d_out):
    """gen_golden_step.gen_step_fcos unchanged, with the product configuration / initial state built under REG_DISCRETE False and the
    result written to step_fcos_cont.npz"""
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
            sd = OrderedDict((k, v.detach().clone().contiguous()) for k, v in model.state_dict().items())
            cfg_nokl = get_config(kind, 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.KL_LOSS", False] + OVERRIDES)
        finally:
            sys.path.remove(pkg)
            for k in [k for k in sys.modules if k == "ubteacher" or k.startswith("ubteacher.")]:
                del sys.modules[k]
            sys.modules.update(saved)
        fcos_mod = sys.modules["ubteacher.modeling.fcos.fcos"]     # the reference's, loaded by gen_step_fcos before this call
        d_out["keys_kl"], d_out["shapes_kl"] = ref_state_shapes(fcos_mod, cfg)
        d_out["keys_nokl"], d_out["shapes_nokl"] = ref_state_shapes(fcos_mod, cfg_nokl)
        return cfg, sd

    orig_state, orig_save = S.product_cfg_and_state, np.savez_compressed

    def save(path, **d):
        assert os.path.basename(path) == "step_fcos.npz"
        orig_save(os.path.join(HERE, "step_fcos_cont.npz"), **d)
    S.product_cfg_and_state, np.savez_compressed = product_cfg_and_state, save
    try:
        S.gen_step_fcos(structures, tr)
    finally:
        S.product_cfg_and_state, np.savez_compressed = orig_state, orig_save


if __name__ == "__main__":
    structures, fo, pg, tr = G.install_shims()
    d = gen_outputs(structures, fo, pg)
    gen_step(structures, tr, d)
    np.savez_compressed(os.path.join(HERE, "fcos_cont_outputs.npz"), **d)
    print("fcos_cont_outputs.npz:", len(d), "arrays")
