"""Shared by tests/golden/gen_golden_rcnn_percls.py and tests/test_rcnn_percls_gpu.py (pure torch, no product import): the per-class
predictor weights of the tuned whole-step state."""
import torch

P = "roi_heads.box_predictor."


def percls_tuned(sd, K=80, seed=11):
    """`sd` = a state dict tuned by the class-agnostic recipe (gen_golden_step.rcnn_tune / test_rcnn_step_gpu.tune) whose model was built
    per-class: bbox_pred / bbox_pred_std get [4K, in] weights at the scale the recipe chose for its [4, in] ones (the recipe's own
    generator is left alone, so every other tensor equals the class-agnostic fixture's)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for name in ("bbox_pred", "bbox_pred_std"):
        w = out[P + name + ".weight"]
        scale = float(w.double().abs().mean()) * 1.2533141373155001      # E|x| of a normal = sigma * sqrt(2 / pi)
        out[P + name + ".weight"] = torch.randn(4 * K, w.shape[1], generator=g) * scale
        out[P + name + ".bias"] = torch.zeros(4 * K)
    return out


def teacher_of(sd_s, K=80):
    """the step fixtures' teacher: the student with confident boundaries"""
    sd_t = dict(sd_s)
    sd_t[P + "bbox_pred_std.bias"] = torch.full((4 * K,), -3.0)
    return sd_t
