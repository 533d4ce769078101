"""MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False (the config default) in the boundary-variance ROI predictor: construction, the refused
`tsbetter` combination, the state dict against the executed reference's (tests/golden/rcnn_percls.npz), checkpoints, and the unchanged
class-agnostic layout.  No GPU."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
PC = ["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "smooth_l1"]


def cfg_of(*over):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", "cpu"] + list(over))


def predictor(cfg, klass="FastRCNNFocaltLossBoundaryVarOutputLayers"):
    from ubteacher.modeling import rcnn as R_
    from ubteacher.params import ParamStore
    st = ParamStore()
    return getattr(R_, klass)(cfg, st, 1024, "roi_heads.box_predictor"), st


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "rcnn_percls.npz")))


@pytest.mark.parametrize("klass", ["FastRCNNFocaltLossBoundaryVarOutputLayers", "FastRCNNCrossEntropyBoundaryVarOutputLayers"])
def test_per_class_predictor_constructs(klass):
    pred, _ = predictor(cfg_of(*PC), klass)
    assert pred.nbox == 80 and pred.ch == 728 and pred.ch % 8 == 0        # 81 + 320 + 320 = 721 -> 728


def test_tsbetter_with_per_class_regression_is_refused():
    with pytest.raises(NotImplementedError) as e:
        predictor(cfg_of("MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False, "MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "tsbetter"))
    msg = str(e.value)
    assert "BBOX_PSEUDO_REG_LOSS_TYPE" in msg and "CLS_AGNOSTIC_BBOX_REG" in msg and "first unsupervised step" in msg
    predictor(cfg_of("MODEL.ROI_BOX_HEAD.BBOX_PSEUDO_REG_LOSS_TYPE", "tsbetter"))      # class-agnostic: as before


@pytest.mark.parametrize("K", [80, 3])
def test_state_dict_keys_and_shapes_equal_the_reference(gold, K):
    from ubteacher.modeling import build_model
    m = build_model(cfg_of("MODEL.ROI_HEADS.NUM_CLASSES", K, *PC))
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("roi_heads.box_predictor.")}
    want = {str(k): tuple(int(x) for x in s if x >= 0) for k, s in zip(gold["k%d_keys" % K], gold["k%d_shapes" % K])}
    assert sd == want
    assert want["roi_heads.box_predictor.bbox_pred.weight"] == (4 * K, 1024) == want["roi_heads.box_predictor.bbox_pred_std.weight"]


def test_initialisation_follows_the_reference():
    from ubteacher.modeling import build_model
    torch.manual_seed(0)
    sd = build_model(cfg_of(*PC)).state_dict()
    p = "roi_heads.box_predictor."
    for name, std in (("cls_score", 0.01), ("bbox_pred", 0.001), ("bbox_pred_std", 0.0001)):    # fast_rcnn.py:768-773
        w = sd[p + name + ".weight"].float()
        assert abs(float(w.std()) / std - 1.0) < 0.05 and abs(float(w.mean())) < std * 0.05
        assert float(sd[p + name + ".bias"].abs().max()) == 0.0


def test_reference_checkpoint_round_trip(tmp_path, gold):
    """a checkpoint with the reference's names and shapes (the `model` dict DetectionCheckpointer writes) loads with every predictor
    tensor matched, and what the model saves reads back the same"""
    from ubteacher.checkpoint import DetectionCheckpointer
    from ubteacher.modeling import build_model
    torch.manual_seed(1)
    a = build_model(cfg_of(*PC))
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    pk = sorted(k for k in sd if k.startswith("roi_heads.box_predictor."))
    assert pk == sorted(str(k) for k in gold["k80_keys"])
    for k in pk:                                       # a "reference checkpoint": the reference's keys and shapes, other values
        assert tuple(sd[k].shape) == tuple(int(x) for x in gold["k80_shapes"][list(gold["k80_keys"]).index(k)] if x >= 0)
        sd[k] = torch.randn(sd[k].shape, generator=g) * 0.01
    torch.save({"model": sd}, str(tmp_path / "ref_model.pth"))
    torch.manual_seed(2)
    b = build_model(cfg_of(*PC))
    DetectionCheckpointer(b).load(str(tmp_path / "ref_model.pth"))
    out = b.state_dict()
    for k in sd:
        assert torch.equal(out[k].float().cpu(), sd[k].float()), k
    DetectionCheckpointer(b, save_dir=str(tmp_path / "out")).save("model_x")
    torch.manual_seed(3)
    c = build_model(cfg_of(*PC))
    DetectionCheckpointer(c).load(str(tmp_path / "out" / "model_x.pth"))
    for k, v in c.state_dict().items():
        assert torch.equal(v, out[k]), k


def test_class_agnostic_layout_and_state_dict_unchanged():
    from ubteacher.modeling import build_model
    from ubteacher.modeling import rcnn as R_
    pred, _ = predictor(cfg_of())
    assert pred.nbox == 1 and pred.ch == R_.PRED_CH == 96
    torch.manual_seed(0)
    m = build_model(cfg_of())
    sd = m.state_dict()
    p = "roi_heads.box_predictor."
    assert [tuple(sd[p + k].shape) for k in ("cls_score.weight", "bbox_pred.weight", "bbox_pred_std.weight", "cls_score.bias", "bbox_pred.bias",
                                             "bbox_pred_std.bias")] == [(81, 1024), (4, 1024), (4, 1024), (81,), (4,), (4,)]
    torch.manual_seed(0)
    m2 = build_model(cfg_of("MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", True))
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("name", ["utv2_frcnn_r50.yaml", "utv2_fcos_r50.yaml"])
def test_shipped_yaml_parses_and_builds(name):
    from ubteacher import add_ubteacher_config
    from ubteacher.d2 import get_cfg
    from ubteacher.modeling import build_model
    cfg = get_cfg()
    add_ubteacher_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", name))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"])
    m = build_model(cfg)
    if name == "utv2_frcnn_r50.yaml":
        assert cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG and m.roi_heads.box_predictor.nbox == 1 and m.roi_heads.box_predictor.ch == 96
