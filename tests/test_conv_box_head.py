"""The conv box head (MODEL.ROI_BOX_HEAD.NUM_CONV > 0 with NORM "GN", Detectron2 v0.6 FastRCNNConvFCHead), host side: the state-dict
surface is Detectron2's (key names, shapes, order), D2-layout tensors load and come back bit for bit, the keys that are not built name
themselves, the new tensors sit in the right weight-decay class, and the per-tensor machinery that walks the arena (the clip segment
table, the optimizer state) takes them."""
import functools
import math

import pytest
import torch

HEAD_4CONV1FC = ["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "GN"]
P = "roi_heads.box_head."


def _cfg(opts=()):
    from ubteacher.presets import get_config
    return get_config("rcnn", 1, ["MODEL.DEVICE", "cpu"] + list(opts))


@functools.lru_cache(maxsize=None)
def _model():
    """one CPU model for the module; tests that write to it put back what they changed"""
    from ubteacher.modeling import build_model
    torch.manual_seed(0)
    return build_model(_cfg(HEAD_4CONV1FC))


def test_state_dict_surface_is_detectron2s():
    sd = _model().state_dict()
    want = []
    for k in range(1, 5):      # FastRCNNConvFCHead: conv{k} = Conv2d(bias=False) with .norm = GroupNorm(32, CONV_DIM); then fc1
        want += [(P + "conv%d.weight" % k, (256, 256, 3, 3)), (P + "conv%d.norm.weight" % k, (256,)), (P + "conv%d.norm.bias" % k, (256,))]
    want += [(P + "fc1.weight", (1024, 256 * 7 * 7)), (P + "fc1.bias", (1024,))]
    assert [(k, tuple(v.shape)) for k, v in sd.items() if k.startswith(P)] == want
    # the predictors read FC_DIM features
    assert sd["roi_heads.box_predictor.cls_score.weight"].shape[1] == 1024


def test_initialisation_is_detectron2s():
    sd = _model().state_dict()
    for k in range(1, 5):
        w = sd[P + "conv%d.weight" % k]
        std = math.sqrt(2.0 / (256 * 9))          # c2_msra_fill: kaiming_normal_(mode="fan_out", nonlinearity="relu")
        assert abs(float(w.std()) - std) < 0.01 * std and abs(float(w.mean())) < 0.01 * std
        assert bool((sd[P + "conv%d.norm.weight" % k] == 1).all()) and bool((sd[P + "conv%d.norm.bias" % k] == 0).all())


def test_d2_layout_tensors_load_and_export_bit_identically():
    model = _model()
    before = model.store.flat.clone()
    try:
        g = torch.Generator().manual_seed(3)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        for k in sd:
            if k.startswith(P):
                sd[k] = torch.randn(sd[k].shape, generator=g)       # contiguous [K, C, 3, 3] / [FC, C * S * S]: Detectron2's own layout
        model.load_state_dict(sd)
        back = model.state_dict()
        for k, v in sd.items():
            assert torch.equal(back[k], v), k
        # the arena rows are [K][3][3][C]: what the NHWC conv kernels read
        h = next(h for h in model.store.handles if h.exports and h.exports[0][0] == P + "conv2.weight")
        assert torch.equal(h.t.view(256, 3, 3, 256), sd[P + "conv2.weight"].permute(0, 2, 3, 1))
    finally:
        model.store.flat.copy_(before)
        model.store.touch()


@pytest.mark.parametrize("opts,key", [
    (["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1, "MODEL.ROI_BOX_HEAD.NORM", "BN"], "MODEL.ROI_BOX_HEAD.NORM"),
    (["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 0, "MODEL.ROI_BOX_HEAD.NORM", "GN"], "MODEL.ROI_BOX_HEAD.NUM_FC"),
    (HEAD_4CONV1FC + ["MODEL.ROI_BOX_HEAD.CONV_DIM", 96], "MODEL.ROI_BOX_HEAD.CONV_DIM"),
    (["MODEL.ROI_BOX_HEAD.NUM_CONV", 4, "MODEL.ROI_BOX_HEAD.NUM_FC", 1], "MODEL.ROI_BOX_HEAD.NUM_CONV"),      # NORM "": as before
])
def test_unbuilt_combinations_name_their_key(opts, key):
    from ubteacher.modeling import build_model
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.") + " ") as e:
        build_model(_cfg(opts))
    if key.endswith("NUM_CONV"):
        assert 'NORM "GN"' in str(e.value)


def test_arena_kinds():
    kinds = {}
    for h in _model().store.handles:
        for key, _ in h.exports:
            if key.startswith(P):
                kinds[key] = h.kind
    assert len(kinds) == 14
    for key, kind in kinds.items():     # WEIGHT_DECAY_NORM: norm weight and bias in the no-decay class; conv / fc weights (and fc bias) decay
        assert kind == ("nodecay" if ".norm." in key else "decay"), key


def test_export_segments_take_the_new_tensors():
    from ubteacher.params import export_segments
    st = _model().store
    segs = {k: (a, b, kind) for k, a, b, kind in export_segments(st)}
    named = st.trainable_named()
    assert sorted(segs) == sorted(named)
    for k in named:
        if k.startswith(P):
            assert segs[k][1] - segs[k][0] == named[k][0].numel(), k
    assert segs[P + "conv3.weight"][1] - segs[P + "conv3.weight"][0] == 256 * 256 * 9


def test_arena_sgd_state_round_trip():
    from ubteacher.engine.trainer import ArenaSGD
    from ubteacher.modeling import build_model
    cfg = _cfg(HEAD_4CONV1FC)
    a = _model()
    oa = ArenaSGD(cfg, a)
    oa.store.mom.copy_(torch.randn(oa.store.mom.shape, generator=torch.Generator().manual_seed(1)))
    sd = oa.state_dict()
    for k in (P + "conv1.weight", P + "conv4.norm.bias", P + "fc1.weight"):
        assert tuple(sd["momentum"][k].shape) == tuple(a.state_dict()[k].shape), k
    torch.manual_seed(5)
    ob = ArenaSGD(cfg, build_model(cfg))
    ob.load_state_dict(sd)
    back = ob.state_dict()["momentum"]
    assert list(back) == list(sd["momentum"])
    for k, v in sd["momentum"].items():
        assert torch.equal(back[k], v), k
    oa.store.mom.zero_()


def test_default_head_is_unchanged():
    """NUM_CONV 0: no conv layer, no new key, the same arena"""
    from ubteacher.modeling import build_model
    torch.manual_seed(0)
    m = build_model(_cfg())
    assert m.roi_heads.convs == []
    assert [k for k in m.state_dict() if k.startswith(P)] == [P + "fc1.weight", P + "fc1.bias", P + "fc2.weight", P + "fc2.bias"]
