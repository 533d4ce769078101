"""SOLVER.CLIP_GRADIENTS / NESTEROV in ArenaSGD, host side: the segment table (the reference's parameter tensors as element ranges of
the arena, derived from the export views) and the validation of the solver keys at construction.  Models are built on the CPU."""
import pytest
import torch


def _cfg(kind, extra=()):
    from ubteacher.presets import get_config
    return get_config(kind, 1, ["SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1, "SOLVER.AMP.ENABLED", False,
                                "MODEL.DEVICE", "cpu"] + list(extra))


_MODELS = {}


def _model(kind):
    """one CPU model per detector for the whole module (nothing below writes to it)"""
    if kind not in _MODELS:
        from ubteacher.modeling import build_model
        torch.manual_seed(0)
        _MODELS[kind] = build_model(_cfg(kind))
    return _MODELS[kind]


VARIANTS = {"fcos": [], "rcnn": [],
            # the per-class ROI Linear: 4 * 80 bbox_pred rows behind the class scores in one fused matrix
            "rcnn_percls": ["MODEL.ROI_HEADS.LOSS", "FocalLoss", "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "smooth_l1",
                            "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", False]}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_segments_are_the_reference_tensors(variant):
    from ubteacher.modeling import build_model
    from ubteacher.params import export_segments
    kind = variant.split("_")[0]
    model = _model(kind) if not VARIANTS[variant] else build_model(_cfg(kind, VARIANTS[variant]))
    st = model.store
    segs = export_segments(st)
    named = st.trainable_named()
    # every trainable exported key has exactly one segment, of the reference tensor's numel
    assert sorted(k for k, _, _, _ in segs) == sorted(named) and len(segs) == len(named) > 50
    for k, a, b, kind_ in segs:
        assert b - a == named[k][0].numel() > 0, k
        lo, hi = st.ranges[kind_]
        assert lo <= a and b <= hi, k
    # disjoint, sorted, inside the trainable prefix
    for (ka, _, ea, _), (kb, sb, _, _) in zip(segs, segs[1:]):
        assert ea <= sb, (ka, kb)
    assert segs[0][1] >= 0 and segs[-1][2] <= st.n_train
    # the range IS the tensor: writing a segment's range of the arena shows up in that key's export view and in no other
    flat_before = st.flat.clone()
    try:
        for i in (0, len(segs) // 2, len(segs) - 1):
            k, a, b, _ = segs[i]
            st.flat[:st.n_train].zero_()
            st.flat[a:b] = 1.0
            sd = st.state_dict()
            for k2 in named:
                assert float(sd[k2].sum()) == (b - a if k2 == k else 0.0), (k, k2)
    finally:
        st.flat.copy_(flat_before)
    if variant == "fcos":     # the fused handles are split on the reference's key layout
        keys = {k for k, _, _, _ in segs}
        p = "proposal_generator.fcos_head."
        assert {p + "bbox_pred.weight", p + "bbox_pred_std.weight", p + "ctrness.weight", p + "cls_tower.0.weight",
                p + "bbox_tower.0.weight", p + "cls_tower.1.weight", p + "bbox_tower.1.bias"} <= keys
    if variant == "rcnn":
        keys = {k for k, _, _, _ in segs}
        assert {"proposal_generator.rpn_head.objectness_logits.weight", "proposal_generator.rpn_head.anchor_deltas.weight",
                "roi_heads.box_predictor.cls_score.weight", "roi_heads.box_predictor.bbox_pred_std.bias"} <= keys
    if variant == "rcnn_percls":
        by_key = {k: b - a for k, a, b, _ in segs}
        assert by_key["roi_heads.box_predictor.bbox_pred.weight"] == 320 * 1024 and by_key["roi_heads.box_predictor.bbox_pred.bias"] == 320


def test_chunk_table_tiles_the_arena():
    from ubteacher.engine.trainer import ArenaSGD
    from ubteacher.params import SegmentTable
    model = _model("fcos")
    opt = ArenaSGD(_cfg("fcos", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
                                 "SOLVER.WEIGHT_DECAY_NORM", 0.5]), model)
    tb = opt.segment_table()
    assert tb is opt.segment_table()                       # built once
    st = model.store
    cs, seg, wd, sc = tb.chunk_start.tolist(), tb.chunk_seg.tolist(), tb.chunk_wd.tolist(), tb.seg_chunks.tolist()
    assert cs[0] == 0 and cs[-1] == st.n_train == tb.n and len(cs) == tb.nchunks + 1 == len(seg) + 1
    assert all(0 < b - a <= SegmentTable.CHUNK for a, b in zip(cs, cs[1:]))
    nd = st.ranges["nodecay"][0]
    covered = [0] * tb.nseg
    for c, (a, b) in enumerate(zip(cs, cs[1:])):
        assert (b <= nd) or (a >= nd)                      # no chunk crosses the weight-decay border
        assert wd[c] == (float(torch.tensor(opt.wd, dtype=torch.float32)) if b <= nd else 0.5)   # the kernel's fp32 argument
        if seg[c] >= 0:
            s, e = tb.segments[seg[c]]
            assert s <= a and b <= e
            covered[seg[c]] += b - a
            assert sc[seg[c]][0] <= c < sc[seg[c]][0] + sc[seg[c]][1]
    assert covered == [e - s for s, e in tb.segments]
    assert sum(n for _, n in sc) == sum(1 for s in seg if s >= 0)
    # a large tensor is many chunks: it is not serialised onto one workgroup
    assert max(n for _, n in sc) >= 100
    with pytest.raises(ValueError):
        SegmentTable(10, [(0, 4), (3, 6)], [(0, 10, 0.0)], "cpu")
    with pytest.raises(ValueError):
        SegmentTable(10, [(0, 4)], [(0, 9, 0.0)], "cpu")


def test_default_configuration_builds_no_table():
    from ubteacher.engine.trainer import ArenaSGD
    opt = ArenaSGD(_cfg("fcos"), _model("fcos"))
    assert not opt.segmented and opt._seg_table is None
    assert ArenaSGD(_cfg("fcos", ["SOLVER.NESTEROV", True]), _model("fcos")).segmented
    # CLIP_* keys are read only when clipping is enabled, as in Detectron2
    assert not ArenaSGD(_cfg("fcos", ["SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "nonsense"]), _model("fcos")).segmented
    # WEIGHT_DECAY_BIAS equal to WEIGHT_DECAY is the built behaviour
    ArenaSGD(_cfg("fcos", ["SOLVER.WEIGHT_DECAY_BIAS", 0.0001]), _model("fcos"))


@pytest.mark.parametrize("keys, exc, match", [
    (["SOLVER.BIAS_LR_FACTOR", 2.0], NotImplementedError, "SOLVER.BIAS_LR_FACTOR"),
    (["SOLVER.WEIGHT_DECAY_BIAS", 0.0], NotImplementedError, "SOLVER.WEIGHT_DECAY_BIAS"),
    (["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model"], NotImplementedError,
     "SOLVER.CLIP_GRADIENTS.CLIP_TYPE"),
    (["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.0], ValueError, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE"),
    (["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", -1.0], ValueError, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE"),
    (["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", 3.0],
     NotImplementedError, "SOLVER.CLIP_GRADIENTS.NORM_TYPE"),
    (["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", 0.0],
     NotImplementedError, "SOLVER.CLIP_GRADIENTS.NORM_TYPE"),
])
def test_unbuilt_solver_keys_raise_naming_the_key(keys, exc, match):
    from ubteacher.engine.trainer import ArenaSGD
    with pytest.raises(exc, match=match):
        ArenaSGD(_cfg("fcos", keys), _model("fcos"))


@pytest.mark.parametrize("norm_type", [2.0, 1.0, float("inf")])
def test_built_norm_types_construct(norm_type):
    from ubteacher.engine.trainer import ArenaSGD
    opt = ArenaSGD(_cfg("fcos", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm",
                                 "SOLVER.CLIP_GRADIENTS.NORM_TYPE", norm_type]), _model("fcos"))
    assert opt.segmented and opt.norm_type == norm_type and opt.clip_type == "norm"


def test_trainable_stem_has_no_contiguous_segment():
    """MODEL.BACKBONE.FREEZE_AT 0 trains the 7x7 stem, stored as padded rows: its export is a strided view, and the table says so"""
    from ubteacher.engine.trainer import ArenaSGD
    from ubteacher.modeling import build_model
    cfg = _cfg("fcos", ["MODEL.BACKBONE.FREEZE_AT", 0, "SOLVER.CLIP_GRADIENTS.ENABLED", True])
    with pytest.raises(ValueError, match="stem.conv1.weight"):
        ArenaSGD(cfg, build_model(cfg))


def test_checkpoint_format_is_unchanged():
    from ubteacher.engine.trainer import ArenaSGD
    model = _model("fcos")
    a = ArenaSGD(_cfg("fcos"), model).state_dict()
    b = ArenaSGD(_cfg("fcos", ["SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.NESTEROV", True]),
                 model).state_dict()
    assert a["format"] == b["format"] and list(a) == list(b) and list(a["momentum"]) == list(b["momentum"])
