"""Test-time augmentation (TEST.AUG), host side: the view list of ubteacher.modeling.test_time_augmentation.tta_views, the numpy
return-trip reference the GPU tests compare the kernel with (tests/tta_ref.py), the refusals, and the default configuration."""
import numpy as np
import pytest

from tests import tta_ref as R


def _cfg(**aug):
    from ubteacher import add_ubteacher_config
    from ubteacher.d2 import get_cfg
    cfg = get_cfg()
    add_ubteacher_config(cfg)
    for k, v in aug.items():
        cfg.TEST.AUG[k] = v
    return cfg


def test_view_order_sizes_and_chains():
    from ubteacher.modeling.test_time_augmentation import tta_views
    cfg = _cfg(MIN_SIZES=(64, 96), FLIP=True)
    v = tta_views(cfg, (96, 128), (96, 128))
    assert [(x["size"], x["flip"]) for x in v] == [((64, 85), False), ((64, 85), True), ((96, 128), False), ((96, 128), True)]
    assert v[0]["transforms"] == [("resize", 96, 128, 64, 85)]
    assert v[1]["transforms"] == [("resize", 96, 128, 64, 85), ("hflip", 85)]
    assert [(h, w, f) for h, w, f in R.views((96, 128), (64, 96), 4000, True)] == [x["size"] + (x["flip"],) for x in v]
    # FLIP False halves the list
    v2 = tta_views(_cfg(MIN_SIZES=(64, 96), FLIP=False), (96, 128), (96, 128))
    assert [(x["size"], x["flip"]) for x in v2] == [((64, 85), False), ((96, 128), False)]
    # MAX_SIZE caps the long side: 96 x 128 at short side 96 would be 96 x 128; capped at 100 it is 75 x 100
    v3 = tta_views(_cfg(MIN_SIZES=(96,), MAX_SIZE=100, FLIP=False), (96, 128), (96, 128))
    assert v3[0]["size"] == (75, 100) == R.shortest_edge(96, 128, 96, 100)
    # the loader image differs from the record's (height, width): a leading resize opens every chain
    v4 = tta_views(cfg, (96, 128), (144, 192))
    assert all(x["transforms"][0] == ("resize", 144, 192, 96, 128) for x in v4)
    assert v4[3]["transforms"] == [("resize", 144, 192, 96, 128), ("resize", 96, 128, 96, 128), ("hflip", 128)]
    # a portrait image: the short side is the width
    assert tta_views(_cfg(MIN_SIZES=(64,), FLIP=False), (128, 96), (128, 96))[0]["size"] == (85, 64)


def test_default_view_list_is_nine_sizes_times_flip():
    from ubteacher.modeling.test_time_augmentation import tta_views
    v = tta_views(_cfg(), (800, 1333), (480, 800))
    assert len(v) == 18 and [x["size"][0] for x in v[0::2]] == [400, 500, 600, 700, 800, 900, 1000, 1100, 1200]
    assert [x["flip"] for x in v] == [False, True] * 9


def test_transform_table_holds_one_fp32_ratio_per_step():
    from ubteacher import hip
    from ubteacher.modeling.test_time_augmentation import tta_table, tta_views
    v = tta_views(_cfg(MIN_SIZES=(64, 96), FLIP=True), (96, 128), (150, 199))
    t = tta_table(v, (150, 199))
    assert t.dtype == np.float32 and t.shape == (4, hip.TTA_STRIDE)
    assert t[1, hip.TTA_FLIP] == 1 and t[1, hip.TTA_WVIEW] == 85 and t[0, hip.TTA_FLIP] == 0
    assert t[0, hip.TTA_RX_VIEW] == np.float32(128 / 85) and t[0, hip.TTA_RY_VIEW] == np.float32(96 / 64)
    assert t[0, hip.TTA_RX_LEAD] == np.float32(199 / 128) and t[0, hip.TTA_RY_LEAD] == np.float32(150 / 96)
    assert t[2, hip.TTA_RX_VIEW] == 1 and tuple(t[3, hip.TTA_ORIG_H:hip.TTA_ORIG_W + 1]) == (150, 199)
    t0 = tta_table(tta_views(_cfg(MIN_SIZES=(64,), FLIP=False), (96, 128), (96, 128)), (96, 128))
    assert t0[0, hip.TTA_RX_LEAD] == 1 and t0[0, hip.TTA_RY_LEAD] == 1


def test_return_trip_reference():
    rng = np.random.default_rng(0)
    # un-flip followed by flip is the identity on integer boxes
    x1 = rng.integers(0, 60, 50); y1 = rng.integers(0, 40, 50)
    b = np.stack([x1, y1, x1 + rng.integers(1, 25, 50), y1 + rng.integers(1, 24, 50)], 1).astype(np.float32)
    assert np.array_equal(R.unflip(R.unflip(b, 85), 85), b)
    f = R.unflip(b, 85)
    assert np.all(f[:, 0] <= f[:, 2]) and np.array_equal(f[:, 0], 85 - b[:, 2]) and np.array_equal(f[:, 1::2], b[:, 1::2])
    # a flipped box that starts at x1 = 0 lands on W
    assert R.unflip(np.array([[0, 3, 10, 9]], np.float32), 85)[0].tolist() == [75, 3, 85, 9]
    # a resize chain maps the view's corner box onto the original's corner box (to fp32 rounding of the two ratios)
    for view in ((64, 85, False), (64, 85, True), (96, 128, False)):
        corner = np.array([[0, 0, view[1], view[0]]], np.float32)
        back = R.return_trip(corner, view, (96, 128), (150, 199))
        np.testing.assert_allclose(back[0], [0, 0, 199, 150], rtol=3e-7, atol=0)
    # one multiplication per step, not one combined ratio
    b1 = np.array([[7.3, 5.1, 33.7, 41.9]], np.float32)
    want_x = np.float32(np.float32(b1[0, 0] * np.float32(128 / 85)) * np.float32(199 / 128))
    assert R.return_trip(b1, (64, 85, False), (96, 128), (150, 199))[0, 0] == want_x
    assert R.clip(np.array([[-3, -1, 250, 151]], np.float32), (150, 199))[0].tolist() == [0, 0, 199, 150]


@pytest.mark.parametrize("aug,key", [(dict(MIN_SIZES=()), "TEST.AUG.MIN_SIZES"), (dict(MIN_SIZES=(400, 0)), "TEST.AUG.MIN_SIZES"),
                                     (dict(MIN_SIZES=(400, -8)), "TEST.AUG.MIN_SIZES"), (dict(MIN_SIZES=(400, 800), MAX_SIZE=700), "TEST.AUG.MAX_SIZE")])
def test_refusals_name_their_key(aug, key):
    from ubteacher.modeling.test_time_augmentation import DetectorWithTTA, tta_views
    cfg = _cfg(**aug)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        tta_views(cfg, (96, 128), (96, 128))
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        DetectorWithTTA(cfg, object())


def test_default_config_runs_no_tta(monkeypatch):
    """TEST.AUG.ENABLED False (every shipped YAML): the --eval-only path returns Trainer.test's result and never builds the wrapper"""
    import argparse
    import train_net
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    for kind in ("fcos", "rcnn"):
        assert get_config(kind).TEST.AUG.ENABLED is False
    calls = []
    monkeypatch.setattr(UBTeacherTrainer, "build_model", classmethod(lambda cls, cfg: type("M", (), {})()))
    monkeypatch.setattr(UBTeacherTrainer, "test", classmethod(lambda cls, cfg, model, evaluators=None: calls.append("test") or {"bbox": {"AP": 1.0}}))
    monkeypatch.setattr(UBTeacherTrainer, "test_with_TTA", classmethod(lambda cls, cfg, model: calls.append("tta") or {"bbox_TTA": {"AP": 2.0}}))
    monkeypatch.setattr(train_net, "setup_logger", lambda *a, **k: None)
    args = argparse.Namespace(config_file=train_net.default_argument_parser().get_default("config_file"), eval_only=True, resume=False,
                              opts=["MODEL.WEIGHTS", "", "MODEL.DEVICE", "cpu", "SEED", 0])
    res = train_net.main(args)
    assert calls == ["test"] and not any(k.endswith("_TTA") for k in res)
    args.opts += ["TEST.AUG.ENABLED", True]
    res = train_net.main(args)
    assert calls == ["test", "test", "tta"] and res["bbox"]["AP"] == 1.0 and res["bbox_TTA"]["AP"] == 2.0


def test_more_candidates_than_the_nms_takes_is_refused_by_name():
    import torch
    from ubteacher import hip
    from ubteacher.modeling.test_time_augmentation import DetectorWithTTA
    tta = DetectorWithTTA(_cfg(), type("M", (), {"training": False})())
    D = hip.NMS_MAX_CANDIDATES // 18 + 1
    dets = [(None, torch.zeros(D), None, None)] * 18
    with pytest.raises(ValueError, match=r"TEST\.AUG\.MIN_SIZES.*TEST\.DETECTIONS_PER_IMAGE"):
        tta.merge(dets, None, (96, 128))
