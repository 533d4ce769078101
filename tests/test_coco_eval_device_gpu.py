"""The device COCO box evaluator (csrc/coco_eval.hip, evaluation/coco_eval_device.py, TEST.EVALUATOR "COCOeval_device"): its precision
and recall arrays equal the host reference's (coco_box_eval) exactly, its six AP numbers equal COCOBoxEvaluator's, it plugs into
Trainer.test for both detectors, and a two-rank run gives the one-rank result."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
sys.path.insert(0, ROOT)

from tests.test_coco_dataset import tiny  # noqa: E402,F401  (the registered tiny COCO-format set)
from tests.test_coco_eval_full import make_split  # noqa: E402

SPLITS = [
    dict(seed=11),
    dict(seed=12, tie_scores=True),
    dict(seed=13, big_pair=150, det_max=30, tie_scores=True),
    dict(seed=14, many_gt=100, gt_max=5),
    dict(seed=15, crowd_p=0.25),
    dict(seed=16, json_area=True, crowd_p=0.1),
    dict(seed=17, empty_p=0.35),
    dict(seed=18, foreign_classes=True, zero_area=True),
    dict(seed=19, n_images=1, gt_max=12, det_max=120, tie_scores=True),
    dict(seed=20, n_images=2000, gt_max=4, det_max=8, crowd_p=0.05, json_area=True, tie_scores=True, empty_p=0.1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", SPLITS, ids=["s%d" % k["seed"] for k in SPLITS])
def test_device_arrays_equal_host(kw):
    from ubteacher.evaluation import coco_box_eval
    from ubteacher.evaluation.coco_eval_device import device_box_eval
    kw = dict(kw)
    n = kw.pop("n_images", 40)
    pred, gt = make_split(n_images=n, **kw)
    p_host, r_host, s_host = coco_box_eval(pred, gt, 6)
    p_dev, r_dev, s_dev = device_box_eval(pred, gt, 6)
    assert np.array_equal(p_dev, p_host), np.argwhere(p_dev != p_host)[:8]
    assert np.array_equal(r_dev, r_host), np.argwhere(r_dev != r_host)[:8]
    for k, v in s_host.items():
        assert s_dev[k] == v or (math.isnan(v) and math.isnan(s_dev[k])), k


def _outputs_for(dicts, shift, seed=0):
    from ubteacher.d2.structures import Boxes, Instances
    from ubteacher.data.dataset_mapper import to_xyxy_abs
    g = torch.Generator().manual_seed(seed)
    ins, outs = [], []
    for d in dicts:
        keep = [a for a in d["annotations"] if not a["iscrowd"]]
        inst = Instances((d["height"], d["width"]))
        b = torch.tensor([to_xyxy_abs(a) for a in keep], dtype=torch.float32).reshape(-1, 4)
        inst.pred_boxes = Boxes((b + shift * torch.rand(b.shape, generator=g)).cuda())
        inst.scores = torch.linspace(0.9, 0.5, len(keep)).cuda()
        inst.pred_classes = torch.tensor([a["category_id"] for a in keep], dtype=torch.int64).cuda()
        ins.append({"image_id": d["image_id"], "height": d["height"], "width": d["width"]})
        outs.append({"instances": inst})
    return ins, outs


@pytest.mark.gpu
def test_dataset_ground_truth_equals_host_evaluator_and_names_classes(tiny):  # noqa: F811
    from ubteacher.data import DatasetCatalog
    from ubteacher.evaluation import COCOBoxEvaluator, DeviceCOCOBoxEvaluator
    name = tiny[0]
    dicts = DatasetCatalog.get(name)
    for shift in (0.0, 4.0):
        ins, outs = _outputs_for(dicts, shift)
        host, dev = COCOBoxEvaluator(4, dataset_name=name), DeviceCOCOBoxEvaluator(4, dataset_name=name)
        host.process(ins, outs)
        dev.process(ins, outs)
        rh, rd = host.evaluate()["bbox"], dev.evaluate()["bbox"]
        for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"):
            assert rd[k] == rh[k], (k, rd[k], rh[k])
        assert {"AP-person", "AP-dog", "AP-bottle", "AP-toothbrush"} <= set(rd)
        assert {"AR1", "AR10", "AR100", "ARs", "ARm", "ARl"} <= set(rd)
    assert rd["AP"] < 100.0


@pytest.mark.gpu
def test_default_config_keeps_the_host_evaluator():
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.evaluation import COCOBoxEvaluator, DeviceCOCOBoxEvaluator
    from tests.utv2_testutil import small_fcos_cfg
    cfg = small_fcos_cfg()
    assert cfg.TEST.EVALUATOR == "COCOeval"
    assert type(UBTeacherTrainer.build_evaluator(cfg, "synthetic_val")) is COCOBoxEvaluator
    cfg.TEST.EVALUATOR = "COCOeval_device"
    assert type(UBTeacherTrainer.build_evaluator(cfg, "synthetic_val")) is DeviceCOCOBoxEvaluator


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fcos", "rcnn"])
def test_trainer_test_with_the_device_evaluator(tiny, kind):  # noqa: F811
    from tests.utv2_testutil import small_fcos_cfg
    from ubteacher.engine import UBRCNNTeacherTrainer, UBTeacherTrainer
    from ubteacher.evaluation import DeviceCOCOBoxEvaluator
    from ubteacher.presets import get_config
    name = tiny[0]
    if kind == "fcos":
        cfg, T = small_fcos_cfg(), UBTeacherTrainer
    else:
        cfg = get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0, "MODEL.DEVICE", "cuda"])
        T = UBRCNNTeacherTrainer
    cfg.DATASETS.TEST = (name,)
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 96, 160
    cfg.TEST.EVALUATOR = "COCOeval_device"
    assert isinstance(T.build_evaluator(cfg, name), DeviceCOCOBoxEvaluator)
    torch.manual_seed(0)
    tr = T(cfg)
    res = T.test(cfg, tr.model_teacher)
    keys = set(res["bbox"])
    assert {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"} <= keys
    nc = cfg.MODEL.ROI_HEADS.NUM_CLASSES if kind == "rcnn" else cfg.MODEL.FCOS.NUM_CLASSES
    assert len([k for k in keys if k.startswith("AP-")]) == nc and "AP-person" in keys
    assert res["_speed"]["images"] >= 1


def _instances_batch(pred, gt, ids):
    from ubteacher.d2.structures import Boxes, Instances
    ins, outs = [], []
    for iid in ids:
        g, p = gt[iid], pred[iid]
        gi = Instances((800, 800))
        gi.gt_boxes = Boxes(torch.tensor(g["boxes"], dtype=torch.float32).reshape(-1, 4).cuda())
        gi.gt_classes = torch.tensor(g["classes"], dtype=torch.int64).cuda()
        pi = Instances((800, 800))
        pi.pred_boxes = Boxes(torch.from_numpy(p["boxes"]).reshape(-1, 4).cuda())
        pi.scores = torch.from_numpy(p["scores"]).cuda()
        pi.pred_classes = torch.from_numpy(p["classes"]).cuda()
        ins.append({"image_id": iid, "instances": gi})
        outs.append({"instances": pi})
    return ins, outs


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ubteacher.evaluation import DeviceCOCOBoxEvaluator
        torch.cuda.set_device(0)
        pred, gt = make_split(seed=31, n_images=60, tie_scores=True)
        ids = list(gt)
        half = (len(ids) + 1) // 2
        mine = ids[:half] if rank == 0 else ids[half:]
        ev = DeviceCOCOBoxEvaluator(6)
        ev.process(*_instances_batch(pred, gt, mine))
        res = ev.evaluate()
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_give_the_one_rank_result():
    from ubteacher.evaluation import DeviceCOCOBoxEvaluator
    pred, gt = make_split(seed=31, n_images=60, tie_scores=True)
    ev = DeviceCOCOBoxEvaluator(6)
    ev.process(*_instances_batch(pred, gt, list(gt)))
    want = ev.evaluate()["bbox"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r, out = q.get(timeout=240)
            res[r] = out
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    assert res[1] == {}
    got = res[0]["bbox"]
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == v or (math.isnan(v) and math.isnan(got[k])), k
