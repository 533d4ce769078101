"""N>1 host logic on CPU: world_size-2 gloo process groups (one process per rank) exercise the pieces
of the data-parallel step that do not need a GPU: the flat gradient all-reduce + 1/world scaling, the
fused [num_pos, sum ctrness] normaliser all-reduce, per-rank batch sharding of the loader, and the
rank-0 metric gather/averaging."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, received):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ubteacher.engine.trainer import _TrainerBase
    from ubteacher.modeling.fcos import FCOSOutputs
    from ubteacher.presets import get_config
    from ubteacher.utils import comm
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    out = {}
    # (1) flat gradient all-reduce: SUM then the optimizer's 1/world scale == DDP mean
    class Store:
        pass
    class Model:
        pass
    tr = _TrainerBase.__new__(_TrainerBase)
    tr.world_size = comm.get_world_size()
    tr.model = Model(); tr.model.store = Store()
    g = torch.Generator().manual_seed(100 + rank)
    tr.model.store.grad = torch.randn(1000, generator=g)
    local = tr.model.store.grad.clone()
    scale = tr._allreduce_grads()
    out["grad_mean"] = (tr.model.store.grad * scale)
    out["local"] = local
    # (2) fused loss normalisers
    sums = torch.tensor([3.0 + rank, 1.5 * (rank + 1), 0, 0, 0, 0, 0, 0])
    npa, den = FCOSOutputs._normalisers(sums)
    out["npa"], out["den"] = float(npa), float(den)
    sums0 = torch.zeros(8)
    npa0, den0 = FCOSOutputs._normalisers(sums0)
    out["npa0"], out["den0"] = float(npa0), float(den0)
    # (2b) a rank running the fused student pass next to a rank running the two passes (their image lists pad to different canvases):
    # the fused path's normaliser reduction must be the same three collectives the per-pass path issues, in the same order
    trio = [torch.tensor([1.0 + rank + 10 * i, 0.5 * (rank + 1) + i, 0, 0, 0, 0, 0, 0]) for i in range(3)]
    if rank == 0:
        out["joint"] = FCOSOutputs._joint_normaliser_sums(*trio).tolist()
    else:
        pairs = [FCOSOutputs._normalisers(t) for t in trio]
        out["joint"] = [float(v) * 2 for pr in pairs for v in pr]      # _normalisers returns world means (clamps inactive here)
    # (3) loader sharding
    cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 4, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "MODEL.DEVICE", "cpu"])
    ld = SyntheticTwoCropLoader(cfg, height=32, width=48, device="cpu")
    lq, lk, uq, uk = next(iter(ld))
    out["sizes"] = (len(lq), len(lk), len(uq), len(uk))
    out["img0"] = lk[0]["image"].clone()
    # (4) metric gather on rank 0
    tr.model.device = torch.device("cpu")
    tr.iter = 0; tr.storage = None; tr._pending_metrics = None; tr._last_metrics = {}
    tr.log_period = 1
    tr._write_metrics({"loss_a": torch.tensor(1.0 + rank), "loss_b": 2.0 * (rank + 1), "data_time": 0.1 * (rank + 1), "other": 7.0})
    out["metrics"] = tr._last_metrics
    # (5) bucketed, backward-overlapped all-reduce of the gradient arena == one flat all-reduce
    from ubteacher.utils.grad_sync import GradBuckets

    class H:
        def __init__(self, offset, numel, g):
            self.offset, self.numel, self.g = offset, numel, g
    gflat = torch.randn(5000, generator=torch.Generator().manual_seed(7 + rank))
    ref = gflat.clone()
    sizes, hs, off = [700, 300, 1200, 40, 900, 1000, 860], [], 0
    for n in sizes:
        hs.append(H(off, n, gflat[off:off + n])); off += n
    gb = GradBuckets(gflat, hs, bucket_bytes=4 * 1000)
    out["nbuckets"] = len(gb.bounds)
    out["cover"] = (gb.bounds[0][0], gb.bounds[-1][1], all(gb.bounds[i][1] == gb.bounds[i + 1][0] for i in range(len(gb.bounds) - 1)))
    gb.on_forward(hs)          # every layer used once ...
    gb.on_forward(hs[2:4])     # ... two of them twice (a second student pass)
    gb.arm()
    early = []
    for h in reversed(hs):     # backward reports in reverse order
        gb.on_backward_done([h])
        early.append(sum(gb.launched))
    out["launched_before_finish"] = sum(gb.launched)
    gb.on_backward_done(hs[2:4])
    out["launched_after_second_pass"] = sum(gb.launched)
    gb.finish()
    dist.all_reduce(ref, op=dist.ReduceOp.SUM)
    out["bucketed_equals_flat"] = bool(torch.equal(gflat, ref))
    out["reset"] = (sum(gb.pending), sum(gb.launched), len(gb.works))
    out["order"] = list(gb.last_order)
    # ranks whose writers differ (rank 1 runs an extra, unfused pass over two layers) and whose backward completes the layers in
    # different orders must still issue the bucket collectives in the same (static, descending) order
    g2 = torch.randn(5000, generator=torch.Generator().manual_seed(70 + rank))
    ref2 = g2.clone()
    gflat.copy_(g2)
    gb.on_forward(hs)
    if rank == 1:
        gb.on_forward(hs[:2])
    gb.arm()
    for h in (list(reversed(hs)) if rank == 0 else hs):
        gb.on_backward_done([h])
    if rank == 1:
        gb.on_backward_done(hs[:2])
    gb.finish()
    dist.all_reduce(ref2, op=dist.ReduceOp.SUM)
    out["order2"] = list(gb.last_order)
    out["bucketed_equals_flat2"] = bool(torch.equal(gflat, ref2))
    # (6) the two-crop loader over a registered dataset: the label / unlabel split by the seed table, TrainingSampler streams whose
    # seed is shared by the ranks (comm.shared_random_seed) and rank-strided, per-rank batch sizes = total // world (host logic only:
    # an identity mapper stands in for the GPU one)
    import itertools
    from ubteacher.data import DatasetCatalog, build_detection_semisup_train_loader_two_crops, register_synthetic
    if "gloo_ds" in DatasetCatalog:
        DatasetCatalog.remove("gloo_ds")
    register_synthetic("gloo_ds", 50, seed=5)
    cfg2 = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 4, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "MODEL.DEVICE", "cpu"])
    cfg2.DATASETS.TRAIN = ("gloo_ds",)
    cfg2.DATASETS.CROSS_DATASET = False
    cfg2.DATALOADER.SUP_PERCENT = 30.0
    cfg2.DATALOADER.RANDOM_DATA_SEED = 0
    cfg2.DATALOADER.RANDOM_DATA_SEED_PATH = os.path.join(ROOT, "tests", "golden", "supervision_small.json")
    cfg2.DATALOADER.FILTER_EMPTY_ANNOTATIONS = False
    ident = lambda d: ({"image_id": d["image_id"], "width": d["width"], "height": d["height"], "v": "s"},
                       {"image_id": d["image_id"], "width": d["width"], "height": d["height"], "v": "w"})
    loader = build_detection_semisup_train_loader_two_crops(cfg2, mapper=ident)
    seq = []
    for lq, lk, uq, uk in itertools.islice(iter(loader), 6):
        seq.append(([d["image_id"] for d in lq], [d["image_id"] for d in uq], len(lk), len(uk)))
    out["loader_seq"] = seq
    out["label_stream"] = list(itertools.islice(iter(loader.label_dataset.sampler), 12))
    # (5) ADVICE r4: the test loader shards the set over the ranks; COCOBoxEvaluator.evaluate() gathers every rank's predictions and
    # ground truth on the main rank (Detectron2 COCOEvaluator(distributed=True)) - rank 0 reports the AP of the WHOLE set, the others {}
    import numpy as np
    from ubteacher.evaluation.coco_eval import COCOBoxEvaluator, coco_box_ap
    def _img(i):
        b = np.array([[10.0 + i, 10.0, 60.0 + i, 50.0]])
        gt = dict(boxes=b, classes=np.array([i % 2]))
        # image 1's detection has the wrong class: the whole-set AP differs from either shard's
        pr = dict(boxes=b.copy(), scores=np.array([0.9 - 0.1 * i]), classes=np.array([0]))
        return gt, pr
    ev = COCOBoxEvaluator(num_classes=2)
    for i in range(4):
        if i % world == rank:                                       # InferenceSampler-style shard
            ev._gt[i], ev._pred[i] = _img(i)
    out["eval"] = ev.evaluate()
    whole_gt, whole_pr = {}, {}
    for i in range(4):
        whole_gt[i], whole_pr[i] = _img(i)
    out["eval_whole"] = {"bbox": coco_box_ap(whole_pr, whole_gt, 2)}
    q.put((rank, out))
    # the tensors in `out` travel as shared-memory handles that the parent fetches from THIS process while it unpickles them: stay alive
    # until the parent has both results (a rank that exits first takes its handle server with it and the parent's q.get fails)
    assert received.wait(300)
    dist.barrier()
    dist.destroy_process_group()


def test_world_size_2_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    received = ctx.Event()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, received)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    received.set()
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    mean = (res[0]["local"] + res[1]["local"]) / 2
    for r in range(world):
        assert torch.allclose(res[r]["grad_mean"], mean)          # identical averaged grads on every rank
        assert res[r]["npa"] == pytest.approx((3.0 + 4.0) / 2)      # == single-process value on the concatenated batch / world
        assert res[r]["den"] == pytest.approx((1.5 + 3.0) / 2)
        assert res[r]["npa0"] == 1.0 and res[r]["den0"] == pytest.approx(1e-6)   # clamps (fcos_outputs.py:321,362)
        # mixed fused / per-pass ranks: the same three collectives met each other (no hang, no mismatched sizes) and both see the world sums
        want = [v for i in range(3) for v in ((1.0 + 10 * i) + (2.0 + 10 * i), (0.5 + i) + (1.0 + i))]
        assert res[r]["joint"] == pytest.approx(want)
        assert res[r]["sizes"] == (2, 2, 1, 1)                      # IMG_PER_BATCH_* // world (data/build.py:240-241)
    assert not torch.equal(res[0]["img0"], res[1]["img0"])          # ranks see different images
    assert res[0]["eval"] == res[0]["eval_whole"] and res[1]["eval"] == {}     # dataset AP on the main rank only (gathered shards)
    assert 0.0 < res[0]["eval"]["bbox"]["AP"] < 100.0
    m = res[0]["metrics"]
    assert m["loss_a"] == pytest.approx(1.5) and m["loss_b"] == pytest.approx(3.0) and m["other"] == pytest.approx(7.0)
    assert m["total_loss"] == pytest.approx(4.5)                    # sum of averaged keys starting with "loss"
    assert res[1]["metrics"] == {}                                  # only the main process aggregates
    import json
    labeled = set(json.load(open(os.path.join(ROOT, "tests", "golden", "supervision_small.json")))["30.0"]["0"])
    for r in range(world):
        for lids, uids, nlk, nuk in res[r]["loader_seq"]:
            assert len(lids) == nlk == 2 and len(uids) == nuk == 1           # 4 // 2 labeled, 2 // 2 unlabeled per rank
            assert set(lids) <= labeled and not (set(uids) & labeled)
    # one shared permutation stream, rank-strided: interleaving the two ranks' index streams gives a sequence of permutations of range(15)
    inter = [res[i % 2]["label_stream"][i // 2] for i in range(24)]
    assert sorted(inter[:15]) == list(range(15)) and res[0]["label_stream"] != res[1]["label_stream"]
    for r in range(world):
        assert res[r]["nbuckets"] >= 3 and res[r]["cover"] == (0, 5000, True)
        assert 0 < res[r]["launched_before_finish"] < res[r]["nbuckets"]     # buckets with a layer still pending wait
        assert res[r]["launched_after_second_pass"] == res[r]["nbuckets"]
        assert res[r]["bucketed_equals_flat"] and res[r]["reset"] == (0, 0, 0)
        desc = list(range(res[r]["nbuckets"] - 1, -1, -1))
        assert res[r]["order"] == desc and res[r]["order2"] == desc and res[r]["bucketed_equals_flat2"]   # static launch order
