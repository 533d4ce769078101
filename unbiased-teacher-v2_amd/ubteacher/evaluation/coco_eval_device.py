"""COCO box evaluation of a whole split on the GPU (TEST.EVALUATOR "COCOeval_device"): the COCOBoxEvaluator surface (reset / process /
evaluate, ground truth from a registered set or riding on the inputs as `instances`), scored by the HIP kernels of csrc/coco_eval.hip.
The AP numbers are bit-identical to coco_box_ap's; the result also carries pycocotools' recall summary (AR1 / AR10 / AR100 / ARs / ARm /
ARl) and Detectron2 COCOEvaluator's per-class `AP-<name>` (evaluation/coco_eval.py:summarize).

process() keeps clones of the output tensors on the device (they may be views of buffers the next forward pass reuses) and neither
copies nor synchronises; evaluate() packs everything CSR by image in the evaluator's image order, gathers the ranks' packs on rank 0,
runs the kernels there and brings back only the small precision / recall arrays."""
import numpy as np
import torch

from .coco_eval import AREA_NAMES, AREA_RNG, IOU_THRS, MAX_DETS, REC_THRS, summarize

_DATASET_GT = {}   # dataset name -> packed ground truth of the registered set (packed and uploaded once per name and device)


def _box_areas(boxes):
    """(x2 - x1) * (y2 - y1) in fp64, _evaluate_image's expression for ground truth without an `area` field"""
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) if len(boxes) else np.zeros(0)


def _ragged_index(starts, lens):
    """the concatenation of arange(s, s + n) over (starts, lens), int64 numpy"""
    lens = np.asarray(lens, np.int64)
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    shift = np.asarray(starts, np.int64) - (np.cumsum(lens) - lens)
    return np.arange(total, dtype=np.int64) + np.repeat(shift, lens)


class _DatasetGT:
    """the ground truth of a registered set, CSR by the set's image order, on the device"""

    def __init__(self, dataset_name, device):
        from ..data import DatasetCatalog
        from ..data.dataset_mapper import to_xyxy_abs
        boxes, classes, crowd, area, lens, self.index = [], [], [], [], [], {}
        for d in DatasetCatalog.get(dataset_name):
            annos = d.get("annotations", [])
            b = np.asarray([to_xyxy_abs(a) for a in annos], float).reshape(-1, 4)
            # COCOBoxEvaluator ranks by the json `area` only when every annotation of the image has one, else by the box areas
            ar = np.asarray([a["area"] for a in annos], float) if annos and all("area" in a for a in annos) else _box_areas(b)
            self.index[d["image_id"]] = len(lens)
            boxes.append(b)
            classes.append(np.asarray([a["category_id"] for a in annos], np.int64).reshape(-1))
            crowd.append(np.asarray([a.get("iscrowd", 0) for a in annos], bool).reshape(-1))
            area.append(ar.reshape(-1))
            lens.append(len(annos))
        self.lens = np.asarray(lens, np.int64)
        self.starts = np.cumsum(self.lens) - self.lens
        self.max_class = int(max((int(c.max()) for c in classes if len(c)), default=-1))
        cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)  # noqa: E731
        self.boxes = torch.from_numpy(cat(boxes, (0, 4), np.float64).reshape(-1, 4)).to(device)
        self.classes = torch.from_numpy(cat(classes, 0, np.int32)).to(device)
        self.crowd = torch.from_numpy(cat(crowd, 0, np.uint8)).to(device)
        self.area = torch.from_numpy(cat(area, 0, np.float64)).to(device)


class DeviceCOCOBoxEvaluator:
    """COCOBoxEvaluator on the device; see the module docstring.  num_classes: the classes scored (0 .. num_classes - 1; None: up to the
    largest ground-truth class); dataset_name: a registered set whose dicts carry the ground truth (None: `instances` on the inputs)."""

    def __init__(self, num_classes=None, dataset_name=None, device=None):
        self.num_classes = num_classes
        self.dataset_name = dataset_name
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dataset_gt = None
        if dataset_name is not None:
            key = (dataset_name, str(self.device))
            if key not in _DATASET_GT:
                _DATASET_GT[key] = _DatasetGT(dataset_name, self.device)
            self._dataset_gt = _DATASET_GT[key]
        self.reset()

    def reset(self):
        self._ids = []      # image id per processed image, in process order
        self._det = []      # (boxes fp32 [D, 4], scores fp32 [D], classes [D]) clones on the device
        self._gt = []       # (boxes [G, 4], classes [G]) clones on the device (ground truth riding on the inputs)
        self.precision = self.recall = None     # the arrays of the last evaluate() on rank 0 (numpy [10, 101, K, 4] / [10, K, 4, 3])

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            inst = out["instances"] if "instances" in out else out["proposals"]
            self._ids.append(inp["image_id"])
            self._det.append((inst.pred_boxes.tensor.detach().to(self.device, torch.float32).clone().reshape(-1, 4),
                              inst.scores.detach().to(self.device, torch.float32).clone().reshape(-1),
                              inst.pred_classes.detach().to(self.device).clone().reshape(-1)))
            if self._dataset_gt is None:
                gt = inp["instances"]
                self._gt.append((gt.gt_boxes.tensor.detach().to(self.device).clone().reshape(-1, 4),
                                 gt.gt_classes.detach().to(self.device).clone().reshape(-1)))

    def _pack(self):
        """this rank's images packed: ids, per-image detection / ground-truth counts, concatenated tensors"""
        dev = self.device
        dlens = [int(b.shape[0]) for b, _, _ in self._det]
        det = (torch.cat([b for b, _, _ in self._det]) if self._det else torch.zeros((0, 4), device=dev),
               torch.cat([s for _, s, _ in self._det]) if self._det else torch.zeros(0, device=dev),
               torch.cat([c for _, _, c in self._det]).to(torch.int32) if self._det else torch.zeros(0, dtype=torch.int32, device=dev))
        pack = {"ids": list(self._ids), "dlens": dlens, "det": det}
        if self._dataset_gt is None:
            pack["glens"] = [int(b.shape[0]) for b, _ in self._gt]
            pack["gt"] = (torch.cat([b for b, _ in self._gt]).to(torch.float64) if self._gt else torch.zeros((0, 4), dtype=torch.float64, device=dev),
                          torch.cat([c for _, c in self._gt]).to(torch.int32) if self._gt else torch.zeros(0, dtype=torch.int32, device=dev))
        return pack

    def evaluate(self):
        """Detectron2 COCOEvaluator(distributed=True).evaluate: every rank's packs are gathered on rank 0 and merged there in rank order
        with dict.update semantics (an image seen twice keeps its first position and its last value, as COCOBoxEvaluator's dicts do);
        the other ranks return {}."""
        from ..utils import comm
        pack = self._pack()
        if comm.get_world_size() > 1:
            comm.synchronize()
            host = lambda t: tuple(x.cpu() for x in t)  # noqa: E731  (the packs travel pickled, as host tensors)
            pack["det"] = host(pack["det"])
            if "gt" in pack:
                pack["gt"] = host(pack["gt"])
            parts = comm.gather(pack, dst=0)
            if not comm.is_main_process():
                return {}
        else:
            parts = [pack]
        return {"bbox": self._score(parts)}

    def _score(self, parts):
        from .. import hip
        dev = self.device
        # dict.update order over the ranks: position of the first occurrence, value of the last
        where, ent = {}, 0
        for p in parts:
            for i, iid in enumerate(p["ids"]):
                where[iid] = ent + i
            ent += len(p["ids"])
        chosen = np.asarray(list(where.values()), np.int64)
        identity = len(chosen) == ent and bool(np.all(chosen == np.arange(ent)))
        N = len(chosen)

        def merged(key, lens_key):
            cat = [torch.cat([p[key][j].to(dev) for p in parts]) for j in range(len(parts[0][key]))]
            lens = np.concatenate([np.asarray(p[lens_key], np.int64) for p in parts]) if ent else np.zeros(0, np.int64)
            if identity:
                return cat, lens
            starts = np.cumsum(lens) - lens
            idx = torch.from_numpy(_ragged_index(starts[chosen], lens[chosen])).to(dev)
            return [t.index_select(0, idx) for t in cat], lens[chosen]

        def offsets(lens):
            return torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)

        (dbox, dscore, dcls), dlens = merged("det", "dlens")
        ids = list(where.keys())
        if self._dataset_gt is None:
            (gbox, gcls), glens = merged("gt", "glens")
            gcrowd = torch.zeros(gcls.shape[0], dtype=torch.uint8, device=dev)
            garea = None
            max_class = int(gcls.max()) if gcls.numel() and self.num_classes is None else -1
        else:
            ds = self._dataset_gt
            rows = np.asarray([ds.index[i] for i in ids], np.int64)
            glens = ds.lens[rows]
            idx = torch.from_numpy(_ragged_index(ds.starts[rows], glens)).to(dev)
            gbox, gcls, gcrowd, garea = (t.index_select(0, idx) for t in (ds.boxes, ds.classes, ds.crowd, ds.area))
            max_class = ds.max_class
        K = int(self.num_classes) if self.num_classes is not None else max_class + 1
        names = None
        if self.dataset_name is not None:
            from ..data import MetadataCatalog
            names = MetadataCatalog.get(self.dataset_name).thing_classes
        names = list(names)[:K] + [str(k) for k in range(len(names), K)] if names else [str(k) for k in range(max(K, 0))]
        if N == 0 or K <= 0:
            self.precision, self.recall = -np.ones((len(IOU_THRS), len(REC_THRS), max(K, 0), 4)), -np.ones((len(IOU_THRS), max(K, 0), 4, 3))
            return summarize(self.precision, self.recall, names)
        prec, rec = hip.coco_box_eval(dbox.contiguous(), dscore.contiguous(), dcls.contiguous(), offsets(dlens), gbox.contiguous(),
                                      gcrowd.contiguous(), None if garea is None else garea.contiguous(), gcls.contiguous(), offsets(glens), K,
                                      int(glens.max()) if len(glens) else 0, IOU_THRS, REC_THRS, [AREA_RNG[a] for a in AREA_NAMES],
                                      MAX_DETS)
        self.precision, self.recall = prec.cpu().numpy(), rec.cpu().numpy()      # kept for inspection (tools/bench_eval.py)
        return summarize(self.precision, self.recall, names)


def device_box_eval(predictions, ground_truth, num_classes, device=None):
    """coco_box_eval(predictions, ground_truth, num_classes) with the arrays computed by the kernels: the same host dicts (coco_box_ap's
    input format, images in ground_truth's order) packed CSR and uploaded.  Returns (precision, recall, stats) as numpy / dict."""
    from .. import hip
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    db, ds, dc, dl, gb, gc, gcr, ga, gl = [], [], [], [], [], [], [], [], []
    for img, g in ground_truth.items():
        b = np.asarray(g["boxes"], float).reshape(-1, 4)
        c = np.asarray(g["classes"]).reshape(-1)
        gb.append(b)
        gc.append(c)
        gcr.append(np.asarray(g.get("iscrowd", np.zeros(len(c))), bool).reshape(-1))
        ga.append(np.asarray(g["area"], float).reshape(-1) if g.get("area") is not None else _box_areas(b))
        gl.append(len(c))
        p = predictions.get(img)
        n = len(np.asarray(p["classes"]).reshape(-1)) if p is not None else 0
        if n:
            db.append(np.asarray(p["boxes"], np.float32).reshape(-1, 4))
            ds.append(np.asarray(p["scores"], np.float32).reshape(-1))
            dc.append(np.asarray(p["classes"]).reshape(-1))
        dl.append(n)
    up = lambda xs, shape, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt))).to(dev)  # noqa: E731
    off = lambda lens: torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)  # noqa: E731
    prec, rec = hip.coco_box_eval(up(db, (0, 4), np.float32).reshape(-1, 4), up(ds, 0, np.float32), up(dc, 0, np.int32), off(dl),
                                  up(gb, (0, 4), np.float64).reshape(-1, 4), up(gcr, 0, np.uint8), up(ga, 0, np.float64), up(gc, 0, np.int32),
                                  off(gl), num_classes, max(gl, default=0), IOU_THRS, REC_THRS, [AREA_RNG[a] for a in AREA_NAMES], MAX_DETS)
    prec, rec = prec.cpu().numpy(), rec.cpu().numpy()
    return prec, rec, summarize(prec, rec)
