"""Whole UTv2 steps with the deeper and grouped backbones (MODEL.RESNETS.DEPTH 101, the ResNeXt X-101-32x8d with STRIDE_IN_1X1 False)
against the CPU oracle.  The oracle's detectors call its module-level `resnet50` when they run, so the tests swap in a Detectron2
ResNet / ResNeXt restated here (depth and groups read off the state dict, grouped conv2 through F.conv2d(groups=...)); oracle/ is not
touched.  Bounds: those of test_fcos_step_gpu.py::test_full_semisup_step_parity / test_rcnn_step_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import utv2_oracle as O
from tests.utv2_testutil import FixedLoader, cpu_state, make_batch, rcnn_tune, small_fcos_cfg, tune_state_for_pseudo_labels

pytestmark = pytest.mark.gpu
H, W = 96, 128

VARIANTS = {
    "R-101": dict(DEPTH=101),
    "X-101-32x8d": dict(DEPTH=101, NUM_GROUPS=32, WIDTH_PER_GROUP=8, STRIDE_IN_1X1=False),
}


def general_resnet(stride_in_1x1):
    """D2 build_resnet_backbone (bottleneck blocks, FrozenBN) for any depth / groups found in the state dict"""
    def resnet(sd, x, prefix, out_features):
        outs = {}
        x = F.conv2d(x, sd[prefix + ".stem.conv1.weight"], None, 2, 3)
        x = F.relu(O.frozen_bn(x, sd, prefix + ".stem.conv1.norm"))
        x = F.max_pool2d(x, 3, 2, 1)
        for si in range(4):
            name = "res%d" % (si + 2)
            b = 0
            while "%s.%s.%d.conv1.weight" % (prefix, name, b) in sd:
                p = "%s.%s.%d" % (prefix, name, b)
                stride = 2 if (b == 0 and si > 0) else 1
                s1, s2 = (stride, 1) if stride_in_1x1 else (1, stride)
                if (p + ".shortcut.weight") in sd:
                    sc = O.frozen_bn(F.conv2d(x, sd[p + ".shortcut.weight"], None, stride), sd, p + ".shortcut.norm")
                else:
                    sc = x
                w2 = sd[p + ".conv2.weight"]
                o = F.relu(O.frozen_bn(F.conv2d(x, sd[p + ".conv1.weight"], None, s1), sd, p + ".conv1.norm"))
                o = F.relu(O.frozen_bn(F.conv2d(o, w2, None, s2, 1, 1, w2.shape[0] // w2.shape[1]), sd, p + ".conv2.norm"))
                o = O.frozen_bn(F.conv2d(o, sd[p + ".conv3.weight"], None, 1), sd, p + ".conv3.norm")
                x = F.relu(o + sc)
                b += 1
            if name in out_features:
                outs[name] = x
        return outs
    return resnet


def _apply(cfg, spec):
    for k, v in spec.items():
        setattr(cfg.MODEL.RESNETS, k, v)
    return cfg


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def normerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _gap_threshold(values, lo=0.35, hi=0.65):
    """a threshold in the middle of the widest gap between consecutive sorted values around the median (as in test_fcos_step_gpu.py):
    a deeper random-init teacher may put a detection right at the config's threshold, where 1e-6-level differences between the two
    implementations decide the pseudo set"""
    v = torch.sort(values.double().flatten())[0]
    a, b = int(lo * (len(v) - 1)), max(int(hi * (len(v) - 1)), int(lo * (len(v) - 1)) + 1)
    gaps = v[a + 1:b + 1] - v[a:b]
    i = int(torch.argmax(gaps)) + a
    return float((v[i] + v[i + 1]) / 2)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_fcos_step_parity(name, monkeypatch):
    from ubteacher.engine import UBTeacherTrainer
    spec = VARIANTS[name]
    monkeypatch.setattr(O, "resnet50", general_resnet(spec.get("STRIDE_IN_1X1", True)))
    cfg = _apply(small_fcos_cfg(), spec)
    torch.manual_seed(0)
    prod, orac = make_batch(12, 2, 2, H, W, "cuda")
    tr = UBTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    assert len(tr.model.backbone.bottom_up.stages[2][1]) == 23
    sd_s = tune_state_for_pseudo_labels(cpu_state(tr.model), [d["image"] for d in orac[3]])
    sd_t = dict(sd_s)
    sd_t["proposal_generator.fcos_head.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    S = cfg.SEMISUPNET
    with torch.no_grad():
        t_sd = O.ema_update(sd_s, sd_t, S.EMA_KEEP_RATE)
        tl = O.fcos_forward(t_sd, [d["image"] for d in orac[3]], sd_s["pixel_mean"], sd_s["pixel_std"])
        S.BBOX_THRESHOLD = _gap_threshold(torch.cat([d["cls_confid"] for d in O.fcos_predict(O.FCOSCfg(), *tl[:4], tl[4], tl[5], "cls")]))
        S.BBOX_THRESHOLD_REG = _gap_threshold(torch.cat([d["cls_confid"] for d in O.fcos_predict(O.FCOSCfg(), *tl[:4], tl[4], tl[5],
                                                                                              "cls_n_loc")]), 0.2, 0.5)
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    rec_o, new_s, new_t, grads, bufs, pseudo = O.fcos_semisup_step(
        O.FCOSCfg(), sd_s, sd_t, orac, keep_rate=cfg.SEMISUPNET.EMA_KEEP_RATE, lam_u=cfg.SEMISUPNET.UNSUP_LOSS_WEIGHT,
        lam_r=cfg.SEMISUPNET.UNSUP_REG_LOSS_WEIGHT, thr_cls=S.BBOX_THRESHOLD, thr_reg=S.BBOX_THRESHOLD_REG, lr=0.01, momentum=0.9, wd=1e-4,
        mean=sd_s["pixel_mean"], pix_std=sd_s["pixel_std"], frozen_prefixes=("backbone.bottom_up.stem", "backbone.bottom_up.res2"))
    assert sum(len(p["boxes"]) for p in pseudo[0]) > 0 and sum(len(p["boxes"]) for p in pseudo[1]) > 0
    assert "backbone.bottom_up.res4.22.conv2.weight" in grads
    pc, pr = tr._last_pseudo
    for i, p in enumerate(pseudo[0]):
        assert int(pc["valid"][i].sum()) == len(p["boxes"])
    for i, p in enumerate(pseudo[1]):
        assert int(pr["valid"][i].sum()) == len(p["boxes"])
    for k, v in rec_o.items():
        assert k in rec, k
        assert abs(rec[k] - v) <= 1e-3 * max(abs(v), 1e-6), (k, rec[k], v)
    s_after, t_after = cpu_state(tr.model), cpu_state(tr.model_teacher)
    for k in new_s:
        err = float((s_after[k].double() - new_s[k].double()).abs().max())
        upd = float((new_s[k].double() - sd_s[k].double()).abs().max())
        assert err <= 1e-4 * float(new_s[k].abs().max()) + 3e-3 * upd + 1e-12, k
    for k in new_t:
        assert torch.equal(t_after[k], new_t[k]), k
    checked = 0
    for k, (p, gview) in tr.model.store.trainable_named().items():
        if k in grads and grads[k].abs().max() > 0:
            if k.startswith("backbone.bottom_up"):
                # 1e-2 as for R-50, in the norm: 20 more random-init blocks than R-50 flip more ReLU gates on 1e-6-level forward
                # differences, which moves single elements of a deep layer's gradient (measured: up to 1.4e-2 of its max in res4)
                assert normerr(gview, grads[k]) < 1e-2 and relerr(gview, grads[k]) < 3e-2, k
            else:       # the heads see the deeper backbone's feature differences too (measured: up to 3.2e-3 against R-50's 3e-3)
                assert relerr(gview, grads[k]) < 5e-3, k
            checked += 1
    assert checked > 100


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_rcnn_step_parity(name, monkeypatch):
    from ubteacher.engine import UBRCNNTeacherTrainer
    from ubteacher.presets import get_config
    spec = VARIANTS[name]
    monkeypatch.setattr(O, "resnet50", general_resnet(spec.get("STRIDE_IN_1X1", True)))
    nb = 1
    cfg = _apply(get_config("rcnn", 1, ["SOLVER.IMG_PER_BATCH_LABEL", nb, "SOLVER.IMG_PER_BATCH_UNLABEL", nb, "SEMISUPNET.BURN_UP_STEP", 0,
                                        "MODEL.DEVICE", "cuda"]), spec)
    torch.manual_seed(0)
    prod, orac = make_batch(31, nb, nb, H, W, "cuda")
    tr = UBRCNNTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(3, 1, 1)
    pstd = torch.tensor(cfg.MODEL.PIXEL_STD).view(3, 1, 1)
    sd_s = rcnn_tune(cpu_state(tr.model), [d["image"] for d in orac[3]], mean, pstd)
    sd_t = dict(sd_s)
    sd_t["roi_heads.box_predictor.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    with torch.no_grad():
        dets, _ = O.rcnn_teacher(O.ema_update(sd_s, sd_t, cfg.SEMISUPNET.EMA_KEEP_RATE), [d["image"] for d in orac[3]], mean, pstd, thr=-1.0)
    cfg.SEMISUPNET.BBOX_THRESHOLD = _gap_threshold(torch.cat([d["scores"] for d in dets]))
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    g = torch.Generator().manual_seed(99)
    rpn_keys, roi_keys = [], []

    def rpn_src(n, m, device):
        k = torch.rand(n, m, generator=g)
        rpn_keys.append(k)
        return k.to(device)

    def roi_src(n, m, device):
        k = torch.rand(n, m, generator=g)
        roi_keys.append(k)
        return k.to(device)

    tr.model.proposal_generator.sample_keys = rpn_src
    tr.model.roi_heads.sample_keys = roi_src
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    O.FAST_ROI_ALIGN[0] = True      # the oracle's separable RoIAlign, as in test_rcnn_step_gpu.py's separable_roi_align fixture
    try:
        _rcnn_oracle_checks(cfg, nb, orac, sd_s, sd_t, rec, rpn_keys, roi_keys, tr, mean, pstd)
    finally:
        O.FAST_ROI_ALIGN[0] = False


def _rcnn_oracle_checks(cfg, nb, orac, sd_s, sd_t, rec, rpn_keys, roi_keys, tr, mean, pstd):
    post = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN

    def compact_roi(keys, nprops, ngts):
        return [torch.cat((keys[i, :nprops[i]], keys[i, post:post + ngts[i]])) for i in range(keys.shape[0])]

    t_sd = O.ema_update(sd_s, sd_t, cfg.SEMISUPNET.EMA_KEEP_RATE)
    with torch.no_grad():
        pseudo, _ = O.rcnn_teacher(t_sd, [d["image"] for d in orac[3]], mean, pstd, thr=cfg.SEMISUPNET.BBOX_THRESHOLD)
        _, props_sup, _ = O.rcnn_student_losses(sd_s, [d["image"] for d in orac[0] + orac[1]], [d["gt"] for d in orac[0] + orac[1]],
                                                rpn_keys[0], [torch.zeros(2000)] * (2 * nb), False, mean, pstd)
        _, props_uns, _ = O.rcnn_student_losses(sd_s, [d["image"] for d in orac[2]], pseudo, rpn_keys[1], [torch.zeros(2000)] * nb,
                                                True, mean, pstd)
    assert sum(len(p["boxes"]) for p in pseudo) > 0, "test setup: teacher produced no pseudo boxes"
    gl = tr._last_pseudo
    for i, p in enumerate(pseudo):
        assert int(gl["valid"][i].sum()) == len(p["boxes"])
    keys = dict(rpn_sup=rpn_keys[0], rpn_unsup=rpn_keys[1],
                roi_sup=compact_roi(roi_keys[0], [len(p["boxes"]) for p in props_sup], [len(d["gt"]["boxes"]) for d in orac[0] + orac[1]]),
                roi_unsup=compact_roi(roi_keys[1], [len(p["boxes"]) for p in props_uns], [len(p["boxes"]) for p in pseudo]))
    rec_o, new_s, new_t, grads, _ = O.rcnn_semisup_step(sd_s, sd_t, orac, keys, keep_rate=cfg.SEMISUPNET.EMA_KEEP_RATE,
                                                       lam_u=cfg.SEMISUPNET.UNSUP_LOSS_WEIGHT, lam_r=cfg.SEMISUPNET.UNSUP_REG_LOSS_WEIGHT,
                                                       thr=cfg.SEMISUPNET.BBOX_THRESHOLD, lr=0.01, mean=mean, pix_std=pstd)
    for k, v in rec_o.items():
        assert k in rec, k
        # as in test_rcnn_full_semisup_step_parity; loss_rpn_cls_pseudo too sums over anchors labelled by the matcher against pseudo
        # boxes that differ by 1e-5 between the two teachers - with R-101's deeper random-init features measured at 3.9e-3
        tol = 2e-2 if k == "loss_rpn_loc_pseudo" else 5e-3 if k == "loss_rpn_cls_pseudo" else 1e-3
        assert abs(rec[k] - v) <= tol * max(abs(v), 1e-6), (k, rec[k], v)
    t_after, s_after = cpu_state(tr.model_teacher), cpu_state(tr.model)
    for k in new_t:
        assert torch.equal(t_after[k], new_t[k]), k
    for k in new_s:
        err = float((s_after[k].double() - new_s[k].double()).abs().max())
        upd = float((new_s[k].double() - sd_s[k].double()).abs().max())
        assert err <= 1e-4 * float(new_s[k].abs().max()) + 4e-2 * upd + 1e-12, k


def _fcos_step_losses(spec, amp, seen=None):
    from ubteacher import ops
    from ubteacher.engine import UBTeacherTrainer
    cfg = _apply(small_fcos_cfg(), spec)
    cfg.SOLVER.AMP.ENABLED = amp
    torch.manual_seed(0)
    prod, orac = make_batch(12, 2, 2, H, W, "cuda")
    tr = UBTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    sd_s = tune_state_for_pseudo_labels(cpu_state(tr.model), [d["image"] for d in orac[3]])
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_s)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = 0.01
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    assert ops.PRECISION[0] == ("fp16" if amp else "fp32")
    if seen is not None:
        for name, blocks, trainable in tr.model.backbone.bottom_up.stages:
            if name != "res2":
                assert trainable and all(id(b) in seen for b in blocks), name   # the fused AMP node ran every block of res3-res5
    return {k: v for k, v in rec.items() if k.startswith("loss")}


def test_x101_fp16_step_fused_and_close_to_fp32(monkeypatch):
    """An fp16 AMP step of X-101 runs res3-res5 through the fused bottleneck node (grouped conv2, stride on conv2); its losses deviate from
    the fp32 step on the same batch by no more than twice what the R-50 step's deviate (floor 1e-3)"""
    monkeypatch.setenv("UTV2_PRECISION", "fp16")
    monkeypatch.setattr(O, "resnet50", general_resnet(False))     # tune_state_for_pseudo_labels runs the oracle's forward
    from ubteacher import ops
    seen = set()
    orig = ops._BottleneckFn.apply

    def spy(x, hk, block):
        seen.add(id(block))
        return orig(x, hk, block)

    try:
        r50 = {amp: _fcos_step_losses({}, amp) for amp in (False, True)}
        monkeypatch.setattr(ops._BottleneckFn, "apply", spy)
        x101 = {False: _fcos_step_losses(VARIANTS["X-101-32x8d"], False), True: _fcos_step_losses(VARIANTS["X-101-32x8d"], True, seen)}
    finally:
        ops.set_precision("fp32")

    def dev(r):
        return max(abs(r[True][k] - r[False][k]) / max(abs(r[False][k]), 1e-6) for k in r[False] if abs(r[False][k]) > 1e-6)
    assert all(np.isfinite(v) for r in (r50, x101) for d in r.values() for v in d.values())
    assert dev(x101) <= 2 * max(dev(r50), 1e-3), (dev(x101), dev(r50))


def test_x101_step_as_hipgraph_equals_eager(monkeypatch):
    """run_step_graph with the X-101 backbone: two eager steps, capture, three replays - the same losses and weights as five eager steps"""
    monkeypatch.setenv("UTV2_PRECISION", "bf16")
    from ubteacher import ops
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    import bench
    cfg = _apply(get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                        "SOLVER.AMP.ENABLED", True, "MODEL.DEVICE", "cuda"]), VARIANTS["X-101-32x8d"])
    outs = []
    try:
        for graph in (False, True):
            torch.manual_seed(0)
            tr = UBTeacherTrainer(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=96, width=128))
            bench.tune_for_pseudo_labels(tr, tr._data_loader.batches[0])
            tr.iter, tr.log_period = 1, 10 ** 9
            tr.optimizer.param_groups[0]["lr"] = 1e-3
            recs = []
            for _ in range(5):
                (tr.run_step_graph if graph else tr.run_step_full_semisup)()
                tr.iter += 1
                recs.append(dict(tr.flush_metrics()))
            torch.cuda.synchronize()
            if graph:
                assert tr._step_graphs and all(st["graph"] is not None for st in tr._step_graphs.values())
            outs.append((recs, tr.model.flat_state().clone(), tr.model_teacher.flat_state().clone()))
    finally:
        ops.STEP_GRAPH[0] = False
        ops.set_precision("fp32")
    (ra, sa, ta), (rb, sb, tb) = outs
    for a, b in zip(ra, rb):
        for k, v in a.items():
            if k.startswith("loss"):
                assert v == v and abs(b[k] - v) <= 1e-4 * max(abs(v), 1e-3), (k, v, b[k])
    assert torch.isfinite(sa).all() and torch.isfinite(sb).all()
    assert float((sa - sb).abs().max()) <= 1e-4 * float(sa.abs().max()) and float((ta - tb).abs().max()) <= 1e-4 * float(ta.abs().max())


def test_frozen_grouped_res2_declines_the_fused_frozen_kernel(monkeypatch):
    """X-101's frozen res2 (grouped conv2, 256-wide) runs per conv: the fused frozen-block kernel (64-channel intermediates in LDS) is
    never called for it, while the R-50 res2 keeps using it"""
    monkeypatch.setenv("UTV2_PRECISION", "bf16")
    from ubteacher import hip, ops
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    calls = []
    orig = hip.bottleneck_fwd_bf16
    monkeypatch.setattr(hip, "bottleneck_fwd_bf16", lambda *a, **k: calls.append(1) or orig(*a, **k))
    try:
        ops.set_precision("bf16")
        for spec, want in (({}, 3), (VARIANTS["X-101-32x8d"], 0)):
            cfg = _apply(get_config("fcos", 1, ["MODEL.DEVICE", "cuda"]), spec)
            torch.manual_seed(0)
            m = build_model(cfg)
            m.folder.fold()
            blocks = m.backbone.bottom_up.stages[0][1]
            x = torch.randn(2, 24, 32, 64, device="cuda").relu().to(hip.h16_dtype())
            del calls[:]
            with torch.no_grad():
                for b in blocks:
                    x = b(x)
            torch.cuda.synchronize()
            assert len(calls) == want and torch.isfinite(x.float()).all()
    finally:
        ops.set_precision("fp32")
