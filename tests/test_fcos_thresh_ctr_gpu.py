"""MODEL.FCOS.THRESH_WITH_CTR on the device (csrc/fcos.hip: utv2_fcos_rank_keys_f / utv2_fcos_decode_f / utv2_fcos_decode_cont_f with
flags = UTV2_FCOS_THRESH_WITH_CTR) against the golden executed from the reference (tests/golden/thresh_ctr.npz) and, where the golden
has no case, against the torch restatement of tests/test_fcos_thresh_ctr.py (itself held to that golden to the bit).

Bounds.  Indices exact, no excluded case: the generator asserted that no product lies within 1e-5 (relative) of the threshold and no two
scores at a top-k / POST_NMS_TOPK boundary or IoU at NMS_TH lie within 1e-6, and two fp32 sigmoids of the device differ from torch's by
a few ulp (< 1e-6 relative).  cls_confid / scores: 1e-6 absolute (values <= 1: about 8 ulp).  centerness, std, boxes: the tolerances of
tests/test_fcos_kernels_gpu.py::test_decode_nms.  Step losses: the 1e-3 relative bound of tests/test_fcos_step_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_fcos_thresh_ctr import C, CRITERIA, HEADS, STRIDES, T, golden_level_inputs, load_gold, restate_level

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG = "failed with code"
BS = {"d": 80, "c": 16}          # box row pitch: 68 bins | std 4 | ctr 1 | pad; ltrb 4 | std 4 | ctr 1 | pad (modeling.fcos.BOX_STRIDE_CONT)


def close(a, b, rtol=1e-5, atol=1e-6):
    from tests.test_fcos_kernels_gpu import close as c
    c(a, b, rtol=rtol, atol=atol)


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def H():
    from ubteacher import hip
    return hip


def box_rows(head, reg, std, ctr):
    """NCHW head tensors of one level -> the product's box rows [N * h * w, BS]"""
    n = reg.shape[0] * reg.shape[2] * reg.shape[3]
    R = reg.shape[1]
    b = torch.zeros((n, BS[head]))
    b[:, :R] = reg.permute(0, 2, 3, 1).reshape(n, R)
    b[:, R:R + 4] = std.permute(0, 2, 3, 1).reshape(n, 4)
    b[:, R + 4] = ctr.permute(0, 2, 3, 1).reshape(n)
    return b


def fresh_outs(N, M):
    return dict(boxes=torch.full((N, M, 4), 9.0, device=DEV), scores=torch.full((N, M), 9.0, device=DEV),
                classes=torch.full((N, M), 9, dtype=torch.int32, device=DEV), locations=torch.full((N, M, 2), 9.0, device=DEV),
                centerness=torch.full((N, M), 9.0, device=DEV), cls_confid=torch.full((N, M), 9.0, device=DEV),
                reg_pred_std=torch.full((N, M, 4), 9.0, device=DEV), fpn_levels=torch.full((N, M), 9, dtype=torch.int32, device=DEV),
                valid=torch.full((N, M), 9, dtype=torch.uint8, device=DEV))


def run_level(head, logits, reg, std, ctr, stride, level, thr, topk, method, flags):
    """rank keys -> exact per-row top-k -> decode of one level through hip.py; NCHW inputs.  Returns (keys, top keys, outputs) on the host."""
    hip = H()
    N, nc, h, w = logits.shape
    lg = logits.permute(0, 2, 3, 1).reshape(-1, nc).contiguous().to(DEV)
    bx = box_rows(head, reg, std, ctr).to(DEV)
    reg_max = 16 if head == "d" else hip.REG_CONT
    keys = hip.fcos_rank_keys(lg, bx, reg_max, N, h * w, thr, method, flags=flags)
    width = h * w * nc
    k = min(topk, width)
    row_off = torch.arange(N + 1, dtype=torch.int64, device=DEV) * width
    top = hip.topk_rows(keys.view(-1), row_off, N, width, k)
    outs = fresh_outs(N, k)
    if head == "d":
        hip.fcos_decode(top, lg, bx, reg_max, N, h * w, w, stride, level, method, 0, outs, flags=flags)
    else:
        hip.fcos_decode_cont(top, lg, bx, N, h * w, w, stride, level, method, 0, outs, flags=flags)
    torch.cuda.synchronize()
    return keys.cpu(), top.cpu(), {k_: v.cpu() for k_, v in outs.items()}


def check_row(top, outs, i, want, level, nc=C):
    """image i of one level against `want` (flat, rank, scores, conf, ctr, boxes, std; any order): the same candidates - set equality, and
    the device's descending order must be the order of the expected ranking scores - and every decoded field of every slot"""
    tk = top[i]
    nv = int((tk >= 0).sum())
    assert nv == len(want["flat"]), (nv, len(want["flat"]))
    assert bool((tk[:nv] >= 0).all()) and bool((tk[nv:] == -1).all())
    flat = 0xFFFFFFFF - (tk[:nv] & 0xFFFFFFFF)
    wf = torch.as_tensor(want["flat"]).long()
    order = torch.argsort(wf)
    assert torch.equal(torch.sort(flat)[0], wf[order])
    pos = order[torch.searchsorted(wf[order], flat)]                       # slot of the device's k-th candidate in `want`
    rank = torch.as_tensor(want["rank"])[pos]
    assert bool((rank[:-1] > rank[1:]).all()), "device order is not the descending order of the expected ranking scores"
    o = {k: v[i] for k, v in outs.items()}
    assert torch.equal(o["valid"][:nv], torch.ones(nv, dtype=torch.uint8)) and not bool(o["valid"][nv:].any())
    assert bool((o["scores"][nv:] == -1).all())
    assert torch.equal(o["classes"][:nv].long(), flat % nc) and bool((o["fpn_levels"] == level).all())
    for name, key, tol in (("cls_confid", "conf", 1e-6), ("scores", "scores", 1e-6)):
        err = float((o[name][:nv].double() - torch.as_tensor(want[key])[pos].double()).abs().max()) if nv else 0.0
        assert err <= tol, (name, err)
    if nv:
        close(o["centerness"][:nv], torch.as_tensor(want["ctr"])[pos], rtol=2e-5)
        close(o["reg_pred_std"][:nv], torch.as_tensor(want["std"])[pos])
        close(o["boxes"][:nv], torch.as_tensor(want["boxes"])[pos], rtol=1e-5, atol=2e-4)
    return nv


# ---- kernel level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("method", CRITERIA)
def test_rank_topk_decode_vs_reference_golden(gold, head, method):
    """N = 2, the five levels of the 96 x 128 fixture (12x16 ... 1x1: the last level is a single location and keeps every candidate),
    C = 80: candidates after utv2_topk_rows_i64 and every decode output"""
    from ubteacher.modeling.fcos import METHODS
    hip = H()
    N, thr, topk = int(gold["N"]), float(gold["thr"]), int(gold["topk"])
    counts = []
    for l, s in enumerate(STRIDES):
        keys, top, outs = run_level(head, *golden_level_inputs(gold, head, l), s, l, thr, topk, METHODS[method], hip.FCOS_THRESH_WITH_CTR)
        for i in range(N):
            p = "%s_%s_L%d_I%d_" % (head, method, l, i)
            want = {k: gold[p + k] for k in ("flat", "scores", "conf", "ctr", "boxes", "std")}
            want["rank"] = want["conf"]                                    # :1179: cls_confid is the ranking score
            counts.append((check_row(top, outs, i, want, l), int((keys[i] >= 0).sum())))
    assert any(n == topk and cand > topk for n, cand in counts)             # the cut bites ...
    assert any(0 < n < topk and cand == n for n, cand in counts)            # ... and a row keeps every candidate


@pytest.mark.parametrize("head", HEADS)
def test_flag_off_is_the_call_of_today_bit_for_bit(gold, head):
    """hip.fcos_rank_keys / fcos_decode(_cont) call the entry points that take the flag (utv2_fcos_*_f).  With flags 0 their keys and
    every decode output equal, with torch.equal, those of utv2_fcos_rank_keys / utv2_fcos_decode / utv2_fcos_decode_cont called
    directly as before the flag existed, and the keys are those of the flag-off restatement (candidate mask exact, ranking score 1e-6)
    - not the flag's."""
    from ubteacher.modeling.fcos import METHODS
    hip = H()
    N, thr, topk = int(gold["N"]), float(gold["thr"]), int(gold["topk"])
    l, s = 1, STRIDES[1]
    logits, reg, std, ctr = golden_level_inputs(gold, head, l)
    h, w = logits.shape[2:]
    lg = logits.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    bx = box_rows(head, reg, std, ctr).to(DEV)
    reg_max = 16 if head == "d" else hip.REG_CONT
    for name, m in METHODS.items():
        keys, top, outs = run_level(head, logits, reg, std, ctr, s, l, thr, topk, m, 0)
        raw = torch.full((N, h * w * C), -7, dtype=torch.int64, device=DEV)
        hip.call("utv2_fcos_rank_keys", hip._p_any(lg), hip._p_any(bx), BS[head], reg_max, N, h * w, C, float(thr), int(m),
                 hip.c_p(raw.data_ptr()), h * w * C, hip._stream())
        assert torch.equal(keys, raw.cpu()), name
        ro = fresh_outs(N, top.shape[1])
        tail = [hip._p(ro[k]) for k in ("boxes", "scores", "classes", "locations", "centerness", "cls_confid", "reg_pred_std", "fpn_levels", "valid")]
        td = top.to(DEV)
        if head == "d":
            hip.call("utv2_fcos_decode", hip._p(td), top.shape[1], hip._p(lg), hip._p(bx), BS[head], reg_max, N, h * w, w, C, s, l, int(m),
                     top.shape[1], 0, *tail, hip._stream())
        else:
            hip.call("utv2_fcos_decode_cont", hip._p(td), top.shape[1], hip._p(lg), hip._p(bx), BS[head], N, h * w, w, C, s, l, int(m),
                     top.shape[1], 0, *tail, hip._stream())
        torch.cuda.synchronize()
        for k, v in ro.items():
            assert torch.equal(outs[k], v.cpu()), (name, k)
        if head == "d" and m == 0:
            # the old discrete entry point never checked `method`: 4 (the kernel's own flag bit), 5, 7 ... still write what 0 writes
            for stray in (4, 5, 7, -1):
                so = fresh_outs(N, top.shape[1])
                stail = [hip._p(so[k]) for k in ("boxes", "scores", "classes", "locations", "centerness", "cls_confid", "reg_pred_std", "fpn_levels", "valid")]
                hip.call("utv2_fcos_decode", hip._p(td), top.shape[1], hip._p(lg), hip._p(bx), BS[head], reg_max, N, h * w, w, C, s, l, stray,
                         top.shape[1], 0, *stail, hip._stream())
                torch.cuda.synchronize()
                for k, v in so.items():
                    assert torch.equal(outs[k], v.cpu()), (stray, k)
        off = restate_level(logits, reg, std, ctr, s, head == "d", thr, 10 ** 9, name, False)     # every candidate, no cut
        on = restate_level(logits, reg, std, ctr, s, head == "d", thr, 10 ** 9, name, True)
        for i in range(N):
            cand = (keys[i] >= 0).nonzero().squeeze(1)
            assert torch.equal(cand, torch.sort(off[i]["flat"])[0]), name
            assert not torch.equal(cand, torch.sort(on[i]["flat"])[0])
            got = (keys[i][cand] >> 32).to(torch.int32).view(torch.float32)
            assert float((got - off[i]["rank"][torch.argsort(off[i]["flat"])]).abs().max()) <= 1e-6, name


def edge_inputs(head):
    """3 images, one 2 x 2 level (stride 64): image 0 has confident classes and a centerness of ~6e-6 (no candidate under the key, many
    without it), image 1 more candidates than the top-k, image 2 a few (every one survives)"""
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(3, C, 2, 2, generator=g) * 1.5
    logits[2] -= 4.2
    ctr = torch.randn(3, 1, 2, 2, generator=g)
    ctr[0] = -12.0
    std = torch.randn(3, 4, 2, 2, generator=g)
    reg = torch.randn(3, 68, 2, 2, generator=g) * 2 if head == "d" else torch.randn(3, 4, 2, 2, generator=g) * 2 + 1
    return logits, reg, std, ctr


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("method", CRITERIA)
def test_edge_rows_vs_restatement(head, method):
    from ubteacher.modeling.fcos import METHODS
    hip = H()
    thr, topk, s = 0.05, 50, 64
    inp = edge_inputs(head)
    want = restate_level(*inp, s, head == "d", thr, topk, method, True)
    every = restate_level(*inp, s, head == "d", thr, 10 ** 9, method, True)
    plain = restate_level(*inp, s, head == "d", thr, 10 ** 9, method, False)
    # the test's own ground: the three kinds of row, and no decision within rounding reach (as the golden's generator asserts)
    assert len(want[0]["flat"]) == 0 and len(plain[0]["flat"]) > 100
    assert len(every[1]["flat"]) > topk and 0 < len(every[2]["flat"]) < topk
    p = inp[0].permute(0, 2, 3, 1).reshape(3, -1, C).sigmoid() * inp[3].permute(0, 2, 3, 1).reshape(3, -1).sigmoid()[:, :, None]
    assert float(((p - thr).abs() / thr).min()) > 1e-5
    v = torch.sort(every[1]["rank"], descending=True)[0]
    assert float(v[topk - 1] - v[topk]) > 1e-6
    keys, top, outs = run_level(head, *inp, s, 3, thr, topk, METHODS[method], hip.FCOS_THRESH_WITH_CTR)
    assert bool((keys[0] == -1).all()) and bool((top[0] == -1).all())
    off_keys = hip.fcos_rank_keys(inp[0].permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV), box_rows(head, *inp[1:]).to(DEV),
                                  16 if head == "d" else hip.REG_CONT, 3, 4, thr, METHODS[method], flags=0).cpu()
    assert int((off_keys[0] >= 0).sum()) == len(plain[0]["flat"])
    got = [check_row(top, outs, i, want[i], 3) for i in range(3)]
    assert got[0] == 0 and got[1] == topk and got[2] == len(every[2]["flat"])
    assert not bool(outs["valid"][0].any()) and bool((outs["boxes"][0] == 0).all()) and bool((outs["cls_confid"][0] == 0).all())


@pytest.mark.parametrize("method,flags", [(0, 2), (1, 3), (0, -1), (4, 1), (5, 0)])
def test_unknown_flag_is_refused(method, flags):
    """through hip.py, on live device buffers: UTV2_EARG, nothing launched, nothing written"""
    from tests.test_fcos_thresh_ctr import flag_argument_rows
    hip = H()
    one = torch.zeros(4096, device=DEV)
    for name, args in flag_argument_rows(one.data_ptr(), method, flags):
        assert getattr(hip.load(), name)(*args) == -1000, name
    lg, bx = torch.zeros((4, C), device=DEV), torch.zeros((4, 80), device=DEV)
    with pytest.raises(RuntimeError, match=EARG):
        hip.fcos_rank_keys(lg, bx, 16, 1, 4, 0.05, method, flags=flags)
    outs = fresh_outs(1, 4)
    top = torch.full((1, 4), -1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match=EARG):
        hip.fcos_decode(top, lg, bx, 16, 1, 4, 2, 8, 0, method, 0, outs, flags=flags)
    with pytest.raises(RuntimeError, match=EARG):
        hip.fcos_decode_cont(top, lg, bx, 1, 4, 2, 8, 0, method, 0, outs, flags=flags)
    torch.cuda.synchronize()
    assert bool((one == 0).all()) and bool((outs["scores"] == 9.0).all())


# ---- FCOSOutputs.predict_proposals ------------------------------------------------------------------------------------------------
def key_cfg(gold, head, on=True):
    from tests.test_fcos_cont import cont_outputs_cfg
    from tests.test_fcos_kernels_gpu import fcos_cfg
    cfg = fcos_cfg() if head == "d" else cont_outputs_cfg()
    f = cfg.MODEL.FCOS
    f.THRESH_WITH_CTR = on
    f.INFERENCE_TH_TRAIN = f.INFERENCE_TH_TEST = float(gold["thr"])
    f.PRE_NMS_TOPK_TRAIN = f.PRE_NMS_TOPK_TEST = int(gold["topk"])
    f.POST_NMS_TOPK_TRAIN = f.POST_NMS_TOPK_TEST = int(gold["post_topk"])
    f.NMS_TH = float(gold["nms_th"])
    return cfg


def golden_head_out(gold, head):
    from ubteacher.ops import LevelMeta
    N = int(gold["N"])
    level_hw = [tuple(gold["logits%d" % l].shape[2:]) for l in range(5)]
    logits_all = torch.cat([T(gold["logits%d" % l]).permute(0, 2, 3, 1).reshape(-1, C) for l in range(5)]).contiguous().to(DEV)
    box_all = torch.cat([box_rows(head, *golden_level_inputs(gold, head, l)[1:]) for l in range(5)]).contiguous().to(DEV)
    return {"logits": logits_all, "box": box_all, "meta": LevelMeta(N, level_hw)}, level_hw


def index_of(inst, W):
    """(level, location * C + class) of every detection of an Instances, from its level and location"""
    lev = inst.fpn_levels.long().cpu().numpy()
    s = np.array(STRIDES)[lev]
    loc = inst.locations.cpu().numpy()
    hw = ((loc[:, 1] - s // 2) / s).round().astype(np.int64) * -(-W // s) + ((loc[:, 0] - s // 2) / s).round().astype(np.int64)
    cls = (inst.pred_classes if inst.has("pred_classes") else inst.gt_classes).long().cpu().numpy()
    return lev, hw * C + cls


def check_detections(gold, head, method, det):
    W = int(gold["W"])
    for i, r in enumerate(det.to_instances()):
        p = "%s_%s_det%d_" % (head, method, i)
        assert len(r) == len(gold[p + "flat"]) > 0
        lev, flat = index_of(r, W)
        assert np.array_equal(lev, gold[p + "level"]) and np.array_equal(flat, gold[p + "flat"])     # same detections, same order
        assert float(np.abs(r.scores.cpu().numpy().astype(np.float64) - gold[p + "scores"]).max()) <= 1e-6
        assert float(np.abs(r.cls_confid.cpu().numpy().astype(np.float64) - gold[p + "conf"]).max()) <= 1e-6
        close(r.centerness, gold[p + "ctr"], rtol=2e-5)
        close(r.reg_pred_std, gold[p + "std"])
        close(r.pred_boxes.tensor, gold[p + "boxes"], rtol=1e-5, atol=2e-4)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("mode", ["test", "train"])
def test_predict_proposals_vs_reference_golden(gold, head, mode):
    """the four criteria one by one, eval mode (*_TEST keys) and training mode (*_TRAIN keys: the PseudoGenerator's own FCOSOutputs and
    the YIELD_PROPOSAL proposals read those): post-NMS detections equal the golden's in index and order"""
    from ubteacher.modeling.fcos import FCOSOutputs
    outm = FCOSOutputs(key_cfg(gold, head))
    outm.training = mode == "train"
    head_out, level_hw = golden_head_out(gold, head)
    sizes = [(int(gold["H"]), int(gold["W"]))] * int(gold["N"])
    for method in CRITERIA:
        check_detections(gold, head, method, outm.predict_proposals(head_out, level_hw, sizes, method))


@pytest.mark.parametrize("head", HEADS)
def test_fused_criteria_launch_vs_reference_golden(gold, head, monkeypatch):
    """the (criterion, image) form the trainer uses for the teacher's two pseudo-label criteria (UTV2_FUSE_TEACHER_NMS): all four in one
    call; every kernel call carries the flag next to its criterion, and none does when the key is off"""
    from ubteacher.modeling import fcos as M
    seen = []
    for name in ("fcos_rank_keys", "fcos_decode", "fcos_decode_cont"):
        def spy(*a, _f=getattr(M.hip, name), _i={"fcos_rank_keys": 6, "fcos_decode": 9, "fcos_decode_cont": 8}[name], **k):
            seen.append((a[_i], k.get("flags", 0)))
            return _f(*a, **k)
        monkeypatch.setattr(M.hip, name, spy)
    head_out, level_hw = golden_head_out(gold, head)
    sizes = [(int(gold["H"]), int(gold["W"]))] * int(gold["N"])
    outm = M.FCOSOutputs(key_cfg(gold, head))
    outm.training = False
    dets = outm.predict_proposals(head_out, level_hw, sizes, CRITERIA)
    for method, det in zip(CRITERIA, dets):
        check_detections(gold, head, method, det)
    assert sorted(set(seen)) == [(m, M.hip.FCOS_THRESH_WITH_CTR) for m in range(4)] and len(seen) == 2 * 4 * 5
    del seen[:]
    off = M.FCOSOutputs(key_cfg(gold, head, on=False))
    off.training = False
    off.predict_proposals(head_out, level_hw, sizes, CRITERIA)
    assert sorted(set(seen)) == [(m, 0) for m in range(4)] and len(seen) == 2 * 4 * 5


# ---- model level ------------------------------------------------------------------------------------------------------------------
def step_overrides(gold):
    over = [str(x) for x in gold["step_overrides"]]
    return [v if i % 2 == 0 else (v == "True" if v in ("True", "False") else int(v)) for i, v in enumerate(over)]


def golden_trainer(gold):
    """the trainer of tests/test_fcos_step_gpu.py::test_fcos_step_vs_reference_trainer_golden (batch and initial state of step_fcos.npz)
    with the golden's overrides: the key on, PRE_NMS_TOPK_TRAIN / _TEST 50"""
    from tests.utv2_testutil import FixedLoader, golden_batches, golden_init_state, load_step_golden, small_fcos_cfg, tune_state_for_pseudo_labels
    from ubteacher.engine import UBTeacherTrainer
    d = load_step_golden("fcos")
    _, sd0 = golden_init_state("fcos", d)
    prod, orac = golden_batches(d, DEV)
    cfg = small_fcos_cfg()
    cfg.merge_from_list(step_overrides(gold))
    assert cfg.MODEL.FCOS.THRESH_WITH_CTR is True
    tr = UBTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    sd_s = tune_state_for_pseudo_labels(sd0, [x["image"] for x in orac[3]])
    sd_t = dict(sd_s)
    sd_t["proposal_generator.fcos_head.bbox_pred_std.bias"] = torch.full((4,), -3.0)
    tr.model.load_state_dict(sd_s)
    tr.model_teacher.load_state_dict(sd_t)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = float(d["lr"])
    return tr, cfg, prod, d


def pseudo_sets(tr, W):
    """the step's two pseudo-label sets as per-image (level, flat index) arrays sorted by index, with boxes and scores in that order"""
    out = []
    for pb in tr._last_pseudo:
        per = []
        for r in pb.to_instances(as_gt=True):
            lev, flat = index_of(r, W)
            o = np.lexsort((flat, lev))
            per.append((lev[o], flat[o], r.gt_boxes.tensor.cpu().numpy()[o], r.scores.cpu().numpy()[o]))
        out.append(per)
    return out


def test_step_vs_reference_trainer_golden(gold):
    tr, cfg, prod, d = golden_trainer(gold)
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    assert tr.fuse_teacher_nms
    for k in gold:
        if k.startswith("step_rec_") and k != "step_rec_data_time":
            v = float(gold[k])
            print(k, rec[k[9:]], v)
            assert abs(rec[k[9:]] - v) <= 1e-3 * max(abs(v), 1e-6), (k, rec[k[9:]], v)
    total = 0
    for name, per in zip(("pcls", "preg"), pseudo_sets(tr, int(d["W"]))):
        for i, (lev, flat, boxes, scores) in enumerate(per):
            p = "step_%s%d_" % (name, i)
            o = np.lexsort((gold[p + "flat"], gold[p + "level"]))
            assert np.array_equal(lev, gold[p + "level"][o]) and np.array_equal(flat, gold[p + "flat"][o]), p
            np.testing.assert_allclose(boxes, gold[p + "boxes"][o], rtol=0, atol=2e-2)
            np.testing.assert_allclose(scores, gold[p + "scores"][o], rtol=1e-3)
            total += len(flat)
    assert total > 0


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import torch
from tests.test_fcos_thresh_ctr_gpu import golden_trainer, pseudo_sets
from tests.test_fcos_thresh_ctr import load_gold
tr, cfg, prod, d = golden_trainer(load_gold())
assert not tr.fuse_teacher_nms
tr.run_step_full_semisup()
torch.cuda.synchronize()
torch.save(pseudo_sets(tr, int(d["W"])), sys.argv[1])
"""


def test_unfused_teacher_nms_gives_the_same_pseudo_sets(gold, tmp_path):
    """UTV2_FUSE_TEACHER_NMS=0 (read when the trainer is built: a fresh child process): the second criterion goes through
    PseudoGenerator.nms_from_dense and its own FCOSOutputs - identical pseudo sets, boxes and scores to the bit"""
    path = str(tmp_path / "unfused.pt")
    env = dict(os.environ, UTV2_FUSE_TEACHER_NMS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "unbiased-teacher-v2_amd")), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = torch.load(path, weights_only=False)
    tr, cfg, prod, d = golden_trainer(gold)
    tr.run_step_full_semisup()
    torch.cuda.synchronize()
    mine = pseudo_sets(tr, int(d["W"]))
    assert sum(len(x[0]) for per in mine for x in per) > 0
    for a, b in zip(mine, child):
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)


def test_eval_detections_vs_reference_golden(gold):
    """test-mode inference as Trainer.test() runs it (inference_on_dataset -> eval-mode detector, NMS_CRITERIA_TEST, *_TEST keys ->
    detector_postprocess) on the two weak unlabeled 96 x 128 images: detections equal the golden's in index and order"""
    from ubteacher.evaluation import inference_on_dataset
    tr, cfg, prod, d = golden_trainer(gold)
    Hh, W = int(d["H"]), int(d["W"])
    assert str(gold["eval_criterion"]) == cfg.MODEL.FCOS.NMS_CRITERIA_TEST
    batch = [{"image": x["image"], "height": Hh, "width": W, "image_id": i} for i, x in enumerate(prod[3])]

    class Capture:
        def reset(self):
            self.out = []

        def process(self, inputs, outputs):
            self.out.extend(outputs)

        def evaluate(self):
            return {}
    ev = Capture()
    inference_on_dataset(tr.model_teacher, [batch], ev, cfg)
    assert len(ev.out) == 2
    for i, r in enumerate(ev.out):
        x = r["instances"]
        assert len(x) == len(gold["eval%d_flat" % i]) > 0
        lev, flat = index_of(x, W)
        assert np.array_equal(lev, gold["eval%d_level" % i]) and np.array_equal(flat, gold["eval%d_flat" % i])
        np.testing.assert_allclose(x.scores.cpu().numpy(), gold["eval%d_scores" % i], rtol=1e-3)
        np.testing.assert_allclose(x.pred_boxes.tensor.cpu().numpy(), gold["eval%d_boxes" % i], rtol=0, atol=1e-3 * max(Hh, W))


def test_yield_proposal_train_time_proposals_carry_the_key(gold):
    """MODEL.FCOS.YIELD_PROPOSAL: the student's train-time proposals are predict_proposals of the same head output under the key -
    cls_confid is the centerness product (<= both factors) - and the same forward of the same weights with the key off gives other
    proposals, whose cls_confid is the plain class probability"""
    tr, cfg, prod, d = golden_trainer(gold)
    tr.model.train()
    _, raw, results = tr.model(prod[1], output_raw=True, branch="labeled")
    props = results["proposals"]
    m = props["valid"].bool()
    assert int(m.sum()) > 0
    conf, ctr, sc = props["cls_confid"][m].detach(), props["centerness"][m].detach(), props["scores"][m].detach()
    assert bool((conf > cfg.MODEL.FCOS.INFERENCE_TH_TRAIN).all())
    assert float((sc - conf.sqrt()).abs().max()) <= 1e-6                    # cls_n_ctr: sqrt of the product
    lg = torch.cat([t.detach().permute(0, 2, 3, 1).reshape(-1, C) for t in raw["logits_pred"]])
    assert bool((conf <= ctr * (1 + 1e-6)).all()) and float(conf.max()) <= float(lg.sigmoid().max())
    fo = tr.model.proposal_generator.fcos_outputs
    fo.thresh_with_ctr = False
    try:
        _, _, results_off = tr.model(prod[1], output_raw=True, branch="labeled")
        off = results_off["proposals"]
    finally:
        fo.thresh_with_ctr = True
    mo = off["valid"].bool()
    assert int(mo.sum()) > 0
    conf_o, ctr_o, sc_o = off["cls_confid"][mo].detach(), off["centerness"][mo].detach(), off["scores"][mo].detach()
    assert float((sc_o - (conf_o * ctr_o).sqrt()).abs().max()) <= 1e-6      # cls_n_ctr without the key: sqrt(p * c), cls_confid = p
    assert not torch.equal(off["cls_confid"], props["cls_confid"])


def test_step_as_hipgraph_replays_the_eager_step(monkeypatch):
    """the pattern of tests/test_fcos_step_gpu.py::test_step_as_hipgraph_replays_the_eager_step with the key on: five eager steps against
    two eager + capture + replays - the same losses at every step (1e-4, its bound), the same student / teacher afterwards"""
    monkeypatch.setenv("UTV2_PRECISION", "bf16")
    import bench
    from ubteacher import ops
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "SOLVER.AMP.ENABLED", True, "MODEL.DEVICE", "cuda", "MODEL.FCOS.THRESH_WITH_CTR", True])
    outs = []
    try:
        for graph in (False, True):
            torch.manual_seed(0)
            tr = UBTeacherTrainer(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=96, width=128))
            assert tr.model_teacher.proposal_generator.fcos_outputs.thresh_with_ctr
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
                assert all(st["graph"] is not None for st in tr._step_graphs.values()) and tr._step_graphs
            assert ops.STEP_GRAPH[0] is False
            outs.append((recs, tr.model.flat_state().clone(), tr.model_teacher.flat_state().clone()))
    finally:
        ops.STEP_GRAPH[0] = False
    (ra, sa, ta), (rb, sb, tb) = outs
    assert any(v > 0 for r in ra for k, v in r.items() if k.endswith("_pseudo") and k.startswith("loss")), "no pseudo label reached a loss"
    for a, b in zip(ra, rb):
        for k, v in a.items():
            if k.startswith("loss"):
                assert v == v and abs(b[k] - v) <= 1e-4 * max(abs(v), 1e-3), (k, v, b[k])
    assert torch.isfinite(sa).all() and torch.isfinite(sb).all() and torch.isfinite(tb).all()
    assert float((sa - sb).abs().max()) <= 1e-4 * float(sa.abs().max()) and float((ta - tb).abs().max()) <= 1e-4 * float(ta.abs().max())
