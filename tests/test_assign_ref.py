"""CPU self-test of tests/assign_ref.py: on seeded random INTEGER inputs and on every branch case of test_assign_exact_gpu.py the plain
reference equals the project's oracle (bit-equal values, equal indices); every branch case hits the decision point it claims, with
an exact count; every one-token flip of a comparison changes the expected output of some case; the precondition is enforced."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import utv2_oracle as O
from tests import assign_ref as R

T = torch.from_numpy


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_threshold_table_of_the_issue():
    """the four facts every decision at a threshold rests on"""
    f = np.float32
    assert f(7) / f(10) >= f(0.7) and not f(3) / f(10) < f(0.3) and not f(6) / f(10) > f(0.6) and f(8) / f(16) >= f(0.5)
    assert R.iou((0, 0, 10, 10), (0, 0, 10, 7)) >= f(0.7) and not R.iou((0, 0, 10, 10), (0, 0, 10, 3)) < f(0.3)
    t = torch.tensor([0.7, 0.3, 0.6]) - 0
    got = T(np.array([f(7) / f(10), f(3) / f(10), f(6) / f(10)]))
    assert bool(got[0] >= 0.7) and not bool(got[1] < 0.3) and not bool(got[2] > 0.6) and torch.equal(got, t)


def test_precondition_rejects_what_is_not_exact():
    for bad in ([0.5, 0, 10, 10], [0, 0, 1025, 10], [0, 0, 10, float("nan")], [10, 0, 0, 10], [0, -1025, 1, 1]):
        with pytest.raises(ValueError):
            R.int_boxes(np.array([bad]))
        with pytest.raises(ValueError):
            R.match(np.array([bad]), np.array([[0, 0, 1, 1]]), [1])
    with pytest.raises(ValueError):    # the class offset leaves the exact range
        R.nms(np.array([[0, 0, 1000, 1000]] * 2), [1, 0.5], [5000, 0], [1, 1], 0.5, True)
    with pytest.raises(ValueError):
        R.fcos_targets([(2, 2)], [8], [[-1, 64]], np.zeros((1, 1, 4)), np.zeros((1, 1), int), np.ones((1, 1)), None, 80, 0, center_radius=0.3)
    assert R.int_boxes(np.array([[-1024, -1024, 1024, 1024]])) == [(-1024, -1024, 1024, 1024)]


# ---------------------------------------------------------------------------------------------------------------------------------
# matcher + RPN sampler against O.pairwise_iou / O.matcher / O.subsample_by_keys
def _oracle_rpn(boxes, gb, gv, keys, lo, hi, batch, frac):
    """(vals, slot argument, labels, pos, neg) of one image by the oracle on the COMPACTED valid gts"""
    slots = np.nonzero(gv)[0]
    P = len(boxes)
    if len(slots) == 0:
        iou = torch.zeros((0, P))
    else:
        iou = O.pairwise_iou(T(gb[slots]), T(boxes))
    idx, lab = O.matcher(iou, [lo, hi], [0, -1, 1], True)
    vals = iou.max(dim=0)[0].numpy() if len(slots) else np.full(P, -1, np.float32)
    arg = slots[idx.numpy()] if len(slots) else np.zeros(P, np.int64)
    pos, neg = O.subsample_by_keys(lab, T(keys), batch, frac, 0)
    return vals, arg, lab.numpy(), pos.numpy(), neg.numpy(), iou


def _check_rpn_image(boxes, gb, gv, keys, lo=0.3, hi=0.7, batch=16, frac=0.25):
    mx, arg, gmax = R.match(boxes, gb, gv)
    lq = R.lowq(boxes, gb, gv, gmax)
    vals, oarg, olab, opos, oneg, iou = _oracle_rpn(boxes, gb, gv, keys, lo, hi, batch, frac)
    assert np.array_equal(_bits(mx), _bits(vals)) and np.array_equal(arg, oarg)
    if iou.numel():
        assert np.array_equal(_bits(gmax[np.nonzero(gv)[0]]), _bits(iou.max(dim=1)[0].numpy()))
    npos_max = int(batch * frac)
    lab, pi, pv, ni, nv = R.rpn_labels_and_sample(mx, lq, bool(gv.any()), keys, lo, hi, npos_max, batch)
    assert np.array_equal(lab, olab)
    assert np.array_equal(pi[:pv.sum()], opos) and np.array_equal(ni[:nv.sum()], oneg)
    assert pv[:len(opos)].all() and nv[:len(oneg)].all()


def test_matcher_and_rpn_sampler_equal_the_oracle_on_random_integer_boxes():
    rng = np.random.default_rng(1)
    for seed in range(200):
        P, G = int(rng.integers(1, 40)), int(rng.integers(1, 7))
        boxes, gb = R.random_int_boxes(rng, P), R.random_int_boxes(rng, G)
        gv = (rng.random(G) < 0.7).astype(np.uint8)
        _check_rpn_image(boxes, gb, gv, R.dyadic_keys(rng, P), batch=int(rng.integers(1, 24)))


MATCH_THRESHOLD_CENSUS = [
    dict(iou_eq_7_10=1, iou_eq_3_10=1, iou_eq_1_2=1, iou_one=1, argmax_tie=0, gt_untouched=0, zero_area_gt=0, zero_area_box=1, n_valid=4),
    dict(argmax_tie=1, n_valid=2, gt_untouched=0),
    dict(argmax_tie=1, n_valid=2, gt_untouched=0),
    dict(gt_untouched=1, n_valid=2, argmax_tie=0),
    dict(zero_area_gt=1, gt_untouched=1, n_valid=2),
    dict(n_valid=0),
    dict(n_valid=1, max_only_at_last=0, gt_untouched=0),
]


def test_matcher_threshold_case_hits_its_branches_and_equals_the_oracle():
    inp, census = R.matcher_threshold_case()
    assert len(census) == len(MATCH_THRESHOLD_CENSUS) == 7
    for n, want in enumerate(MATCH_THRESHOLD_CENSUS):
        for k, v in want.items():
            assert census[n][k] == v, (n, k, census[n][k])
    rng = np.random.default_rng(2)
    for n in range(7):
        _check_rpn_image(inp["boxes"], inp["gt_boxes"][n], inp["gt_valid"][n], R.dyadic_keys(rng, 40))
    mx, arg, gmax, lq = R.match_all(inp["boxes"], inp["gt_boxes"], inp["gt_valid"])
    # the anchors that sit on a threshold carry it through max, argument and label
    assert Fraction(float(mx[0, 0])).limit_denominator(100) == Fraction(7, 10) and list(arg[0, :4]) == [0, 1, 2, 3]
    lab = R.rpn_labels_and_sample(mx[0], np.zeros(40), True, np.zeros(40), 0.3, 0.7, 4, 8)[0]
    assert list(lab[:5]) == [1, -1, -1, 1, 0]        # 7/10 -> positive, 3/10 -> not negative, 1/2 ignored, 1 positive, 0 negative
    assert arg[1, 5] == 0 and arg[2, 5] == 1          # first slot wins, also behind the hole
    assert lq[3].all() and lq[4].all() and not lq[5].any() and mx[5].max() == -1
    assert lq[6].sum() == 2 and lq[0].sum() == 4


@pytest.mark.parametrize("G", [1, 64, 65, 256])
@pytest.mark.parametrize("P", [1, 256, 257])
def test_matcher_boundary_cases_hit_their_branches_and_equal_the_oracle(G, P):
    rng = np.random.default_rng(3)
    for per_image in (False, True):
        inp, census = R.matcher_boundary_case(G, P, per_image)
        nv = {1: 1, 64: 1, 65: 2, 256: 5}[G]
        assert census[0]["n_valid"] == census[1]["n_valid"] == nv
        assert census[0]["max_only_at_last"] == nv and census[0]["gt_untouched"] == 0
        assert list(np.nonzero(inp["gt_valid"][0])[0]) == ([0] if G == 1 else [s for s in R.WAVE_SLOTS if s < G])
        for n in range(2):
            b = inp["boxes"][n] if per_image else inp["boxes"]
            _check_rpn_image(b, inp["gt_boxes"][n], inp["gt_valid"][n], R.dyadic_keys(rng, P), batch=8)


# ---------------------------------------------------------------------------------------------------------------------------------
# ROI sampler against O.roi_label_and_sample
def _check_roi_image(rng, P, G, batch, frac, num_classes=5):
    prop, gb = R.random_int_boxes(rng, P), R.random_int_boxes(rng, G)
    gc = rng.integers(0, num_classes, size=G)
    gs = (rng.integers(1, 9, size=G) / 8).astype(np.float32)
    gstd = (rng.integers(1, 9, size=(G, 4)) / 8).astype(np.float32)
    pb = np.concatenate([prop, gb])
    keys = R.dyadic_keys(rng, len(pb))
    gt = dict(boxes=T(gb), classes=T(gc), scores=T(gs), pred_boxes_std=T(gstd))
    want = O.roi_label_and_sample(T(prop), gt, T(keys), True, num_classes, batch, frac)
    gv = np.ones(G, np.uint8)
    mx, arg, _ = R.match(pb, gb, gv) if G else (np.full(len(pb), -1, np.float32), np.zeros(len(pb), np.int32), None)
    got = R.roi_sample(pb, np.ones(len(pb)), mx, arg, keys, gb, gc, gv, gs, gstd, 0.5, num_classes, batch, int(batch * frac))
    k = len(want["gt_classes"])
    assert int(got["valid"].sum()) == k and got["valid"][:k].all()
    assert np.array_equal(got["gt_classes"][:k], want["gt_classes"].numpy()) and (got["gt_classes"][k:] == -1).all()
    for name in ("proposal_boxes", "gt_boxes", "gt_confid", "gt_loc_std"):
        assert np.array_equal(_bits(got[name][:k]), _bits(want[name].numpy())), name
        assert not got[name][k:].any()
    return got


def test_roi_sampler_equals_the_oracle_on_random_integer_boxes():
    rng = np.random.default_rng(4)
    nfg = []
    for seed in range(200):
        got = _check_roi_image(rng, int(rng.integers(1, 30)), int(rng.integers(0, 5)), int(rng.integers(1, 20)), 0.25)
        nfg.append(got["nfg"])
    assert max(nfg) > 0 and min(nfg) == 0


RPN_SAMPLER_CENSUS = {
    True: dict(over=6, room0=3, short=9, equal_keys=250, empty_images=3, lowq_over_ignored=4, lowq_over_negative=80),
    False: dict(over=0, room0=0, short=7, equal_keys=305, empty_images=3, lowq_over_ignored=0, lowq_over_negative=0),
}


@pytest.mark.parametrize("with_lowq", [True, False])
def test_rpn_sampler_case_hits_its_branches_and_equals_the_oracle(with_lowq):
    inp, want, census = R.rpn_sampler_case(with_lowq)
    assert census == RPN_SAMPLER_CENSUS[with_lowq] and len(want) == 21
    for (npos_max, batch, n), (lab, pi, pv, ni, nv) in want.items():
        olab = torch.full((40,), -1, dtype=torch.int8)
        v = T(inp["mx"][n])
        olab[v < 0.3] = 0
        olab[v >= 0.7] = 1
        olab[T(inp["lowq"][n]).bool()] = 1
        if not inp["gt_valid"][n].any():
            olab[:] = 0
        assert np.array_equal(lab, olab.numpy())
        pos, neg = O.subsample_by_keys(olab, T(inp["keys"][n]), batch, (npos_max + 0.5) / batch, 0)
        assert np.array_equal(pi[:pv.sum()], pos.numpy()) and np.array_equal(ni[:nv.sum()], neg.numpy())


ROI_CENSUS = {
    1: dict(mx_eq_thr=1, nfg=[1, 0, 0], equal_keys=0, invalid_between=0, has_gt=[1, 0, 1]),
    511: dict(mx_eq_thr=4, nfg=[5, 0, 6], equal_keys=1339, invalid_between=170, has_gt=[1, 0, 1]),
    512: dict(mx_eq_thr=2, nfg=[8, 0, 1], equal_keys=1341, invalid_between=170, has_gt=[1, 0, 1]),
    513: dict(mx_eq_thr=1, nfg=[7, 0, 3], equal_keys=1344, invalid_between=171, has_gt=[1, 0, 1]),
}


def roi_caps(census):
    """(B, the nfg_max values): the foreground count of image 0 is exactly nfg_max, and nfg_max + 1"""
    nfg0 = census["nfg"][0]
    return nfg0 + 8, sorted({nfg0, max(nfg0 - 1, 0), 4})


@pytest.mark.parametrize("P", [1, 511, 512, 513])
def test_roi_case_hits_its_branches_and_equals_the_oracle(P):
    """the oracle's matcher + subsample_by_keys on the valid proposals and the valid gts (roi_label_and_sample itself appends the gt
    boxes to the proposals; the kernel's caller has done that before)"""
    c, census = R.roi_case(P)
    assert census == ROI_CENSUS[P]
    assert c["mx"][0, 0] == np.float32(0.5) and c["arg"][0, 0] == 0
    B, caps = roi_caps(census)
    for nfg_max in caps:
        for n in range(3):
            got = R.roi_sample_image(c, n, B, nfg_max)
            vi = np.nonzero(c["valid"][n])[0]
            slots = np.nonzero(c["gv"][n])[0]
            if len(slots):
                iou = O.pairwise_iou(T(c["gb"][n][slots]), T(c["boxes"][n][vi]))
                midx, lab = O.matcher(iou, [0.5], [0, 1], False)
                cls = T(c["gc"][n][slots]).long()[midx].clone()
                cls[lab == 0] = R.ROI_CLASSES
            else:
                midx = torch.zeros(len(vi), dtype=torch.int64)
                cls = torch.full((len(vi),), R.ROI_CLASSES, dtype=torch.int64)
            fgi, bgi = O.subsample_by_keys(cls, T(c["keys"][n][vi]), B, (nfg_max + 0.5) / B, R.ROI_CLASSES)
            sel = torch.cat((fgi, bgi)).numpy()
            k = len(sel)
            assert int(got["valid"].sum()) == k and got["valid"][:k].all() and got["nfg"] == len(fgi)
            assert np.array_equal(got["sampled_idx"][:k], vi[sel]) and np.array_equal(got["gt_classes"][:k], cls.numpy()[sel])
            assert np.array_equal(_bits(got["proposal_boxes"][:k]), _bits(c["boxes"][n][vi[sel]]))
            if len(slots):
                g = slots[midx.numpy()[sel]]
                assert np.array_equal(_bits(got["gt_boxes"][:k]), _bits(c["gb"][n][g]))
                assert np.array_equal(_bits(got["gt_confid"][:k]), _bits(c["gs"][n][g]))
                assert np.array_equal(_bits(got["gt_loc_std"][:k]), _bits(c["gstd"][n][g]))
            else:
                assert not got["gt_boxes"].any() and not got["gt_confid"].any() and not got["gt_loc_std"].any()
            assert (got["gt_classes"][k:] == -1).all() and not got["proposal_boxes"][k:].any() and not got["gt_boxes"][k:].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# FCOS targets against O.fcos_targets
def _soi(edges):
    """sizes of interest from their inner edges, as FCOSOutputs builds them: [-1, e0], [e0, e1], ..., [e_last, INF]"""
    e = [-1.0] + [float(v) for v in edges] + [R.INF]
    return [[a, b] for a, b in zip(e[:-1], e[1:])]


def _oracle_fcos(names_or_arrays, drop_empty, radius, level_hw=R.FCOS_HW, strides=R.FCOS_STRIDES, edges=R.FCOS_SOI_EDGES, num_classes=80):
    gb, gc, gv, gs = names_or_arrays
    cfg = O.FCOSCfg(strides=list(strides), soi_edges=list(edges), num_classes=num_classes, center_sample=radius > 0, radius=radius)
    assert [[float(a), float(b)] for a, b in cfg.soi] == _soi(edges)
    locs = [O.compute_locations(h, w, s) for (h, w), s in zip(level_hw, strides)]
    gts, slot_of = [], []
    for n in range(len(gv)):
        s = np.nonzero(gv[n])[0]
        slot_of.append(s)
        gts.append(dict(boxes=T(gb[n][s]).float(), classes=T(gc[n][s]).long(), reg_pred_std=T(gs[n][s]).float()))
    out = O.fcos_targets(cfg, locs, gts, ignore_near=bool(drop_empty & 2))
    lab = torch.cat(out["labels"]).numpy().astype(np.int64)
    keep = torch.cat(out["keep_locations"]).numpy()
    reg, bv = torch.cat(out["reg_targets"]).numpy(), torch.cat(out["boundary_vars"]).numpy()
    ti = torch.cat(out["target_inds"]).numpy()
    # the oracle's target_inds count the compacted gts of the images before; bring them back to slots.  Image of every row:
    N = len(gv)
    img = np.concatenate([np.repeat(np.arange(N), h * w) for (h, w) in level_hw])
    base = np.concatenate([[0], np.cumsum([len(s) for s in slot_of])])
    slot = np.array([slot_of[n][t - base[n]] if len(slot_of[n]) else -1 for n, t in zip(img, ti)])
    empty = np.array([len(slot_of[n]) == 0 for n in img])
    drop = (~keep) & (empty & bool(drop_empty & 1) | ~empty)
    lab = np.where(drop, -1, lab)
    return lab.astype(np.int32), reg, bv, slot.astype(np.int32)


def _check_fcos(arrays, drop_empty, radius, **kw):
    gb, gc, gv, gs = arrays
    soi = _soi(kw.get("edges", R.FCOS_SOI_EDGES))
    got = R.fcos_targets(kw.get("level_hw", R.FCOS_HW), kw.get("strides", R.FCOS_STRIDES), soi, gb, gc, gv, gs, 80, drop_empty,
                         center_radius=radius)
    want = _oracle_fcos(arrays, drop_empty, radius, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    assert np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(_bits(got[2]), _bits(want[2]))
    return got


FCOS_PLAIN = ["edges", "one_inside", "soi_hi_l0", "soi_lo_l1", "soi_lo_l1_minus", "soi_hi_l1", "soi_hi_l1_plus", "area_tie", "area_tie_hole",
              "smaller_uncared", "empty"]
FCOS_CS = ["cs_radius", "cs_clip", "cs_quirk", "edges", "empty"]
# exact counts of the events of each image alone (drop_empty 0; radius 0 for the plain images, 1.5 for the cs_ ones)
FCOS_CENSUS = {
    "edges": dict(on_edge=10, positive=2),
    "one_inside": dict(one_inside=10, positive=12),
    "soi_hi_l0": dict(mx_eq_soi_hi=3, mx_above_soi_hi=1),
    "soi_lo_l1": dict(mx_eq_soi_lo=1),
    "soi_lo_l1_minus": dict(mx_below_soi_lo=1),
    "soi_hi_l1": dict(mx_eq_soi_hi=1),
    "soi_hi_l1_plus": dict(mx_above_soi_hi=1),
    "area_tie": dict(area_tie=1),
    "area_tie_hole": dict(area_tie=1),
    "smaller_uncared": dict(smaller_uncared=1),
    "empty": dict(empty_images=1, positive=0),
    "cs_radius": dict(cs_on_radius=12),
    "cs_clip": dict(cs_clipped=14, positive=2),
    "cs_quirk": dict(cs_quirk_images=1, positive=0),
}


@pytest.mark.parametrize("name", sorted(R.FCOS_IMAGES))
def test_fcos_image_hits_its_branch_with_an_exact_count(name):
    radius = 1.5 if name.startswith("cs_") else 0.0
    got = _check_fcos(R.fcos_pack([name]), 0, radius)
    census = got[4]
    print(name, {k: v for k, v in census.items() if v})
    for k, v in FCOS_CENSUS[name].items():
        assert census[k] == v, (name, k, census[k])


def test_fcos_branch_batches_equal_the_oracle_under_every_drop_rule():
    for drop_empty in (0, 1, 2, 3):
        _check_fcos(R.fcos_pack(FCOS_PLAIN), drop_empty, 0.0)
        got = _check_fcos(R.fcos_pack(FCOS_CS), drop_empty, 1.5)
        assert (got[4]["ignored"] > 0) == bool(drop_empty & 2)
    for MAXG, slot0 in ((1, 0), (256, 253)):          # valid slots only at the end of a full-width table
        names = ["edges", "empty"] if MAXG == 1 else FCOS_PLAIN
        got = _check_fcos(R.fcos_pack(names, MAXG, slot0), 0, 0.0)
        assert got[3].max() == slot0 + (0 if MAXG == 1 else 2)
    lab = R.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, *R.fcos_pack(["area_tie", "area_tie_hole", "smaller_uncared"]), 80, 0)
    p = R.fcos_locations(R.FCOS_HW, R.FCOS_STRIDES).index((0, 20, 20))     # level 0 rows are image-major: 260 per image
    assert [int(lab[3][n * 260 + p]) for n in range(3)] == [0, 1, 0] and [int(lab[0][n * 260 + p]) for n in range(3)] == [11, 13, 15]


def test_fcos_range_and_active_subset():
    """img0 / active / batch: gt arrays of 2 images placed at images 1, 2 of a batch of 4, image 2 switched off"""
    arrays = R.fcos_pack(["edges", "area_tie"])
    full = R.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, *arrays, 80, 0)
    sub = R.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, *arrays, 80, 0, active=[1, 1, 0, 1], batch=4, img0=1)
    assert sub[4]["inactive_images"] == 3
    off = 0
    for (h, w) in R.FCOS_HW:
        hw = h * w
        for k in range(4):
            a = sub[k][4 * off:4 * off + 4 * hw].reshape((4, hw) + sub[k].shape[1:])
            f = full[k][2 * off:2 * off + 2 * hw].reshape((2, hw) + full[k].shape[1:])
            assert np.array_equal(a[1], f[0])
            if k in (0, 3):
                assert (a[[0, 2, 3]] == -1).all()
            else:
                assert not a[[0, 2, 3]].any()
        off += hw


def test_fcos_targets_equal_the_oracle_on_random_integer_boxes():
    rng = np.random.default_rng(6)
    hw, strides = [(5, 6), (3, 3)], [8, 16]
    for seed in range(100):
        n, MAXG = 2, 4
        xy = rng.integers(-8, 40, size=(n, MAXG, 2))
        wh = rng.choice([8, 16, 24, 40, 72], size=(n, MAXG, 2))
        gb = np.concatenate([xy, xy + wh], axis=2).astype(np.float32)
        gv = (rng.random((n, MAXG)) < 0.6).astype(np.uint8)
        gc = rng.integers(0, 80, size=(n, MAXG)).astype(np.int32)
        gs = (rng.integers(1, 9, size=(n, MAXG, 4)) / 8).astype(np.float32)
        for radius in (0.0, 1.5):
            _check_fcos((gb, gc, gv, gs), int(rng.integers(0, 4)), radius, level_hw=hw, strides=strides, edges=[32])


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS against O.nms / O.batched_nms
def _oracle_nms(c, thr, aware):
    vi = torch.from_numpy(np.nonzero(c["valid"])[0])
    if len(vi) == 0:
        return []
    b, s = T(c["boxes"])[vi], T(c["scores"])[vi]
    k = O.batched_nms(b, s, T(c["classes"])[vi].long(), thr) if aware else O.nms(b, s, thr)
    return vi[k].tolist()


def _check_nms(c, thr, aware):
    keep, census = R.nms(c["boxes"], c["scores"], c["classes"], c["valid"], thr, aware)
    assert keep == _oracle_nms(c, thr, aware)
    return keep, census


NMS_SIZES = [(1, 1), (64, 64), (65, 64), (65, 65), (128, 64), (128, 65), (128, 128), (129, 65), (129, 129), (192, 192)]


@pytest.mark.parametrize("M,nvalid", NMS_SIZES)
def test_nms_structured_cases_hit_their_branches_and_equal_the_oracle(M, nvalid):
    for aware, ncls in ((False, 1), (True, 3)):
        c = R.nms_structured_case(M, nvalid, seed=M * 7 + nvalid, ncls=ncls)
        keep, census = _check_nms(c, 0.6, aware)
        assert census["n_valid"] == nvalid
        if nvalid >= 64:
            # 1 and 6 suppressed, 3 kept at exactly 6/10, 8 kept; 7 suppressed only when classes are ignored; 130 by 12 across a chunk
            assert census["iou_eq_thr"] == 1
            assert census["suppressed"] == 2 + (not aware) + (nvalid > 130)
            assert census["score_tie"] == 2 + (nvalid > 64)
            assert len(keep) == nvalid - census["suppressed"]


def test_nms_random_bucket_and_zero_sign_cases_equal_the_oracle():
    hits = 0
    for seed in range(150):
        M = [1, 5, 30, 64, 65, 100][seed % 6]
        c = R.nms_random_case(M, seed, ncls=3, nvalid=None if seed % 2 else max(1, M - 3))
        for thr in (0.5, 0.6):
            for aware in (False, True):
                hits += _check_nms(c, thr, aware)[1]["iou_eq_thr"]
    assert hits > 50                                   # integer boxes land ON the threshold all the time
    keep, census = _check_nms(R.nms_bucket_case(), 0.5, True)
    cl = R.nms_bucket_case()["classes"]
    assert (cl % 32 == 3).sum() == 64 and (cl % 32 == 5).sum() == 65 and census["suppressed"] > 0
    c = R.nms_zero_sign_case()
    for aware in (False, True):
        keep, census = _check_nms(c, 0.5, aware)
        assert keep == [0, 2, 3] and census["zero_sign_tie"] == 3
    # a pair at exactly 1/2 is kept at thr 0.5, one unit more is suppressed
    two = dict(boxes=np.array([[0, 0, 10, 10], [0, 0, 10, 5]], np.float32), scores=np.array([1, 0.5], np.float32),
               classes=np.zeros(2, np.int32), valid=np.ones(2, np.uint8))
    assert _check_nms(two, 0.5, False)[0] == [0, 1]
    two["boxes"][1, 3] = 6
    assert _check_nms(two, 0.5, False)[0] == [0]


def test_nms_truncation_and_kthvalue_rule():
    c = R.nms_structured_case(192, 192, seed=9)
    full, _ = R.nms(c["boxes"], c["scores"], c["classes"], c["valid"], 0.6, False)
    K = len(full)
    sc = c["scores"]
    assert R.nms(c["boxes"], sc, c["classes"], c["valid"], 0.6, False, post_topk=K, max_out=K)[0] == full
    assert R.nms(c["boxes"], sc, c["classes"], c["valid"], 0.6, False, post_topk=K - 1, max_out=K)[0] == full[:K - 1]
    assert R.nms(c["boxes"], sc, c["classes"], c["valid"], 0.6, False, max_out=50)[0] == full[:50]
    t = R.kth_tie_index(full, sc)
    assert sc[full[t - 1]] == sc[full[t]] and sc[full[t]] > sc[full[t + 1]]
    assert R.nms(c["boxes"], sc, c["classes"], c["valid"], 0.6, False, post_topk=t, max_out=K)[0] == full[:t + 1]
    assert R.nms(c["boxes"], sc, c["classes"], c["valid"], 0.6, False, post_topk=t, max_out=t)[0] == full[:t]


# ---------------------------------------------------------------------------------------------------------------------------------
# top-k and decode
@pytest.mark.parametrize("k", [1, 2, 1000, 8192])
def test_topk_case_hits_its_branches_and_equals_torch_topk(k):
    flat, off, width, census = R.topk_case(k)
    assert census == dict(rows=8, zero_width=1, k_minus_1=1, k_exact=1, k_plus_1=1, just_over_4096=2 if k <= 2 else 1, one_list=k + 1,
                          bit62=1) and width >= 4100
    got = R.topk_rows(flat, off, k)
    for r in range(8):
        row = T(flat[off[r]:off[r + 1]])
        assert len(set(row[row >= 0].tolist())) == int((row >= 0).sum())       # distinct keys: the answer is unique
        kk = min(k, len(row))
        ref = torch.topk(row, kk).values if kk else row
        ref = torch.where(ref >= 0, ref, torch.full_like(ref, -1))
        assert np.array_equal(got[r, :kk], ref.numpy()) and (got[r, kk:] == -1).all()


def test_decode_case_hits_its_branches_and_equals_the_oracle():
    c = R.decode_case()
    N, A, hw = c["N"], R.DEC_A, R.DEC_HW
    keys = R.rpn_rank_keys(c["head"], hw, N, A)
    widths = [h * A for h in hw]
    off = np.array([0] + list(np.cumsum([w for w in widths for _ in range(N)])), dtype=np.int64)
    top = R.topk_rows(keys, off, max(widths))
    top[1, 3] = -1                                     # an empty candidate slot
    boxes, scores, lvls, keep, census = R.rpn_decode(top, c["head"], c["anchors"], c["image_hw"], hw, widths, N, A, R.DEC_MIN)
    print(census)
    # 8 = the six 4-wide second anchors of image 0 that stay inside W (pixel 2's is 5 wide), the box clipped exactly to W = 96 and
    # the box clipped to 0; 13 corners beyond W / H; 15 of the 32 candidates kept
    assert census == dict(empty=1, nonfinite=2, w_eq_min=8, w_min_plus1=2, clip_hi=13, clip_lo=2, kept=15)
    with R.flipped("decode_min"):
        assert R.rpn_decode(top, c["head"], c["anchors"], c["image_hw"], hw, widths, N, A, R.DEC_MIN)[3].sum() > keep.sum()
    # the same candidates through the oracle's apply_deltas + clip + keep (find_top_rpn_proposals with min size DEC_MIN)
    row0 = a0 = o0 = 0
    for l, (n_pix, k) in enumerate(zip(hw, widths)):
        for n in range(N):
            for j in range(k):
                key = int(top[l * N + n, j])
                if key < 0:
                    assert keep[n, o0 + j] == 0 and not boxes[n, o0 + j].any()
                    continue
                idx = (1 << 31) - 1 - (key & ((1 << 31) - 1))
                p, a = divmod(idx, A)
                row = T(c["head"][row0 + n * n_pix + p])
                b = O.rpn_apply_deltas(row[A + 4 * a:A + 4 * a + 4][None], T(c["anchors"][a0 + idx])[None])[0]
                H, W = c["image_hw"][n]
                fin = bool(torch.isfinite(b).all() and torch.isfinite(row[a]))
                bc = torch.stack((b[0].clamp(0, W), b[1].clamp(0, H), b[2].clamp(0, W), b[3].clamp(0, H)))
                assert np.array_equal(np.nan_to_num(boxes[n, o0 + j], nan=-7), np.nan_to_num(bc.numpy(), nan=-7))
                assert bool(keep[n, o0 + j]) == (fin and bool(bc[2] - bc[0] > R.DEC_MIN) and bool(bc[3] - bc[1] > R.DEC_MIN))
                assert scores[n, o0 + j] == (row[a] if fin else 0) and lvls[n, o0 + j] == l
        row0 += N * n_pix
        a0 += n_pix * A
        o0 += k


# ---------------------------------------------------------------------------------------------------------------------------------
# every one-token flip of a comparison changes what some branch case expects
def _expect_all():
    out = {}
    inp, _ = R.matcher_threshold_case()
    mx, arg, gmax, lq = R.match_all(inp["boxes"], inp["gt_boxes"], inp["gt_valid"])
    out["match"] = (mx.tobytes(), arg.tobytes())
    zero = np.zeros(40)
    out["rpn"] = [R.rpn_labels_and_sample(mx[n], lq[n] * 0, bool(inp["gt_valid"][n].any()), zero, 0.3, 0.7, 4, 8)[0].tobytes() for n in range(7)]
    gc = np.arange(4)
    out["roi"] = R.roi_sample(inp["boxes"], np.ones(40), mx[0], arg[0], zero, inp["gt_boxes"][0], gc, inp["gt_valid"][0], zero, np.zeros((4, 4)),
                              0.5, 80, 16, 4)["gt_classes"].tobytes()
    f = R.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, *R.fcos_pack(FCOS_PLAIN), 80, 0)
    out["fcos"] = (f[0].tobytes(), f[3].tobytes())
    c = R.nms_structured_case(65, 65, seed=1)
    out["nms"] = R.nms(c["boxes"], c["scores"], c["classes"], c["valid"], 0.6, False)[0]
    return out


@pytest.mark.parametrize("rule,part", [("match_first", "match"), ("rpn_hi", "rpn"), ("rpn_lo", "rpn"), ("roi_thr", "roi"),
                                       ("fcos_inside", "fcos"), ("fcos_soi_hi", "fcos"), ("fcos_soi_lo", "fcos"), ("fcos_first", "fcos"),
                                       ("nms_thr", "nms")])
def test_every_flipped_comparison_changes_an_expected_output(rule, part):
    base = _expect_all()
    with R.flipped(rule):
        mut = _expect_all()
    assert mut[part] != base[part]
    assert all(mut[k] == base[k] for k in base if k != part and not (part == "match" and k in ("rpn", "roi")))
