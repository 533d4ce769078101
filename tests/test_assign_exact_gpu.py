"""The decision kernels - match_boxes / match_lowq, the RPN and ROI samplers, fcos_targets, the NMS pipeline, the radix top-k and the
RPN decode - on inputs that sit exactly ON their comparisons (tests/assign_ref.py): an IoU equal to a threshold, a location on a box
edge, a regress distance equal to a size-of-interest bound, equal areas, equal IoUs, equal scores, counts of 64 / 65 / k / max_out.  All
coordinates are small integers, so fp32 is exact and every comparison below is equality of integers, bytes or fp32 bit patterns; the
expected values come from the plain Python reference, which tests/test_assign_ref.py holds against the oracle on the CPU."""
import numpy as np
import pytest
import torch

from tests import assign_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def same(got, want):
    """bitwise equality of a device tensor and a numpy array of the same dtype"""
    g = got.cpu().numpy()
    w = np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    ok = g.tobytes() == w.tobytes()
    if not ok:                                         # what differs, for the log
        bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
        print("mismatch: %d of %d, first at %s: got %r want %r" % (len(bad), g.size, bad[:4].tolist(), g[tuple(bad[0])] if len(bad) else None,
                                                                   w[tuple(bad[0])] if len(bad) else None))
    return ok


# ---------------------------------------------------------------------------------------------------------------------------------
# matcher
def _match_gpu(inp):
    from ubteacher import hip
    boxes, gb, gv = cu(inp["boxes"]), cu(inp["gt_boxes"]), cu(inp["gt_valid"])
    mx, arg, gmax = hip.match_boxes(boxes, gb, gv, want_gt_max=True)
    lq = hip.match_lowq(boxes, gb, gv, gmax)
    return mx, arg, gmax, lq


def _check_match(inp):
    mx, arg, gmax, lq = _match_gpu(inp)
    rmx, rarg, rgmax, rlq = R.match_all(inp["boxes"], inp["gt_boxes"], inp["gt_valid"])
    assert same(mx, rmx) and same(arg, rarg) and same(gmax, rgmax.view(np.int32)) and same(lq, rlq)
    return rmx, rarg, rlq


def test_box_iou_is_bit_equal_on_integer_boxes():
    from ubteacher import hip
    rng = np.random.default_rng(0)
    inp, _ = R.matcher_threshold_case()
    for a, b in ((inp["boxes"], inp["gt_boxes"][0]), (R.random_int_boxes(rng, 37), R.random_int_boxes(rng, 300)),
                 (R.random_int_boxes(rng, 9), R.random_int_boxes(rng, 1))):
        assert same(hip.box_iou(cu(a), cu(b)), R.pairwise_iou(a, b))


def test_matcher_on_thresholds_ties_untouched_and_degenerate_gts():
    inp, census = R.matcher_threshold_case()
    assert len(census) == 7
    mx, arg, lq = _check_match(inp)
    assert list(arg[0, :4]) == [0, 1, 2, 3] and arg[1, 5] == 0 and arg[2, 5] == 1 and lq[3].all() and mx[5].max() == -1


@pytest.mark.parametrize("G", [1, 64, 65, 256])
@pytest.mark.parametrize("P", [1, 256, 257])
def test_matcher_on_wave_and_block_boundaries(G, P):
    ncases = 0
    for per_image in (False, True):
        inp, census = R.matcher_boundary_case(G, P, per_image)
        assert census[0]["max_only_at_last"] == census[0]["n_valid"] > 0
        _check_match(inp)
        ncases += 1
    assert ncases == 2


def test_matcher_dense_random_integer_boxes():
    rng = np.random.default_rng(8)
    G, P = 70, 300
    inp = dict(boxes=R.random_int_boxes(rng, P), gt_boxes=np.stack([R.random_int_boxes(rng, G) for _ in range(2)]),
               gt_valid=(rng.random((2, G)) < 0.8).astype(np.uint8))
    mx, arg, lq = _check_match(inp)
    ties = sum(R.match_census(inp["boxes"], inp["gt_boxes"][n], inp["gt_valid"][n])["argmax_tie"] for n in range(2))
    assert ties == 20      # integer boxes: equal IoUs are the rule, not the exception


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN sampler
@pytest.mark.parametrize("with_lowq", [True, False])
def test_rpn_sampler_on_thresholds_lowq_overrides_empty_images_and_equal_keys(with_lowq):
    """the seven images of the matcher threshold case in ONE launch (image 5 has no gt).  (npos_max, batch): (4, 8) more positives than
    npos_max; (4, 4) a negative room of exactly 0; (16, 64) fewer candidates than slots.  The counts are those test_assign_ref.py pins."""
    from ubteacher import hip
    from tests.test_assign_ref import RPN_SAMPLER_CENSUS
    inp, want, census = R.rpn_sampler_case(with_lowq)
    assert census == RPN_SAMPLER_CENSUS[with_lowq]
    N = len(inp["mx"])
    ncases = 0
    for npos_max, batch in R.RPN_SAMPLER_CONFIGS:
        pidx, pval, nidx, nval, has_gt = hip.rpn_sample(cu(inp["mx"]), cu(inp["lowq"]), cu(inp["gt_valid"]), cu(inp["keys"]), 0.3, 0.7,
                                                        npos_max, batch)
        for n in range(N):
            lab, rpi, rpv, rni, rnv = want[(npos_max, batch, n)]
            assert same(pval[n], rpv) and same(nval[n], rnv) and int(has_gt[n]) == bool(inp["gt_valid"][n].any())
            assert same(pidx[n] * pval[n], rpi) and same(nidx[n] * nval[n], rni)
            ncases += 1
    assert ncases == 21


# ---------------------------------------------------------------------------------------------------------------------------------
# ROI sampler
@pytest.mark.parametrize("P", [1, 511, 512, 513])
def test_roi_sampler_on_the_threshold_the_sort_width_and_the_foreground_cap(P):
    """R.roi_case: proposal 0 of image 0 at IoU exactly 1/2 (foreground), an image without gt, invalid slots between valid ones, nfg_max
    equal to the foreground count of image 0 and one less; the census is the one test_assign_ref.py pins"""
    from ubteacher import hip
    from tests.test_assign_ref import ROI_CENSUS, roi_caps
    c, census = R.roi_case(P)
    assert census == ROI_CENSUS[P] and c["mx"][0, 0] == np.float32(0.5) and c["arg"][0, 0] == 0
    B, caps = roi_caps(census)
    ncases = 0
    for nfg_max in caps:
        got = hip.roi_sample(cu(c["boxes"]), cu(c["valid"]), cu(c["mx"]), cu(c["arg"]), cu(c["keys"]), cu(c["gb"]), cu(c["gc"]), cu(c["gv"]),
                             cu(c["gs"]), cu(c["gstd"]), 0.5, R.ROI_CLASSES, B, nfg_max)
        for n in range(3):
            want = R.roi_sample_image(c, n, B, nfg_max)
            for name in ("proposal_boxes", "gt_classes", "gt_boxes", "valid", "sampled_idx", "gt_confid", "gt_loc_std"):
                assert same(got[name][n], want[name]), (name, n, nfg_max)
            if n == 0:
                assert want["nfg"] == min(census["nfg"][0], nfg_max)
            if n == 1:
                assert want["nfg"] == 0 and not want["gt_boxes"].any()          # has_gt false: all background, zero gt box
            if n == 2 and P > 1:
                assert not np.isin(want["sampled_idx"][want["valid"] == 1], np.arange(1, P, 3)).any()
            ncases += 1
    assert ncases == 3 * len(caps)


# ---------------------------------------------------------------------------------------------------------------------------------
# FCOS targets
FCOS_PLAIN = ["edges", "one_inside", "soi_hi_l0", "soi_lo_l1", "soi_lo_l1_minus", "soi_hi_l1", "soi_hi_l1_plus", "area_tie", "area_tie_hole",
              "smaller_uncared", "empty"]
FCOS_CS = ["cs_radius", "cs_clip", "cs_quirk", "edges", "empty"]


def _check_fcos(arrays, drop_empty, radius, **kw):
    from ubteacher import hip
    gb, gc, gv, gs = arrays
    act = kw.get("active")
    got = hip.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, cu(gb), cu(gc), cu(gv), cu(gs), 80, drop_empty,
                           active=None if act is None else cu(np.array(act, np.uint8)), center_radius=radius, batch=kw.get("batch"),
                           img0=kw.get("img0", 0))
    want = R.fcos_targets(R.FCOS_HW, R.FCOS_STRIDES, R.FCOS_SOI, gb, gc, gv, gs, 80, drop_empty, active=act, center_radius=radius,
                          batch=kw.get("batch"), img0=kw.get("img0", 0))
    for k, name in enumerate(("labels", "reg_targets", "bvars", "gt_inds")):
        assert same(got[k], want[k]), (name, drop_empty, radius)
    return want


@pytest.mark.parametrize("drop_empty", [0, 1, 2, 3])
def test_fcos_targets_on_edges_size_bounds_and_area_ties(drop_empty):
    assert sum(h * w for h, w in R.FCOS_HW) == 350        # not a multiple of 256; the level boundary 260 lies inside block 1
    want = _check_fcos(R.fcos_pack(FCOS_PLAIN), drop_empty, 0.0)
    c = want[4]
    assert c["on_edge"] == 75 and c["one_inside"] == 10 and c["mx_eq_soi_hi"] == 4 and c["mx_eq_soi_lo"] == 1 and c["area_tie"] == 2
    assert c["mx_above_soi_hi"] == 2 and c["mx_below_soi_lo"] == 1 and c["smaller_uncared"] == 1 and c["empty_images"] == 1
    lab = want[0][:11 * 260].reshape(11, 260)
    assert ((lab[10] == -1).all() if drop_empty & 1 else (lab[10] == 80).all()) and c["ignored"] == 0


@pytest.mark.parametrize("drop_empty", [0, 2])
def test_fcos_targets_centre_sampling_radius_clip_quirk_and_ignored_locations(drop_empty):
    c = _check_fcos(R.fcos_pack(FCOS_CS), drop_empty, 1.5)[4]
    assert c["cs_on_radius"] == 12 and c["cs_clipped"] == 31 and c["cs_quirk_images"] == 1 and c["ignored"] == (110 if drop_empty else 0)


def test_fcos_targets_gt_table_widths_and_image_subsets():
    want = _check_fcos(R.fcos_pack(["edges", "empty"], 1, 0), 0, 0.0)
    assert want[3].max() == 0
    want = _check_fcos(R.fcos_pack(FCOS_PLAIN, 256, 253), 0, 0.0)          # valid slots only at 253 .. 255
    assert sorted(set(want[3].tolist())) == [-1, 253, 254, 255]
    want = _check_fcos(R.fcos_pack(["edges", "area_tie"]), 0, 0.0, active=[1, 1, 0, 1], batch=4, img0=1)
    assert want[4]["inactive_images"] == 3 and want[4]["positive"] > 0
    want = _check_fcos(R.fcos_pack(["edges", "area_tie"]), 1, 0.0, active=[1, 1], batch=2, img0=0)
    assert want[4]["inactive_images"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# NMS
def _nms_gpu(cases, thr, aware, post_topk, max_out):
    """the cases (equal M) as the images of one launch -> list of kept-slot lists"""
    from ubteacher import hip
    stack = lambda k: np.stack([c[k] for c in cases])
    keep, cnt = hip.nms_batched(cu(stack("boxes")), cu(stack("scores")), cu(stack("classes")), cu(stack("valid")), thr,
                                class_aware=aware, post_topk=post_topk, max_out=max_out)
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    out = []
    for n in range(len(cases)):
        assert (keep[n, cnt[n]:] == -1).all()
        out.append(keep[n, :cnt[n]].tolist())
    return out


def _check_nms(cases, thr, aware, post_topk=-1, max_out=None):
    M = len(cases[0]["scores"])
    mo = M if max_out is None else max_out
    got = _nms_gpu(cases, thr, aware, post_topk, mo)
    want = [R.nms(c["boxes"], c["scores"], c["classes"], c["valid"], thr, aware, post_topk, mo)[0] for c in cases]
    assert got == want, (thr, aware, post_topk, max_out)
    return want


NMS_SIZES = [(1, 1), (64, 64), (65, 64), (65, 65), (128, 64), (128, 65), (128, 128), (129, 65), (129, 129), (192, 192)]


@pytest.mark.parametrize("aware", [False, True])
@pytest.mark.parametrize("M,nvalid", NMS_SIZES)
def test_nms_on_the_threshold_score_ties_and_chunk_boundaries(M, nvalid, aware):
    """image 0: the structured case (IoU exactly 6/10 kept, 7/10 suppressed, a suppressed box that cannot suppress, identical boxes of
    two classes, equal scores in slot order, chunk 0 -> chunk 2 suppression); image 1: dense random integer boxes with score ties."""
    cases = [R.nms_structured_case(M, nvalid, seed=M * 7 + nvalid, ncls=3 if aware else 1), R.nms_random_case(M, M + nvalid, 3, nvalid)]
    full = _check_nms(cases, 0.6, aware)
    _check_nms(cases, 0.5, aware)
    K = len(full[0])
    ncases = 2
    for post, mo in ((K, None), (max(K - 1, 1), None), (-1, max(K // 2, 1)), (max(K // 2, 1), max(K - 1, 1)), (3, 2)):
        _check_nms(cases, 0.6, aware, post, mo)
        ncases += 1
    if nvalid > 64 and not aware:
        t = R.kth_tie_index(full[0], cases[0]["scores"])          # the k-th score is shared across the chunk boundary 63 | 64
        assert _check_nms(cases, 0.6, aware, t, None)[0] == full[0][:t + 1]
        assert _check_nms(cases, 0.6, aware, t, t)[0] == full[0][:t]
        ncases += 2
    assert ncases == 7 + 2 * (nvalid > 64 and not aware)


def test_nms_buckets_of_64_and_65_pairs_on_the_threshold_and_signed_zero_scores():
    _check_nms([R.nms_bucket_case()], 0.5, True)
    _check_nms([R.nms_bucket_case()], 0.5, True, post_topk=20, max_out=40)
    two = dict(boxes=np.array([[0, 0, 10, 10], [0, 0, 10, 5]], np.float32), scores=np.array([1, 0.5], np.float32),
               classes=np.zeros(2, np.int32), valid=np.ones(2, np.uint8))
    over = dict(two, boxes=np.array([[0, 0, 10, 10], [0, 0, 10, 6]], np.float32))
    for aware in (False, True):
        assert _check_nms([two, over], 0.5, aware) == [[0, 1], [0]]           # 1/2 at thr 0.5 kept; one unit more suppressed
        # -0.0 and +0.0 are EQUAL scores: the slot decides, slot 0 (-0.0) is kept and suppresses its copy in slot 1
        assert _check_nms([R.nms_zero_sign_case()], 0.5, aware) == [[0, 2, 3]]


# ---------------------------------------------------------------------------------------------------------------------------------
# top-k and the RPN decode
@pytest.mark.parametrize("k", [1, 2, 3, 1000, 8192])
def test_topk_rows_on_k_boundaries_digits_and_row_shapes(k):
    from ubteacher import hip
    flat, off, width, census = R.topk_case(k)
    assert census["rows"] == 8 and census["zero_width"] == 1 and census["k_exact"] == census["k_minus_1"] == census["k_plus_1"] == 1 and census["one_list"] == k + 1
    want = R.topk_rows(flat, off, k)
    got = hip.topk_rows(cu(flat), cu(off), 8, width, k)
    assert same(got, want)
    assert torch.equal(hip.topk_rows(cu(flat), cu(off), 8, width, k), got)


def test_rpn_rank_keys_topk_and_decode_on_min_size_clip_and_non_finite_values():
    from ubteacher import hip
    c = R.decode_case()
    N, A, hw = c["N"], R.DEC_A, R.DEC_HW
    widths = [h * A for h in hw]
    head = cu(c["head"])
    keys = hip.rpn_rank_keys(head, hw, N, A)
    rkeys = R.rpn_rank_keys(c["head"], hw, N, A)
    assert same(keys, rkeys)
    off = np.array([0] + list(np.cumsum([w for w in widths for _ in range(N)])), dtype=np.int64)
    top = hip.topk_rows(keys, cu(off), len(hw) * N, max(widths), max(widths))
    rtop = R.topk_rows(rkeys, off, max(widths))
    assert same(top, rtop)
    rtop[1, 3] = -1                                    # an empty candidate slot
    boxes, scores, lvls, keep = hip.rpn_decode(cu(rtop), head, cu(c["anchors"]), cu(c["image_hw"]), hw, widths, N, A, (1.0, 1.0, 1.0, 1.0),
                                               4.135, R.DEC_MIN)
    rb, rs, rl, rk, census = R.rpn_decode(rtop, c["head"], c["anchors"], c["image_hw"], hw, widths, N, A, R.DEC_MIN)
    assert census == dict(empty=1, nonfinite=2, w_eq_min=8, w_min_plus1=2, clip_hi=13, clip_lo=2, kept=15)
    assert same(keep, rk) and same(lvls, rl) and same(scores, rs)
    nan = np.isnan(rb)
    assert nan.sum() == 2 and same(torch.isnan(boxes), nan) and same(torch.nan_to_num(boxes, nan=0.0), np.nan_to_num(rb, nan=0.0))
