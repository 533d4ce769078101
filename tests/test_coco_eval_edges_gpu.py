"""csrc/coco_eval.hip at its decision points and size edges, against the independent oracle tests/coco_ref.py (never against the host
restatement): every known-answer case and structured split of test_coco_ref.py through device_box_eval, with the match / ignore bit
of every (detection, area, threshold) read back from the workspace; the taken-word, max_dets, chunk, wave and thread edges of the match
and accumulate kernels; the key, offset and rank kernels alone; the entry points' refusals; DeviceCOCOBoxEvaluator.
All inputs are small integers, all comparisons exact."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
sys.path.insert(0, ROOT)

from tests import coco_ref as ref  # noqa: E402
from tests.test_coco_ref import CASES, SCORE_LIST, SEEDS, image, oracle, split, twice_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 0xA5
GRID_STRIDE_N = 4096 * 256 + 3          # one element more than 4096 blocks of 256 threads cover (+ 2)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align256(n):
    return (n + 255) & ~255


def device_chain(pred, gt, K, max_dets=100):
    """hip.coco_box_eval's call chain through the C ABI on device_box_eval's packing, keeping what the chain leaves in the workspace
    (layout: csrc/coco_eval.hip, utv2_coco_match - mbits at 0, ibits after align256(8 D), bit a * 10 + t of the word of each position
    of the pair order).  The workspace starts as SENTINEL bytes.  Returns precision, recall and, per image in gt's order,
    matched / ignored bool [D, 4, 10] and scored bool [D] in the image's detection order, and `untouched` bool [D]: both words of the
    detection still hold the sentinel."""
    from ubteacher import hip
    from ubteacher.evaluation.coco_eval import AREA_NAMES, AREA_RNG, IOU_THRS, REC_THRS
    db, ds, dc, dl, gb, gc, gcr, ga, gl = [], [], [], [], [], [], [], [], []
    for img, g in gt.items():
        b = np.asarray(g["boxes"], float).reshape(-1, 4)
        c = np.asarray(g["classes"]).reshape(-1)
        gb.append(b)
        gc.append(c)
        gcr.append(np.asarray(g.get("iscrowd", np.zeros(len(c))), bool).reshape(-1))
        ga.append(np.asarray(g["area"], float).reshape(-1) if g.get("area") is not None else (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
        gl.append(len(c))
        p = pred.get(img)
        n = len(np.asarray(p["classes"]).reshape(-1)) if p is not None else 0
        if n:
            db.append(np.asarray(p["boxes"], F32).reshape(-1, 4))
            ds.append(np.asarray(p["scores"], F32).reshape(-1))
            dc.append(np.asarray(p["classes"]).reshape(-1))
        dl.append(n)
    cat = lambda xs, shape, dt: _dev(np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt))  # noqa: E731
    off = lambda lens: _dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))  # noqa: E731
    dbox, dscore, dcls, doff = cat(db, (0, 4), F32).reshape(-1, 4), cat(ds, 0, F32), cat(dc, 0, np.int32), off(dl)
    gbox, gcrowd, garea, gcls, goff = cat(gb, (0, 4), np.float64).reshape(-1, 4), cat(gcr, 0, np.uint8), cat(ga, 0, np.float64), \
        cat(gc, 0, np.int32), off(gl)
    N, D, G = len(gl), int(dscore.numel()), int(gcls.numel())
    npair = N * (K + 1)
    i64 = dict(dtype=torch.int64, device="cuda")
    call, p_, st = hip.call, hip._p, hip._stream()

    def sorted_pairs(scores, cls, offs, n):
        keys = torch.empty(n, **i64)
        if n:
            call("utv2_coco_pair_keys", p_(scores) if scores is not None else None, p_(cls), p_(offs), N, K, p_(keys), st)
        keys, perm = torch.sort(keys, stable=True)
        poff = torch.empty(npair + 1, **i64)
        call("utv2_coco_seg_offsets", p_(keys), n, npair, p_(poff), st)
        return keys, perm, poff

    key1, dperm, dpoff = sorted_pairs(dscore, dcls, doff, D)
    _, gperm, gpoff = sorted_pairs(None, gcls, goff, G)
    key2 = torch.empty(D, **i64)
    rank = torch.empty(D, dtype=torch.uint8, device="cuda")
    call("utv2_coco_rank_keys", p_(key1), p_(dpoff), D, K, max_dets, p_(key2), p_(rank), st)
    key2, perm2 = torch.sort(key2, stable=True)
    cat_off = torch.empty(K + 1, **i64)
    call("utv2_coco_seg_offsets", p_(key2), D, K, p_(cat_off), st)
    nbytes = int(hip.load().utv2_coco_eval_workspace_bytes(D, K))
    assert nbytes == 2 * _align256(8 * max(D, 1)) + _align256(16 * K)
    ws = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    area_flat = [v for a in AREA_NAMES for v in AREA_RNG[a]]
    dbl = lambda vals: ctypes.cast((ctypes.c_double * len(vals))(*[float(v) for v in vals]), ctypes.c_void_p)  # noqa: E731
    call("utv2_coco_match", p_(dbox), p_(dperm), p_(dpoff), p_(gbox), p_(gcrowd), p_(garea), p_(gperm), p_(gpoff), N, K, D, max_dets,
         max(gl, default=0), dbl(IOU_THRS), dbl(area_flat), p_(ws), st)
    precision = torch.empty((10, 101, K, 4), dtype=torch.float64, device="cuda")
    recall = torch.empty((10, K, 4, 3), dtype=torch.float64, device="cuda")
    call("utv2_coco_accumulate", p_(perm2), p_(cat_off), p_(rank), K, D, dbl(REC_THRS), p_(ws), p_(precision), p_(recall), st)
    host = ws.cpu().numpy()
    stride = _align256(8 * max(D, 1))
    words = [host[o:o + 8 * D].view(np.uint64) for o in (0, stride)]
    perm, rk = dperm.cpu().numpy(), rank.cpu().numpy()
    flat = [np.zeros(D, np.uint64) for _ in range(2)]
    flat_scored = np.zeros(D, bool)
    for w, f in zip(words, flat):
        f[perm] = w
    flat_scored[perm] = rk != 255
    sent = np.uint64(int.from_bytes(bytes([SENTINEL]) * 8, "little"))
    shifts = np.arange(40, dtype=np.uint64).reshape(1, 4, 10)
    out = dict(precision=precision.cpu().numpy(), recall=recall.cpu().numpy(), matched={}, ignored={}, scored={}, untouched={})
    o = 0
    for img, n in zip(gt, dl):
        sl = slice(o, o + n)
        out["matched"][img] = ((flat[0][sl].reshape(-1, 1, 1) >> shifts) & np.uint64(1)).astype(bool)
        out["ignored"][img] = ((flat[1][sl].reshape(-1, 1, 1) >> shifts) & np.uint64(1)).astype(bool)
        out["scored"][img] = flat_scored[sl]
        out["untouched"][img] = (flat[0][sl] == sent) & (flat[1][sl] == sent)
        o += n
    return out


AREAS = ("all", "small", "medium", "large")


def assert_device_equals_oracle(pred, gt, K, r, arrays_from_box_eval=True):
    """precision / recall (device_box_eval's and the chain's) and every (detection, area, threshold) bit against the oracle result r"""
    from ubteacher.evaluation.coco_eval_device import device_box_eval
    d = device_chain(pred, gt, K)
    for img in gt:
        assert np.array_equal(d["scored"][img], r["scored"][img]), ("scored", img, np.nonzero(d["scored"][img] != r["scored"][img])[0][:8])
        s = r["scored"][img]
        # a detection that is not scored (foreign class, beyond its pair's 100 best) is never written
        assert np.all(d["untouched"][img][~s]), ("written though not scored", img, np.nonzero(~d["untouched"][img] & ~s)[0][:8])
        for name, rule in (("matched", "dtm"), ("ignored", "dtIg")):
            bad = np.argwhere(d[name][img][s] != r[name][img][s])
            if len(bad):
                i, a, t = bad[0]
                det = int(np.nonzero(s)[0][i])
                raise AssertionError("%s: image %r detection %d area %s IoU threshold %.2f: device %d, oracle %d (%d bits differ)" % (
                    rule, img, det, AREAS[a], ref.IOU_THRS[t], d[name][img][det, a, t], r[name][img][det, a, t], len(bad)))
    srcs = [("chain", d["precision"], d["recall"])]
    if arrays_from_box_eval:
        p, q, stats = device_box_eval(pred, gt, K)
        srcs.append(("device_box_eval", p, q))
        for k in r["stats"]:
            assert stats[k] == r["stats"][k], (k, stats[k], r["stats"][k])
    for name, p, q in srcs:
        assert np.array_equal(q, r["recall"]), (name, "recall [t, k, a, m]", np.argwhere(q != r["recall"])[:8])
        assert np.array_equal(p, r["precision"]), (name, "precision [t, r, k, a]", np.argwhere(p != r["precision"])[:8])


@pytest.mark.parametrize("name", list(CASES) + SEEDS)
def test_cases_and_structured_splits_equal_oracle(name):
    pred, gt, K, r = oracle(name)
    assert_device_equals_oracle(pred, gt, K, r)


# ------------------------------------------------------------------------------------------------------------------------------------
# match kernel sizes: the taken words (32 ground-truth boxes each) and the max_dets cut
def _grid_box(g):
    return [20 * (g % 16), 20 * (g // 16), 20 * (g % 16) + 10, 20 * (g // 16) + 10]


@pytest.mark.parametrize("ng", [1, 31, 32, 33, 64, 65, 96, 97])
def test_match_taken_words(ng):
    """ng boxes of one pair, each with an exact detection, delivered (and scored) in reverse box order, so the bit being set walks down
    through every word edge; a second, lower-scored copy of every detection finds its box taken"""
    gts = [(_grid_box(g), 0, 0, None) for g in range(ng)]
    dets = [(_grid_box(g), F32(1.0) - F32(ng - 1 - g) / 256, 0) for g in reversed(range(ng))]
    dets += [(_grid_box(g), F32(0.5) - F32(g) / 256, 0) for g in range(ng)]
    pred, gt = split({"i": image(dets, gts)})
    r = ref.evaluate(pred, gt, 1)
    assert np.all(r["matched"]["i"][:ng, 0]) and not np.any(r["matched"]["i"][ng:, 0])       # what the case is built for
    assert_device_equals_oracle(pred, gt, 1, r, arrays_from_box_eval=False)


def test_match_only_the_33rd_box_overlapped():
    gts = [(_grid_box(g), 0, 0, None) for g in range(33)]
    dets = [(_grid_box(32), 0.9, 0), (_grid_box(32), 0.8, 0), (_grid_box(32), 0.7, 0)]
    pred, gt = split({"i": image(dets, gts)})
    r = ref.evaluate(pred, gt, 1)
    assert [bool(r["matched"]["i"][d, 0, 0]) for d in range(3)] == [True, False, False]
    assert_device_equals_oracle(pred, gt, 1, r, arrays_from_box_eval=False)


@pytest.mark.parametrize("nd", [1, 99, 100, 101, 150])
def test_match_detections_per_pair(nd):
    """one pair of nd detections: class 0 has its true positive at the last rank (dropped from 101 on), class 1 at rank 99 where there
    is one (else at the last), and both classes carry equal scores around the cut"""
    g = [0, 0, 10, 10]
    far = lambda i: [1000 + 20 * (i % 40), 1000, 1010 + 20 * (i % 40), 1010]  # noqa: E731
    score = lambda i: F32(1.0) - F32(i // 2) / 256        # pairs of equal scores: 98 and 99 tie, 100 and 101 tie  # noqa: E731
    dets = [(g if i == nd - 1 else far(i), score(i), 0) for i in range(nd)]
    tp1 = min(nd, 100) - 1
    dets += [(g if i == tp1 else far(i), score(i), 1) for i in range(nd)]
    pred, gt = split({"i": image(dets, [(g, 0, 0, None), (g, 1, 0, None)])})
    r = ref.evaluate(pred, gt, 2)
    assert int(r["scored"]["i"].sum()) == 2 * min(nd, 100)
    assert r["recall"][0, 0, 0, 2] == (1.0 if nd <= 100 else 0.0) and r["recall"][0, 1, 0, 2] == 1.0
    assert_device_equals_oracle(pred, gt, 2, r, arrays_from_box_eval=False)


# ------------------------------------------------------------------------------------------------------------------------------------
# accumulate kernel sizes: 1024-position chunks walked from the right, 256-position waves, 4 positions per thread
ACC_N = [1, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
SIDES = (20, 40, 100)          # small, medium and large boxes; a detection k / 20 as wide as its box has IoU k / 20


def _acc_split(n, pattern):
    """n detections of one class in score order = image order (scores fall in steps of two positions: ties keep the image order),
    1 - 3 per image.  The position p's box side cycles over SIDES, so the area ranges see different subsets (also of every third position); a true positive at p has
    IoU (10 + p % 10) / 20, so every threshold sees a different subset too.  npig of "all": 20 (a), 7 (b), 10 (c, e), a multiple of 20 (d):
    recalls of 7/10, 7/20, 14/20 and 19/20 - one recall point short of the exact rational - fall wherever the pattern puts them."""
    if pattern == "a":
        tps, npig = {n - 1}, 20
    elif pattern == "b":
        tps, npig = {0}, 7
    elif pattern == "c":
        tps, npig = {p for p in (0, n - 1025, n - 1024, n - 257, n - 256, n - 5, n - 4) if 0 <= p < n}, 10
    elif pattern == "d":
        tps = set(range(0, n, 3))
        npig = 20 * ((len(tps) + 19) // 20)
    else:
        tps, npig = set(), 10
    ims, p, i = {}, 0, 0
    while p < n:
        dets, gts = [], []
        for j in range(min(1 + i % 3, n - p)):
            s = SIDES[(p + p // 3) % 3]
            x = 200 * j
            score = F32(1.0) - F32(p // 2) / 4096
            if pattern == "e":            # inside a crowd box of its own: matched and ignored everywhere
                gts.append(([x, 0, x + s, s], 0, 1, None))
                dets.append(([x + 2, 2, x + s // 2, s // 2], score, 0))
            elif p in tps:
                gts.append(([x, 0, x + s, s], 0, 0, None))
                dets.append(([x, 0, x + (s // 20) * (10 + p % 10), s], score, 0))
            else:
                dets.append(([x, 0, x + s, s], score, 0))
            p += 1
        ims[i] = image(dets, gts)
        i += 1
    # ground truth nobody finds, up to npig, cycling over the sizes
    extra = [([150 * (e % 20), 0, 150 * (e % 20) + SIDES[e % 3], SIDES[e % 3]], 0, 0, None) for e in range(npig - len(tps))]
    for e in range(0, len(extra), 20):
        ims["extra%d" % e] = image([], extra[e:e + 20])
    return split(ims), len(tps), npig


@pytest.mark.parametrize("pattern", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("n", ACC_N)
def test_accumulate_chunk_wave_and_thread_edges(n, pattern):
    (pred, gt), ntp, npig = _acc_split(n, pattern)
    r = ref.evaluate(pred, gt, 1)
    # the case is what it says: npig of "all", and at IoU 0.50 every planned true positive is one
    assert r["recall"][0, 0, 0, 2] == ntp / npig
    if pattern in "abcd":
        assert len({r["recall"][t, 0, 0, 2] for t in range(10)}) > 1        # the thresholds differ
    from ubteacher.evaluation.coco_eval_device import device_box_eval
    p, q, _ = device_box_eval(pred, gt, 1)
    assert np.array_equal(q, r["recall"]), ("recall [t, k, a, m]", np.argwhere(q != r["recall"])[:8])
    assert np.array_equal(p, r["precision"]), ("precision [t, r, k, a]", np.argwhere(p != r["precision"])[:8])


# ------------------------------------------------------------------------------------------------------------------------------------
# the key, offset and rank kernels alone
def _seg_offsets(keys, nseg):
    from ubteacher import hip
    n = len(keys)
    k = _dev(np.asarray(keys, np.int64)) if n else None
    off = torch.full((nseg + 1,), -7, dtype=torch.int64, device="cuda")
    hip.call("utv2_coco_seg_offsets", hip._p(k), n, nseg, hip._p(off), hip._stream())
    return off.cpu().numpy()


def _seg_want(keys, nseg):
    ids = np.minimum(np.asarray(keys, np.int64) >> 32, nseg)
    return np.searchsorted(ids, np.arange(nseg + 1), "left")


def _keys_of(ids, rng):
    """sorted segment ids -> keys with random low halves (the offsets must not depend on them)"""
    ids = np.sort(np.asarray(ids, np.int64))
    return (ids << 32) | rng.integers(0, 2 ** 32, len(ids), dtype=np.int64)


SEG_CASES = {
    "empty": lambda rng: (np.zeros(0, np.int64), 5),
    "one_segment_holds_all": lambda rng: (np.full(700, 3), 6),
    "first_and_last_empty": lambda rng: (rng.integers(1, 9, 900), 10),
    "run_of_1000_empty": lambda rng: (np.concatenate([rng.integers(0, 4, 300), rng.integers(1004, 1010, 300)]), 1010),
    "ids_above_nseg": lambda rng: (np.concatenate([rng.integers(0, 8, 500), rng.integers(8, 40, 200)]), 8),
    "single_key": lambda rng: (np.array([2]), 4),
    "grid_stride": lambda rng: (np.concatenate([rng.integers(0, 3000, GRID_STRIDE_N - 5), rng.integers(4000, 5003, 5)]), 5000),
}


@pytest.mark.parametrize("name", list(SEG_CASES))
def test_seg_offsets_alone(name):
    rng = np.random.default_rng(7)
    ids, nseg = SEG_CASES[name](rng)
    keys = _keys_of(ids, rng)
    got, want = _seg_offsets(keys, nseg), _seg_want(keys, nseg)
    assert want[0] == 0 and want[-1] <= len(keys)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def _rank_keys(key1, pair_off, K, max_dets):
    from ubteacher import hip
    D = len(key1)
    k1, po = _dev(key1), _dev(pair_off)
    key2 = torch.full((D,), -7, dtype=torch.int64, device="cuda")
    rank = torch.full((D,), 77, dtype=torch.uint8, device="cuda")
    hip.call("utv2_coco_rank_keys", hip._p(k1), hip._p(po), D, K, max_dets, hip._p(key2), hip._p(rank), hip._stream())
    return key2.cpu().numpy(), rank.cpu().numpy()


def _rank_want(key1, pair_off, K, max_dets):
    """numpy restatement: a detection of class < K and pair rank < max_dets keeps class << 32 | score bits and its rank; every other
    one goes to class K with rank 255"""
    pid = key1 >> 32
    c = pid % (K + 1)
    r = np.arange(len(key1)) - pair_off[pid]
    keep = (c < K) & (r < max_dets)
    return np.where(keep, (c << 32) | (key1 & 0xFFFFFFFF), np.int64(K) << 32), np.where(keep, r, 255).astype(np.uint8)


def _pairs_to_key1(counts, rng):
    """detections per pair id -> (sorted key1 with random score bits, pair offsets)"""
    counts = np.asarray(counts, np.int64)
    pid = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    key1 = (pid << 32) | rng.integers(0, 2 ** 32, len(pid), dtype=np.int64)
    return key1, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("max_dets", [1, 100])
@pytest.mark.parametrize("big", [False, True], ids=["small", "grid_stride"])
def test_rank_keys_alone(max_dets, big):
    rng = np.random.default_rng(11)
    K = 3
    if big:
        counts = rng.integers(0, 7, 300000)
        counts[1234 * 4 + 1] = 300
        counts[-2] += GRID_STRIDE_N - counts.sum()
        assert counts[-2] >= 0
    else:
        counts = np.array([2, 0, 300, 5,   0, 120, 1, 101,   100, 99, 0, 7])       # 3 images x (3 classes + the class of the rest)
    key1, pair_off = _pairs_to_key1(counts, rng)
    assert not big or len(key1) == GRID_STRIDE_N
    got2, gotr = _rank_keys(key1, pair_off, K, max_dets)
    want2, wantr = _rank_want(key1, pair_off, K, max_dets)
    if not big:      # the pair of 300: ranks 0 .. max_dets - 1 kept, the rest 255 and class K; the class-K pairs dropped whole
        seg = slice(int(pair_off[2]), int(pair_off[3]))
        assert list(wantr[seg]) == list(range(max_dets)) + [255] * (300 - max_dets)
        assert np.all(want2[seg][max_dets:] == K << 32) and np.all(wantr[int(pair_off[3]):int(pair_off[4])] == 255)
    assert np.array_equal(gotr, wantr), np.nonzero(gotr != wantr)[0][:8]
    assert np.array_equal(got2, want2), np.nonzero(got2 != want2)[0][:8]


def test_pair_keys_and_stable_sort_give_the_descending_score_order():
    """the score-order case's list and 1000 random float32 bit patterns without NaN: inside every (image, class) pair the stable sort of
    the keys is np.argsort(-scores, kind="mergesort") - descending, -0 and +0 tied, equal scores in input order"""
    from ubteacher import hip
    rng = np.random.default_rng(5)
    bits_ = rng.integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)
    rand = bits_.view(F32)
    rand = rand[~np.isnan(rand)]
    scores = np.concatenate([np.asarray(SCORE_LIST, F32), rand, np.asarray(SCORE_LIST, F32), rand[:50], rand[:50]]).astype(F32)
    D, K, N = len(scores), 2, 3
    cls = rng.integers(-1, K + 2, D).astype(np.int32)
    cls[:len(SCORE_LIST)] = 0
    off = np.array([0, len(SCORE_LIST) + 400, len(SCORE_LIST) + 400, D], np.int64)      # the second image is empty
    keys = torch.full((D,), -7, dtype=torch.int64, device="cuda")
    d_scores, d_cls, d_off = _dev(scores), _dev(cls), _dev(off)
    hip.call("utv2_coco_pair_keys", hip._p(d_scores), hip._p(d_cls), hip._p(d_off), N, K, hip._p(keys), hip._stream())
    skeys, perm = torch.sort(keys, stable=True)
    skeys, perm = skeys.cpu().numpy(), perm.cpu().numpy()
    img = np.searchsorted(off, np.arange(D), "right") - 1
    pid = img * (K + 1) + np.where((cls >= 0) & (cls < K), cls, K)
    assert np.array_equal(skeys >> 32, pid[perm])
    for p in np.unique(pid):
        members = np.nonzero(pid == p)[0]
        want = members[np.argsort(-scores[members].astype(np.float64), kind="mergesort")]
        got = perm[pid[perm] == p]
        assert np.array_equal(got, want), (int(p), np.nonzero(got != want)[0][:8])
    first = perm[pid[perm] == 0][:len(SCORE_LIST)]
    assert scores[first[0]] == np.inf


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals: an error code and no launch (the outputs keep their fill)
def test_entry_points_refuse_bad_arguments():
    from ubteacher import hip
    lib, st = hip.load(), hip._stream()
    i64 = lambda n, v=-7: torch.full((n,), v, dtype=torch.int64, device="cuda")  # noqa: E731
    u8 = lambda n: torch.full((n,), 77, dtype=torch.uint8, device="cuda")  # noqa: E731
    D, K, N = 8, 2, 2
    key1, poff, key2, rank = i64(D, 0), i64(N * (K + 1) + 1, 0), i64(D), u8(D)
    p_ = lambda t: t.data_ptr()  # noqa: E731
    for md in (0, 255, -1):
        assert lib.utv2_coco_rank_keys(p_(key1), p_(poff), D, K, md, p_(key2), p_(rank), st) != 0, md
    assert lib.utv2_coco_rank_keys(None, p_(poff), D, K, 100, p_(key2), p_(rank), st) != 0
    assert lib.utv2_coco_rank_keys(p_(key1), p_(poff), D, K, 100, None, p_(rank), st) != 0
    assert lib.utv2_coco_rank_keys(p_(key1), p_(poff), D, K, 100, p_(key2), None, st) != 0
    dbox = torch.zeros((D, 4), device="cuda")
    gbox = torch.zeros((D, 4), dtype=torch.float64, device="cuda")
    gcrowd, perm = torch.zeros(D, dtype=torch.uint8, device="cuda"), i64(D, 0)
    ws = u8(int(lib.utv2_coco_eval_workspace_bytes(D, K)))
    thr = (ctypes.c_double * 10)(*ref.IOU_THRS)
    rng = (ctypes.c_double * 8)(*[v for a in ref.AREA_RNG for v in a])
    rec = (ctypes.c_double * 101)(*ref.REC_THRS)
    cp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def match(dbox_=dbox, dperm=perm, N_=N, K_=K, D_=D, max_dets=100, max_gt=4, gbox_=gbox):
        return lib.utv2_coco_match(p_(dbox_) if dbox_ is not None else None, p_(dperm) if dperm is not None else None, p_(poff), p_(gbox_) if gbox_ is not None else None,
                                   p_(gcrowd), None, p_(perm), p_(poff), N_, K_, D_, max_dets, max_gt, cp(thr), cp(rng), p_(ws), st)

    assert match(max_dets=0) != 0
    assert match(max_gt=12801) != 0                    # 401 words of taken bits: more LDS than a workgroup has
    assert match(N_=1 << 20, K_=2047) != 0             # N (K + 1) = 2^31
    assert match(dbox_=None) != 0 and match(dperm=None) != 0 and match(gbox_=None) != 0
    assert lib.utv2_coco_pair_keys(None, p_(perm), p_(poff), 1 << 20, 2047, p_(key2), st) != 0
    assert lib.utv2_coco_pair_keys(None, None, p_(poff), N, K, p_(key2), st) != 0
    assert lib.utv2_coco_seg_offsets(None, D, K, p_(key2), st) != 0
    assert lib.utv2_coco_seg_offsets(p_(key1), D, K, None, st) != 0
    prec = torch.full((10, 101, K, 4), -7.0, dtype=torch.float64, device="cuda")
    recl = torch.full((10, K, 4, 3), -7.0, dtype=torch.float64, device="cuda")
    assert lib.utv2_coco_accumulate(None, p_(poff), p_(rank), K, D, cp(rec), p_(ws), p_(prec), p_(recl), st) != 0
    assert lib.utv2_coco_accumulate(p_(perm), p_(poff), None, K, D, cp(rec), p_(ws), p_(prec), p_(recl), st) != 0
    torch.cuda.synchronize()
    assert torch.all(key2 == -7) and torch.all(rank == 77) and torch.all(ws == 77) and torch.all(prec == -7.0) and torch.all(recl == -7.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# DeviceCOCOBoxEvaluator
def _same(a, b):
    return a == b or (a != a and b != b)


def test_evaluator_image_processed_twice():
    from ubteacher.evaluation import COCOBoxEvaluator, DeviceCOCOBoxEvaluator
    host, dev = COCOBoxEvaluator(1), DeviceCOCOBoxEvaluator(1)
    for inp, out in twice_inputs("cuda"):
        host.process([inp], [out])
        dev.process([inp], [out])
    rh, rd = host.evaluate()["bbox"], dev.evaluate()["bbox"]
    assert rd["AP"] == 100.0 and rd["AP50"] == 100.0 and rd["APm"] == -1.0 and rd["AR1"] == 100.0       # first position, last value
    for k, v in rh.items():
        assert _same(rd[k], v), (k, rd[k], v)


def test_evaluator_area_field_on_some_images_only():
    """a registered set whose annotations carry `area` on some images, on none of others and on part of one (both evaluators then rank
    that image by the box areas): the device result equals the host evaluator's key for key, and the oracle's six numbers"""
    from ubteacher.d2.structures import Boxes, Instances
    from ubteacher.data import DatasetCatalog, MetadataCatalog
    from ubteacher.evaluation import COCOBoxEvaluator, DeviceCOCOBoxEvaluator
    pred, gt = ref.structured_split(201, n_images=12, num_classes=3)
    K, name = 3, "coco_edges_area_on_some"
    dicts, partial = [], None
    for iid, g in gt.items():
        annos = []
        for j in range(len(g["classes"])):
            a = dict(bbox=[float(v) for v in g["boxes"][j]], bbox_mode="XYXY_ABS", category_id=int(g["classes"][j]), iscrowd=int(g["iscrowd"][j]))
            if "area" in g:
                a["area"] = float(g["area"][j])
            annos.append(a)
        if partial is None and "area" in g and len(annos) >= 2:
            partial = iid
            del annos[0]["area"]
            g.pop("area")                      # the oracle's view of that image: box areas
        dicts.append(dict(image_id=iid, height=800, width=800, annotations=annos))
    assert partial is not None and any("area" in g for g in gt.values()) and any("area" not in g for g in gt.values())
    if name in DatasetCatalog:
        DatasetCatalog.remove(name)
    DatasetCatalog.register(name, lambda: dicts)
    MetadataCatalog.get(name).set(thing_classes=["a", "b", "c"])
    try:
        host, dev = COCOBoxEvaluator(K, dataset_name=name), DeviceCOCOBoxEvaluator(K, dataset_name=name)
        for d in dicts:
            p = pred.get(d["image_id"])
            if p is None:
                continue
            inst = Instances((800, 800))
            inst.pred_boxes = Boxes(torch.from_numpy(p["boxes"]).reshape(-1, 4).cuda())
            inst.scores = torch.from_numpy(p["scores"]).cuda()
            inst.pred_classes = torch.from_numpy(p["classes"]).cuda()
            inp = {"image_id": d["image_id"], "height": 800, "width": 800}
            host.process([inp], [{"instances": inst}])
            dev.process([inp], [{"instances": inst}])
        rh, rd = host.evaluate()["bbox"], dev.evaluate()["bbox"]
    finally:
        DatasetCatalog.remove(name)
    for k, v in rh.items():
        assert _same(rd[k], v), (k, rd[k], v)
    # both evaluators score the processed images only, in process order
    seen = [d["image_id"] for d in dicts if d["image_id"] in pred]
    r = ref.evaluate({i: pred[i] for i in seen}, {i: gt[i] for i in seen}, K)
    for k in ref.SIX:
        assert rd[k] == r["stats"][k], (k, rd[k], r["stats"][k])
    for k in ("AR1", "AR10", "AR100", "ARs", "ARm", "ARl"):
        assert rd[k] == r["stats"][k], (k, rd[k], r["stats"][k])
