"""The gather kernels at the end of the inference chains - utv2_nms_pack (RPN), utv2_roi_infer_gather and utv2_roi_infer_pack (ROI
predictor) - against plain torch indexing (tests/loss_tail_ref64.py), bit for bit.  The sortable keys come from hip.roi_infer_keys and are
ordered with torch.sort, so no packing constant is named here: the reference order is the stable descending sort of the candidate
scores (probability descending, flat (proposal, class) index ascending), the tie rule the keys encode."""
import pytest
import torch

from tests import loss_tail_ref64 as T64
from tests.test_loss_kernels_fp64_gpu import dev, same_bits

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHAPES = [(3, 85), (4, 64), (1, 257)]      # N x slots = 255, 256, 257: below, at and above one 256-thread block


def hip():
    from ubteacher import hip as H
    return H


def survivors(N, D, limit, seed, cnts):
    """kidx [N, D]: cnt[n] distinct indices below `limit`, then -1; cnt from {0, 1, D}"""
    g = torch.Generator().manual_seed(seed)
    kidx = torch.full((N, D), -1, dtype=torch.int32)
    cnt = torch.tensor([cnts[n % len(cnts)] for n in range(N)], dtype=torch.int32)
    for n in range(N):
        c = int(cnt[n])
        kidx[n, :c] = torch.randperm(limit, generator=g)[:c].to(torch.int32)
    return kidx, cnt


def all_equal(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape, a.dtype, b.dtype)
        assert same_bits(a, b) if a.dtype == F32 else torch.equal(a.cpu(), b), i


@pytest.mark.parametrize("N,D", SHAPES)
def test_nms_pack_equals_indexing(N, D):
    M = D + 40
    g = torch.Generator().manual_seed(10 + N)
    boxes = torch.randn((N, M, 4), generator=g)
    scores = torch.randn((N, M), generator=g)
    scores[:, 0], scores[:, 1], scores[:, 2] = -0.0, 1e-40, float("nan")       # read back unchanged, bit for bit
    for cnts in ((0, 1, D), (D, 0, 1), (1, D, 0)):
        kidx, cnt = survivors(N, D, M, 20 + N, cnts)
        kidx[:, 0] = torch.where(cnt > 0, torch.tensor(1, dtype=torch.int32), kidx[:, 0])      # the denormal score is among the survivors
        got = hip().nms_pack(dev(kidx), dev(cnt), dev(boxes), dev(scores))
        want = T64.nms_pack(kidx, cnt, boxes, scores)
        all_equal(got, want)
        pad = kidx < 0
        ob, osc, ov = (t.cpu() for t in got)
        assert torch.all(ov[pad] == 0) and same_bits(ob[pad], boxes[:, 0][:, None].expand(N, D, 4)[pad])      # a padded slot reads row 0
        assert int(ov.sum()) == int(cnt.sum())


def roi_inputs(N, P, K, nbox, seed, special):
    g = torch.Generator().manual_seed(seed)
    probs = torch.rand((N * P, K + 1), generator=g)
    deltas = torch.randn((N * P, 4 * nbox), generator=g)
    xy = torch.rand((N, P, 2), generator=g) * 200
    prop = torch.cat((xy, xy + 8 + torch.rand((N, P, 2), generator=g) * 90), dim=2).contiguous()
    valid = torch.ones((N, P), dtype=torch.uint8)
    valid[:, 5] = 0                                    # an empty proposal slot: none of its classes is a candidate
    valid[N - 1, 10:] = 0                              # the last image has fewer candidates than any k: sentinel keys reach the gather
    r0 = (N - 1) * P
    probs[r0 + 7, 2] = float("nan")                    # a non-finite probability drops the whole row
    whwh = torch.tensor([[320.0, 240.0, 320.0, 240.0]]).repeat(N, 1)
    std = torch.randn((N * P, 4 * nbox), generator=g)
    if special:      # with thr = -0.25: -0.0 and a denormal are candidates (of the last image), thr itself is not
        probs[r0 + 3, 1], probs[r0 + 4, 0], probs[r0 + 9, 2] = -0.0, 1e-40, -0.25
    return probs, deltas, prop, valid, whwh, std


def candidates(probs, valid, N, P, K, thr):
    """the score of every (proposal, class) as the keys hold it: -1 where it is no candidate"""
    pr = probs.reshape(N, P, K + 1)[:, :, :K]
    ok = (valid.bool() & torch.isfinite(pr).all(dim=2))[:, :, None] & (pr > thr)
    return torch.where(ok, pr, torch.tensor(-1.0)).reshape(N, P * K)


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("nbox_is_K", [False, True])
@pytest.mark.parametrize("N,k", SHAPES)
def test_roi_infer_gather_and_pack_equal_indexing(N, k, nbox_is_K, special):
    H = hip()
    P, K = 60, 5
    nbox = K if nbox_is_K else 1
    thr = -0.25 if special else 0.3
    probs, deltas, prop, valid, whwh, std = roi_inputs(N, P, K, nbox, 30 + N + nbox, special)
    boxes, keys = H.roi_infer_keys(dev(probs), dev(deltas), dev(prop), dev(valid), dev(whwh), K, 10.0, 5.0, 4.135, thr, nbox=nbox)
    top = torch.sort(keys, dim=1, descending=True)[0][:, :k].contiguous()
    cand = candidates(probs, valid, N, P, K, thr)
    score, flat = torch.sort(cand, dim=1, descending=True, stable=True)      # ties: the lower flat index first
    score, flat = score[:, :k].contiguous(), flat[:, :k].contiguous()
    assert int((score > thr).sum()) > 0 and int((score == -1).sum()) > 0      # candidates and sentinel keys (score -1) both reach the gather
    # the gather's own comparison is strict: hand it a threshold that EQUALS a selected score
    for thr_g in (thr, float(score[0, 1])):
        got = H.roi_infer_gather(top, boxes, K, thr_g)
        want = T64.roi_infer_gather(flat, score, boxes.cpu(), K, thr_g)
        all_equal(got, want)
        assert int(got[4].cpu()[0, 1]) == (1 if thr_g == thr else 0)
    if special:
        sc = got[0].cpu()
        for v in (-0.0, 1e-40):                                               # survive the key round trip unchanged
            t = torch.tensor([v], dtype=F32)
            assert any(same_bits(x.reshape(1), t) for x in sc[N - 1]), v
        assert not bool((sc == -0.25).any())                                  # a probability equal to thr is no candidate
    sc_d, rows_d, cls_d, cb_d, _ = H.roi_infer_gather(top, boxes, K, thr)
    D = k
    for cnts in ((0, 1, D), (D, 0, 1), (1, D, 0)):
        kidx, cnt = survivors(N, D, k, 40 + N, cnts)
        got = H.roi_infer_pack(dev(kidx), dev(cnt), cb_d, sc_d, cls_d, rows_d, dev(std), P, D, nbox=nbox)
        want = T64.roi_infer_pack(kidx, cnt, cb_d.cpu(), sc_d.cpu(), cls_d.cpu(), rows_d.cpu(), std, P, D, nbox)
        all_equal(got, want)
        ov = got[5].cpu()
        assert torch.all(ov[kidx < 0] == 0) and int(ov.sum()) == int(cnt.sum())
        pad = kidx < 0
        assert same_bits(got[0].cpu()[pad], cb_d.cpu()[:, 0][:, None].expand(N, D, 4)[pad])      # a padded slot reads candidate 0
