"""The BatchNorm (csrc/batchnorm.hip) and per-ROI GroupNorm (csrc/groupnorm_roi.hip) kernels give the bits they gave at the commit that
tests/golden/norm_kernels_parent.json names: for every case, library kind and output tensor the fixture holds the SHA-256 of the tensor's
bytes (results only, written by tests/golden/gen_golden_norm_parent.py, which imports the cases and inputs from this module).

Inputs come from an integer formula, ((i * 2654435761 + k) mod 2^32) mapped to multiples of 1/16 in [-2, 2), so that no random-number
generator's version enters a digest; channel 1 is off-centre (+ 300), channel 2 is constant.  16-bit kinds take the values as the
type stores them (round to nearest even).

BN cases (C, sets per level) over three levels, set sizes 2, 63, 64, 65 and 513 rows (513 rows = nine chunks: one stage-2 slice takes
two); C = 260 gives a second column block with a single live quad.  Each case runs training, eval mode, and count_mul = 2 with
biased_running on the case's own moments and sums; every intermediate is hashed.
ROI-GN cases (R, HW, C, G), ReLU on and off: 52 / 53 rows of 256 channels are the last resident and the first re-reading ROI size;
C = 96 leaves idle threads; R = 1025 strides past the 1024 workgroups; in the 5-ROI case ROI 1 is all zero."""
import functools
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_kernels_parent.json")
KINDS = ("fp32", "bf16", "fp16")
EPS, MOMENTUM = 1e-5, 0.1
L = 3
BN_SETS = {1: (65, 2, 513), 2: (2, 63, 64, 65, 513, 2)}        # rows of the sets, level-first; two per level: (level 0: 2, 63) ...
BN_CASES = [(8, 1), (8, 2), (260, 1), (260, 2)]
ROI_CASES = [(3, 52, 256, 32), (3, 53, 256, 32), (3, 5, 96, 8), (1025, 1, 16, 4), (5, 49, 256, 32)]


def bn_id(case):
    return "bn_C%d_sets%d" % case


def roi_id(case, relu):
    return "roi_R%d_HW%d_C%d_G%d_relu%d" % (case + (int(relu),))


def dyadic(n, k):
    """n values in [-2, 2), multiples of 1/16: bits 16.. of (i * 2654435761 + k) mod 2^32 (exact in int64)"""
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + k) % (1 << 32)
    return (((h >> 16) % 64) - 32).float() / 16


def activation(rows, C, k):
    x = dyadic(rows * C, k).reshape(rows, C)
    x[:, 1] += 300.0
    x[:, 2] = 1.5
    return x


def select(kind):
    from ubteacher import hip, ops
    ops.set_precision(kind)
    return torch.float32 if kind == "fp32" else hip.h16_dtype()


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def bn_sets(nper):
    sets, r = [], 0
    for i, n in enumerate(BN_SETS[nper]):
        sets.append((r, n, i // nper))
        r += n
    return sets, r


def bn_digests(case, kind):
    """every intermediate and output of one BN case through the wrappers (the backward's stage-1 sums through the raw entry: the
    wrapper does not hand them out) -> {tensor name: sha256}"""
    from ubteacher import hip
    C, nper = case
    dt = select(kind)
    sets, P = bn_sets(nper)
    st = hip.BnSets(sets, L)
    x, dy = activation(P, C, 1).to(dt).cuda(), activation(P, C, 7).to(dt).cuda()
    ga = (0.5 + (dyadic(L * C, 11).reshape(L, C) + 2) / 4).cuda()
    be = (dyadic(L * C, 13).reshape(L, C) / 8).cuda()
    rm0, rv0 = (dyadic(L * C, 17).reshape(L, C) / 4).cuda(), (1.0 + (dyadic(L * C, 19).reshape(L, C) + 2) / 8).cuda()
    out = {}

    def backward(tag, y, mean, rstd, count_mul, sums=None):
        if sums is None:
            partial = torch.empty((st.nchunks, 2, C), dtype=torch.float64, device="cuda")
            hip.call("utv2_bn_bwd_partial", dy.data_ptr(), y.data_ptr(), x.data_ptr(), hip._dt(x), mean.data_ptr(), rstd.data_ptr(),
                     partial.data_ptr(), P, C, st.n, st.p_row0, st.p_rows, hip._stream())
            sums = hip.bn_reduce(partial, st, divide=False)
            assert torch.equal(sums, hip.bn_bwd_sums(dy, y, x, mean, rstd, st))
            out.update({tag + "partial_bwd": partial, tag + "sums": sums})
        dga, dbe = torch.zeros_like(ga), torch.zeros_like(be)
        dx = hip.bn_bwd_apply(dy, y, x, mean, rstd, ga, sums, dga, dbe, st, count_mul=count_mul)
        out.update({tag + "dx": dx, tag + "dgamma": dga, tag + "dbeta": dbe})
        return sums

    # training
    partial = hip.bn_stats(x, st, partial_only=True)
    moments = hip.bn_reduce(partial, st, divide=True)
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd, scale = hip.bn_finalize(moments, ga, rm, rv, st, EPS, MOMENTUM)
    y = hip.bn_apply_relu(x, mean, scale, be, st)
    out.update(partial_fwd=partial, moments=moments, mean=mean, rstd=rstd, scale=scale, running_mean=rm, running_var=rv, y=y)
    sums = backward("", y, mean, rstd, 1)
    # eval mode
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd, scale = hip.bn_finalize(None, ga, rm, rv, st, EPS, MOMENTUM, training=False)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    out.update(eval_mean=mean, eval_rstd=rstd, eval_scale=scale, eval_y=hip.bn_apply_relu(x, mean, scale, be, st))
    # count_mul = 2 with the biased running variance, on the case's own moments and sums (no second rank)
    rm, rv = rm0.clone(), rv0.clone()
    mean, rstd, scale = hip.bn_finalize(moments, ga, rm, rv, st, EPS, MOMENTUM, count_mul=2, biased_running=True)
    y = hip.bn_apply_relu(x, mean, scale, be, st)
    out.update(sync_mean=mean, sync_rstd=rstd, sync_scale=scale, sync_running_mean=rm, sync_running_var=rv, sync_y=y)
    backward("sync_", y, mean, rstd, 2, sums=sums)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in out.items()}


def roi_digests(case, relu, kind):
    from ubteacher import hip
    R, HW, C, G = case
    dt = select(kind)
    x, dy = activation(R * HW, C, 3).reshape(R, HW, C), dyadic(R * HW * C, 5).reshape(R, HW, C)
    if R == 5:
        x[1] = 0.0
    x, dy = x.to(dt).cuda(), dy.to(dt).cuda()
    ga, be = (0.5 + (dyadic(C, 11) + 2) / 4).cuda(), (dyadic(C, 13) / 8).cuda()
    y, mean, rstd = hip.groupnorm_roi_fwd(x, ga, be, G, EPS, relu)
    dga, dbe = torch.zeros_like(ga), torch.zeros_like(be)
    dx = hip.groupnorm_roi_bwd(dy, x, mean, rstd, ga, be, dga, dbe, G, relu)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dga, dbeta=dbe).items()}


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


def check(cid, kind, got):
    want = fixture()[cid][kind]
    assert sorted(got) == sorted(want), (cid, kind)
    differ = sorted(k for k in got if got[k] != want[k])
    assert not differ, "%s %s: other bytes than the fixture's commit in %s" % (cid, kind, differ)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BN_CASES, ids=bn_id)
def test_batchnorm_bits_are_the_fixture_commits(case, kind):
    check(bn_id(case), kind, bn_digests(case, kind))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ROI_CASES, ids=lambda c: "R%d_HW%d_C%d" % c[:3])
def test_roi_groupnorm_bits_are_the_fixture_commits(case, kind, relu):
    check(roi_id(case, relu), kind, roi_digests(case, relu, kind))
