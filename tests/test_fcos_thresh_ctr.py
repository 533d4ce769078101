"""MODEL.FCOS.THRESH_WITH_CTR (reference fcos_outputs.py:148,1172-1195,1270-1275) without a device: the configuration is accepted, the
default keeps the flag off, the argument checks of the three entry points, and a plain torch restatement of
forward_for_single_feature_map (:1093-1108,1146-1296) held to the golden executed from the reference (tests/golden/thresh_ctr.npz,
gen_golden_thresh_ctr.py) to the bit - the restatement is what the device tests use where the golden has no case (edge shapes,
flag off)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDES = [8, 16, 32, 64, 128]
CRITERIA = ("cls", "cls_n_ctr", "ctr", "cls_n_loc")
HEADS = ("d", "c")
C = 80


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def load_gold():
    return dict(np.load(os.path.join(GOLD, "thresh_ctr.npz"), allow_pickle=False))


def restate_level(logits, reg, std, ctr, stride, discrete, thr, topk, method, thresh_with_ctr):
    """forward_for_single_feature_map for one level.  logits [N, C, h, w], reg [N, 68 | 4, h, w] (continuous: BEFORE the ReLU), std
    [N, 4, h, w], ctr [N, 1, h, w] -> per image a dict: flat (location * C + class), rank (the ranking score), scores, conf, ctr, boxes,
    std - in the reference's order (candidates ascending, or whatever topk(sorted=False) returns).  The square root of the score
    transform (:1271) is taken in fp64 and rounded once to fp32, which is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits) on
    every CPU; torch.sqrt on fp32 is not (1 ulp off on 0.6 % to 20 % of inputs, depending on the machine), see the golden's `scores_cr`."""
    N, nc, h, w = logits.shape
    p = logits.permute(0, 2, 3, 1).reshape(N, -1, nc).sigmoid()
    c = ctr.permute(0, 2, 3, 1).reshape(N, -1).sigmoid()
    sd = std.permute(0, 2, 3, 1).reshape(N, -1, 4)
    r = reg.permute(0, 2, 3, 1).reshape(N, h * w, -1)
    if discrete:                                                     # Integral (:57-78): softmax over the bins, expectation
        r = F.linear(F.softmax(r.reshape(-1, 17), dim=1), torch.linspace(0, 16, 17)[None]).reshape(N, h * w, 4)
    else:
        r = F.relu(r)
    r = r * stride
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    loc = torch.stack([xs.reshape(-1) * stride + stride // 2, ys.reshape(-1) * stride + stride // 2], 1).float()
    if thresh_with_ctr:
        p = p * c[:, :, None]
    cand = p > thr
    n_top = cand.reshape(N, -1).sum(1).clamp(max=topk)
    conf = p
    if not thresh_with_ctr:
        if method == "cls_n_ctr":
            p = p * c[:, :, None]
        elif method == "ctr":
            p = c[:, :, None].expand_as(p)
        elif method == "cls_n_loc":
            p = p * (1 - sd.sigmoid()).mean(2)[:, :, None]
    out = []
    for i in range(N):
        flat = cand[i].reshape(-1).nonzero().squeeze(1)
        rank = p[i].reshape(-1)[flat]
        if len(flat) > int(n_top[i]):
            rank, ti = rank.topk(int(n_top[i]), sorted=False)
            flat = flat[ti]
        hw = flat // nc
        d, l = r[i][hw], loc[hw]
        boxes = torch.stack([l[:, 0] - d[:, 0], l[:, 1] - d[:, 1], l[:, 0] + d[:, 2], l[:, 1] + d[:, 3]], 1)
        scores = rank.double().sqrt().float() if method in ("cls_n_ctr", "cls_n_loc") else rank
        out.append(dict(flat=flat, rank=rank, scores=scores, conf=conf[i].reshape(-1)[flat], ctr=c[i][hw], boxes=boxes, std=sd[i][hw]))
    return out


def golden_level_inputs(gold, head, l):
    return (T(gold["logits%d" % l]), T(gold["reg_%s%d" % (head, l)]), T(gold["std%d" % l]), T(gold["ctr%d" % l]))


def test_build_model_accepts_the_key():
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    cfg = get_config("fcos", 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.THRESH_WITH_CTR", True])
    torch.manual_seed(0)
    model = build_model(cfg)
    assert model.proposal_generator.fcos_outputs.thresh_with_ctr is True
    from ubteacher.modeling.pseudo_generator import PseudoGenerator
    assert PseudoGenerator(cfg).fcos_output.thresh_with_ctr is True


def test_default_config_keeps_the_flag_off():
    from ubteacher.modeling.fcos import FCOSOutputs
    from ubteacher.presets import get_config
    cfg = get_config("fcos", 1, ["MODEL.DEVICE", "cpu"])
    assert cfg.MODEL.FCOS.THRESH_WITH_CTR is False
    assert FCOSOutputs(cfg).thresh_with_ctr is False


def test_flag_value_matches_the_header():
    from ubteacher import hip
    hdr = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "utv2.h")).read()
    assert "#define UTV2_FCOS_THRESH_WITH_CTR %d\n" % hip.FCOS_THRESH_WITH_CTR in hdr
    for name in ("utv2_fcos_rank_keys", "utv2_fcos_decode", "utv2_fcos_decode_cont"):     # both libraries export old and new surface
        assert name in hip.symbols() and name + "_f" in hip.symbols()
    hip.load("bf16"), hip.load("fp16")


def flag_argument_rows(ptr, method, flags):
    """(entry point, arguments) of the three entry points that take the flag, with every other argument valid; `ptr` is a non-null
    address that is never followed when the call is refused"""
    p, st = ctypes.c_void_p(ptr), ctypes.c_void_p(0)
    return [("utv2_fcos_rank_keys_f", (p, p, 80, 16, 1, 1, 4, 0.05, method, flags, p, 4, st)),
            ("utv2_fcos_decode_f", (p, 1, p, p, 80, 16, 1, 1, 1, 4, 8, 0, method, flags, 1, 0, p, p, p, p, p, p, p, p, p, st)),
            ("utv2_fcos_decode_cont_f", (p, 1, p, p, 16, 1, 1, 1, 4, 8, 0, method, flags, 1, 0, p, p, p, p, p, p, p, p, p, st))]


# (method, flags): an unknown flag bit with a valid criterion, and the criterion's range, which the flag must not widen
BAD_FLAGS = [(0, 2), (1, 3), (3, 4), (0, -1), (2, 1 << 30), (4, 0), (4, 1), (5, 1), (-1, 1), (7, 0)]


@pytest.mark.parametrize("method,flags", BAD_FLAGS)
def test_unknown_flag_bits_are_refused_without_a_device(method, flags):
    from ubteacher import hip as H
    for kind in ("bf16", "fp16"):
        lib = H.load(kind)
        buf = (ctypes.c_float * 16)()
        for name, args in flag_argument_rows(ctypes.addressof(buf), method, flags):
            assert getattr(lib, name)(*args) == -1000, (kind, name, method, flags)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("method", CRITERIA)
def test_restatement_reproduces_the_executed_reference(gold, head, method):
    """every (level, image), to the bit: the same candidates, cls_confid (the ranking score), centerness, std and scores, and the boxes
    of the continuous head (relu, one product, one sum: IEEE operations).  For cls_n_ctr / cls_n_loc the scores are held to the golden's
    `scores_cr`: the generator asserted that the reference's scores are torch.sqrt of the recorded cls_confid and lie within 1 ulp of
    the correctly rounded root stored there (torch.sqrt on fp32 differs by that ulp between CPUs: the one that wrote the golden was off
    on 8 of these scores) - the 1 ulp is checked again here on the data.
    Boxes of the discrete head are not reproducible to the bit between CPUs (measured: 3 ulp apart on two machines): Integral is a
    softmax over 17 bins and a 17-term dot product in the BLAS of the machine.  Bound: the distance is sum_j p_j * j <= 16 bins with
    sum_j p_j = 1; each p_j carries the exp, the 17-term normalising sum and the division, the dot product 17 more roundings - 24 units
    of 2^-24 relative to the largest possible distance, times the stride: |d box| <= 24 * 2^-24 * 16 * stride (1.8e-4 at stride 8)."""
    N, thr, topk = int(gold["N"]), float(gold["thr"]), int(gold["topk"])
    cut = 0
    for l, s in enumerate(STRIDES):
        got = restate_level(*golden_level_inputs(gold, head, l), s, head == "d", thr, topk, method, True)
        for i in range(N):
            p = "%s_%s_L%d_I%d_" % (head, method, l, i)
            a, b = torch.argsort(got[i]["flat"]), np.argsort(gold[p + "flat"])
            assert np.array_equal(got[i]["flat"][a].numpy(), gold[p + "flat"][b]), p
            for k, gk in (("conf", "conf"), ("ctr", "ctr"), ("std", "std"), ("scores", "scores_cr")):
                assert np.array_equal(got[i][k][a].numpy(), gold[p + gk][b]), p + k
            if head == "c":
                assert np.array_equal(got[i]["boxes"][a].numpy(), gold[p + "boxes"][b]), p
            else:
                np.testing.assert_allclose(got[i]["boxes"][a].numpy(), gold[p + "boxes"][b], rtol=0, atol=24 * 2.0 ** -24 * 16 * s, err_msg=p)
            assert torch.equal(got[i]["rank"], got[i]["conf"])                             # cls_confid IS the ranking score (:1179)
            ref, cr = gold[p + "scores"], gold[p + "scores_cr"]                            # the reference's own scores: 1 ulp at most
            assert int(np.abs(ref.view(np.int32).astype(np.int64) - cr.view(np.int32).astype(np.int64)).max(initial=0)) <= 1, p
            if method in ("cls", "ctr"):
                assert np.array_equal(ref, cr) and np.array_equal(ref, gold[p + "conf"]), p
            cut += len(a) == topk
    assert cut >= 1


def test_golden_can_show_a_failure(gold):
    """the conditions the generator asserted, seen from the restatement: without the flag other candidates are kept on some row, and for
    cls_n_loc / ctr the kept set is not the one the criterion's own score keeps"""
    N, thr, topk = int(gold["N"]), float(gold["thr"]), int(gold["topk"])
    for method in CRITERIA:
        differs = 0
        for l, s in enumerate(STRIDES):
            off = restate_level(*golden_level_inputs(gold, "d", l), s, True, thr, topk, method, False)
            for i in range(N):
                differs += set(off[i]["flat"].tolist()) != set(gold["d_%s_L%d_I%d_flat" % (method, l, i)].tolist())
        assert differs >= 1, method
