"""ResNet-18 / 34 (Detectron2 BasicBlock stages, MODEL.RESNETS.DEPTH 18 / 34 with RES2_OUT_CHANNELS 64): the config surface, the state-dict
keys, what stays refused, checkpoint loading and the frozen stages.  CPU only: models are built on the CPU and only their state dicts,
arena layout and layer geometry are inspected.  The exact-arithmetic operands of the fused kernel's GPU test are checked here too."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))

BLOCKS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def _opts(depth, *more):
    return ["MODEL.RESNETS.DEPTH", depth, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64] + list(more)


def _cfg(family, opts):
    from ubteacher.presets import get_config
    return get_config(family, 1, ["MODEL.DEVICE", "cpu"] + list(opts))


def _model(family, opts):
    from ubteacher.modeling import build_model
    torch.manual_seed(0)
    return build_model(_cfg(family, opts))


def _d2_keys(depth):
    """{state-dict key: shape} of Detectron2's build_resnet_backbone for DEPTH 18 / 34 (BasicBlock, FrozenBN) under backbone.bottom_up."""
    out = {}

    def conv(prefix, cout, cin, k):
        out[prefix + ".weight"] = (cout, cin, k, k)
        for t in ("weight", "bias", "running_mean", "running_var"):
            out[prefix + ".norm." + t] = (cout,)

    p = "backbone.bottom_up."
    conv(p + "stem.conv1", 64, 3, 7)
    cin = 64
    for si, n in enumerate(BLOCKS[depth]):
        cout = 64 * 2 ** si
        for b in range(n):
            q = "%sres%d.%d." % (p, si + 2, b)
            if cin != cout:
                conv(q + "shortcut", cout, cin, 1)
            conv(q + "conv1", cout, cin, 3)
            conv(q + "conv2", cout, cout, 3)
            cin = cout
    return out


@pytest.mark.parametrize("depth", [18, 34])
@pytest.mark.parametrize("family", ["fcos", "rcnn"])
def test_builds_with_d2_keys_and_widths(family, depth):
    from ubteacher.modeling.backbone import BasicBlock
    m = _model(family, _opts(depth))
    bu = m.backbone.bottom_up
    assert tuple(len(b) for _, b, _ in bu.stages) == BLOCKS[depth]
    assert all(isinstance(b, BasicBlock) for _, blocks, _ in bu.stages for b in blocks)
    assert bu.channels == {"res2": 64, "res3": 128, "res4": 256, "res5": 512}
    sd = m.state_dict()
    got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("backbone.bottom_up.")}
    assert got == _d2_keys(depth)
    assert not any(".conv3." in k for k in got)
    assert sorted({k.split(".")[2] + "." + k.split(".")[3] for k in got if ".shortcut." in k}) == ["res3.0", "res4.0", "res5.0"]
    laterals = [c for c in (64, 128, 256, 512)] if family == "rcnn" else [128, 256, 512]     # FCOS: IN_FEATURES res3 .. res5
    first = 6 - len(laterals)
    for i, c in enumerate(laterals):
        assert tuple(sd["backbone.fpn_lateral%d.weight" % (first + i)].shape) == (256, c, 1, 1)
    # geometry: conv1 carries the stride, every res2 block is an identity block
    for si, (name, blocks, _) in enumerate(bu.stages):
        for b, blk in enumerate(blocks):
            s = 2 if (b == 0 and si > 0) else 1
            assert (blk.conv1.k, blk.conv1.stride, blk.conv1.pad, blk.conv1.relu) == (3, s, 1, True)
            assert (blk.conv2.k, blk.conv2.stride, blk.conv2.pad, blk.conv2.relu) == (3, 1, 1, True)
            assert (blk.shortcut is not None) == (b == 0 and si > 0)
            if blk.shortcut is not None:
                assert (blk.shortcut.k, blk.shortcut.stride, blk.shortcut.relu) == (1, 2, False)


def test_state_dict_view_is_nchw_over_the_arena_matrix():
    m = _model("fcos", _opts(18))
    conv1 = m.backbone.bottom_up.stages[1][1][0].conv1          # res3.0.conv1: 3x3 stride 2, 64 -> 128
    assert tuple(conv1.w.t.shape) == (128, 9 * 64)
    w = torch.randn(128, 64, 3, 3)
    m.state_dict()["backbone.bottom_up.res3.0.conv1.weight"].copy_(w)
    assert torch.equal(conv1.w.t.view(128, 3, 3, 64).permute(0, 3, 1, 2), w)


@pytest.mark.parametrize("opts,key", [
    (["MODEL.RESNETS.DEPTH", 18], "MODEL.RESNETS.DEPTH"),                                   # RES2_OUT_CHANNELS still 256
    (["MODEL.RESNETS.DEPTH", 34], "MODEL.RESNETS.DEPTH"),
    (["MODEL.RESNETS.RES2_OUT_CHANNELS", 64], "MODEL.RESNETS.RES2_OUT_CHANNELS"),           # a bottleneck depth with 64
    (["MODEL.RESNETS.DEPTH", 101, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64], "MODEL.RESNETS.RES2_OUT_CHANNELS"),
    (["MODEL.RESNETS.DEPTH", 200], "MODEL.RESNETS.DEPTH"),
    (["MODEL.RESNETS.DEPTH", 200, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64], "MODEL.RESNETS.DEPTH"),
    (_opts(18, "MODEL.RESNETS.NUM_GROUPS", 32), "MODEL.RESNETS.NUM_GROUPS"),
    (_opts(34, "MODEL.RESNETS.WIDTH_PER_GROUP", 32), "MODEL.RESNETS.WIDTH_PER_GROUP"),
    (_opts(18, "MODEL.RESNETS.DEFORM_ON_PER_STAGE", [False, True, False, False]), "MODEL.RESNETS.DEFORM_ON_PER_STAGE"),
    (_opts(18, "MODEL.RESNETS.NORM", "BN"), "MODEL.RESNETS.NORM"),
])
@pytest.mark.parametrize("family", ["fcos", "rcnn"])
def test_refusals_name_their_key(family, opts, key):
    from ubteacher.modeling import build_model
    cfg = _cfg(family, opts)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")) as e:
        build_model(cfg)
    if opts[:2] in (["MODEL.RESNETS.DEPTH", 18], ["MODEL.RESNETS.DEPTH", 34]) and len(opts) == 2:
        assert "MODEL.RESNETS.RES2_OUT_CHANNELS 64" in str(e.value)         # the pairing Detectron2 asserts


def _to_c2_name(k):
    """inverse of Detectron2's Caffe2 blob-name conversion for a BasicBlock ResNet body (tests/test_backbone_variants.py::_to_c2_name
    without branch2c)"""
    k = k.replace("backbone.bottom_up.", "")
    if k.startswith("stem.conv1."):
        rest = k[len("stem.conv1."):]
        return {"weight": "conv1_w", "norm.weight": "res_conv1_bn_s", "norm.bias": "res_conv1_bn_b"}.get(rest)
    stage, blk, conv, rest = k.split(".", 3)
    br = {"shortcut": "branch1", "conv1": "branch2a", "conv2": "branch2b"}[conv]
    suffix = {"weight": "w", "norm.weight": "bn_s", "norm.bias": "bn_b"}.get(rest)
    return None if suffix is None else "%s_%s_%s_%s" % (stage, blk, br, suffix)


@pytest.mark.parametrize("depth", [18, 34])
def test_c2_and_d2_named_checkpoints_load_every_backbone_tensor(tmp_path, depth):
    from ubteacher.checkpoint import DetectionTSCheckpointer, align_and_update_state_dicts, load_checkpoint_file
    from ubteacher.modeling import build_model
    from ubteacher.modeling.ts_ensemble import EnsembleTSModel
    cfg = _cfg("rcnn", _opts(depth))
    torch.manual_seed(0)
    student, teacher = build_model(cfg), build_model(cfg)
    rng = np.random.default_rng(1)
    backbone = {k: v for k, v in student.state_dict().items() if k.startswith("backbone.bottom_up.")}
    n_convs = 1 + sum(2 * n for n in BLOCKS[depth]) + 3
    assert len(backbone) == 5 * n_convs
    # Caffe2 blob names (weights and the affine of every norm; such pickles hold no running statistics)
    blobs, expect = {}, {}
    for k, v in backbone.items():
        c2 = _to_c2_name(k)
        if c2 is None:
            continue
        arr = rng.standard_normal(tuple(v.shape)).astype(np.float32)
        blobs[c2] = arr
        expect[k] = torch.from_numpy(arr)
    blobs["fc1000_w"] = rng.standard_normal((1000, 512)).astype(np.float32)
    blobs["fc1000_b"] = np.zeros(1000, np.float32)
    path = os.path.join(tmp_path, "R-%d.pkl" % depth)
    with open(path, "wb") as f:
        pickle.dump({"blobs": blobs}, f)
    matched, unmatched = align_and_update_state_dicts(student.state_dict(), load_checkpoint_file(path)["model"])
    assert unmatched == [] and set(matched) == set(expect)
    ck = DetectionTSCheckpointer(EnsembleTSModel(teacher, student), str(tmp_path))
    ck.load(path)
    assert ck.last_load_report["unmatched_checkpoint_keys"] == []
    assert len(expect) == 3 * n_convs
    sd = student.state_dict()
    for k, v in expect.items():
        assert torch.equal(sd[k], v), k
    # Detectron2 names: every tensor of the backbone, running statistics included
    d2 = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32)) for k, v in backbone.items()}
    path2 = os.path.join(tmp_path, "R-%d_d2.pth" % depth)
    torch.save({"model": d2}, path2)
    ck.load(path2)
    sd = student.state_dict()
    for k, v in d2.items():
        assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("freeze_at,frozen_prefixes", [(2, ("stem", "res2")), (1, ("stem",)), (0, ())])
def test_freeze_at_decides_the_arena_kind(freeze_at, frozen_prefixes):
    m = _model("fcos", _opts(18, "MODEL.BACKBONE.FREEZE_AT", freeze_at))
    seen = 0
    for h in m.store.handles:
        for key, _ in h.exports:
            if key.startswith("backbone.bottom_up.") and key.endswith(".weight") and ".norm." not in key:
                part = key.split(".")[2]
                assert h.kind == ("frozen" if part in frozen_prefixes else "decay"), key
                seen += 1
    assert seen == 1 + 2 * 8 + 3
    for name, blocks, trainable in m.backbone.bottom_up.stages:
        assert trainable == (name not in frozen_prefixes)
        assert all(c.trainable == trainable for b in blocks for c in (b.conv1, b.conv2, b.shortcut) if c is not None)
    # the fused bottleneck node's pre-mask contract is not switched on for plain conv nodes: each masks its own incoming gradient
    assert not any(l.premask_input for l in m.backbone.lateral.values())
    assert not any(c.grad_premasked for _, blocks, _ in m.backbone.bottom_up.stages for b in blocks for c in (b.conv1, b.conv2))


def test_r50_keeps_its_premask_flags():
    m = _model("fcos", [])
    assert all(l.premask_input for l in m.backbone.lateral.values())
    assert all(b.input_relu and b.grad_premasked for name, blocks, tr in m.backbone.bottom_up.stages if tr for b in blocks)


@pytest.mark.parametrize("h16", [torch.bfloat16, torch.float16])
def test_exact_basicblock_operands_meet_their_preconditions(h16):
    """tests/basicblock_ref.py: exact domain, live ReLUs, a decisive residual - and the rounding of c1 is live in either 16-bit type"""
    from tests import basicblock_ref as B
    from tests import exact_conv_ref as R
    for shape in B.SHAPES:
        o = B.basicblock_operands(shape)
        assert all(torch.equal(o[k].to(h16).float(), o[k]) for k in ("x", "w1", "w2"))
        y, c1, y0 = B.basicblock_domain(o, h16)
        pre = R.conv_fwd_ref(o["x"], o["w1"], 3, 1, 1, o["s1"], o["b1"], relu=True)
        ties, inexact = R.tie_and_inexact_share(pre, h16)
        assert inexact > 0.01 and ties > 0.005
        assert tuple(y.shape) == tuple(o["x"].shape)
