"""MODEL.FCOS.NORM "BN" / "SyncBN" / "none" without a GPU: the model builds, its state dict has the reference's keys and shapes
(tests/golden/fcos_norm.npz, written by gen_golden_fcos_norm.py from the reference's own FCOSHead) in both tower layouts, checkpoints
travel between the layouts, any other value is refused by name, and "GN" is what it was."""
import os
import re

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_norm.npz")
HEAD = "proposal_generator.fcos_head."


def build(norm, paired, monkeypatch, seed=0):
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    monkeypatch.setenv("UTV2_PAIR_TOWERS", "1" if paired else "0")
    cfg = get_config("fcos", 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.NORM", norm])
    torch.manual_seed(seed)
    return build_model(cfg)


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("norm", ["BN", "SyncBN", "none"])
def test_state_dict_keys_and_shapes_are_the_references(norm, paired, monkeypatch):
    gold = np.load(GOLD)
    want = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(gold[norm + "_keys"], gold[norm + "_shapes"])}
    m = build(norm, paired, monkeypatch)
    assert m.proposal_generator.fcos_head.paired == paired
    got = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith(HEAD)}
    assert sorted(got) == sorted(want)
    assert got == want
    sd = m.state_dict()
    if norm != "none":
        # the reference's module order inside one norm slot, initial values, and the kinds: weight decay as for GN, buffers under the EMA
        keys = [k for k in sd if k.startswith(HEAD + "bbox_tower.4.2.")]
        assert [k.rsplit(".", 1)[1] for k in keys] == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
        assert sd[keys[4]].dtype == torch.int64 and int(sd[keys[4]]) == 0
        assert float(sd[keys[0]].min()) == 1.0 and float(sd[keys[1]].abs().max()) == 0.0
        assert float(sd[keys[2]].abs().max()) == 0.0 and float(sd[keys[3]].min()) == 1.0
        st = m.store
        for bn in m.proposal_generator.fcos_head.bn_layers:
            assert bn.gamma.kind == bn.beta.kind == "nodecay" and bn.running_mean.kind == bn.running_var.kind == "buffer"
            lo, hi = st.ranges["buffer"]
            assert lo <= bn.running_mean.offset < hi and hi <= st.flat.numel()      # inside flat_state(): the EMA's one launch covers it
    else:
        assert not [k for k in sd if re.search(r"_tower\.(1|3|5|7)\.", k)]


def test_other_norm_values_are_refused_by_key(monkeypatch):
    with pytest.raises(NotImplementedError, match=r"MODEL\.FCOS\.NORM"):
        build("LN", True, monkeypatch)


def test_initialisation_stream_does_not_depend_on_the_norm(monkeypatch):
    """norm layers draw nothing: the conv weights of a BN / none head are those of the GN head under the same seed"""
    ref = build("GN", True, monkeypatch).state_dict()
    for norm in ("BN", "none"):
        sd = build(norm, True, monkeypatch).state_dict()
        step = 2 if norm == "none" else 3
        for tower in ("cls_tower", "bbox_tower"):
            for i in range(4):
                assert torch.equal(sd["%s%s.%d.weight" % (HEAD, tower, step * i)], ref["%s%s.%d.weight" % (HEAD, tower, 3 * i)])
        assert torch.equal(sd[HEAD + "cls_logits.weight"], ref[HEAD + "cls_logits.weight"])
        assert torch.equal(sd[HEAD + "ctrness.weight"], ref[HEAD + "ctrness.weight"])


def test_bn_checkpoint_round_trip_and_across_tower_layouts(monkeypatch, tmp_path):
    from ubteacher.checkpoint import DetectionCheckpointer
    a = build("BN", True, monkeypatch, seed=1)
    with torch.no_grad():
        a.store.flat.add_(torch.randn(a.store.flat.shape, generator=torch.Generator().manual_seed(2)) * 0.01)
    a.proposal_generator.fcos_head.bn_counter.value = 7
    DetectionCheckpointer(a, str(tmp_path)).save("bn")
    want = {k: v.clone() for k, v in a.state_dict().items()}
    for paired in (True, False):
        b = build("BN", paired, monkeypatch, seed=3)
        DetectionCheckpointer(b, str(tmp_path)).load(os.path.join(str(tmp_path), "bn.pth"))
        got = b.state_dict()
        assert list(got) == list(want) or sorted(got) == sorted(want)
        for k, v in want.items():
            assert torch.equal(got[k], v), k
        assert b.proposal_generator.fcos_head.bn_counter.value == 7
    # num_batches_tracked is read when present and ignored when absent (strict load included)
    b = build("BN", True, monkeypatch, seed=3)
    b.load_state_dict({k: v for k, v in want.items() if not k.endswith("num_batches_tracked")}, strict=True)
    assert b.proposal_generator.fcos_head.bn_counter.value == 0


def test_gn_key_list_is_unchanged(monkeypatch):
    cont = np.load(os.path.join(os.path.dirname(GOLD), "fcos_cont_outputs.npz"))
    for paired in (True, False):
        sd = build("GN", paired, monkeypatch).state_dict()
        tower = [k for k in sd if "_tower." in k]
        want = ["%s%s_tower.%d.%s" % (HEAD, t, 3 * i + j, p) for t in ("cls", "bbox") for i in range(4) for j in (0, 1) for p in ("weight", "bias")]
        assert tower == want
        assert not m_has_host_ints(sd)
    # ... and the whole FCOS module's keys are still the reference's (recorded for REG_DISCRETE False by gen_golden_fcos_cont.py)
    from ubteacher.modeling import build_model
    from ubteacher.presets import get_config
    m = build_model(get_config("fcos", 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.REG_DISCRETE", False]))
    got = [k for k in m.state_dict() if k.startswith("proposal_generator.")]
    assert sorted(got) == sorted(str(k) for k in cont["keys_kl"])


def m_has_host_ints(sd):
    return [k for k in sd if k.endswith("num_batches_tracked")]
