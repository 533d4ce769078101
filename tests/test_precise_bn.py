"""TEST.PRECISE_BN without a GPU: the host estimator of ubteacher/engine/precise_bn.py against tests/precise_bn_ref64.py, the hook's
schedule, when a hook is built, and get_bn_modules.

Estimator tolerance: both sides are a handful of fp64 operations per element in (possibly) another association order: 1e-13 relative to
max(|value|, pop_sq) (fewer than 100 operations of 1.1e-16 each, see tests/test_bn_precise_kernels_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import precise_bn_ref64 as R


def _cfg(kind, opts):
    from ubteacher.presets import get_config
    return get_config(kind, 1, ["MODEL.DEVICE", "cpu", "SOLVER.IMG_PER_BATCH_LABEL", 1, "SOLVER.IMG_PER_BATCH_UNLABEL", 1] + list(opts))


def _trainer(kind, opts):
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBRCNNTeacherTrainer, UBTeacherTrainer
    cfg = _cfg(kind, opts)
    torch.manual_seed(0)
    return (UBTeacherTrainer if kind == "fcos" else UBRCNNTeacherTrainer)(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=32, width=32))


def _hand_made_sets(L, C, plan, seed=3):
    """plan: (level, B) per set -> sets with |mean| <= std"""
    rng = np.random.default_rng(seed)
    return [(l, rng.uniform(-1.0, 1.0, C), rng.uniform(1.0, 2.0, C), B) for l, B in plan]


@pytest.mark.parametrize("plan", [
    [(0, 4), (0, 2), (1, 4), (1, 2), (0, 4), (0, 2), (1, 4), (1, 2)],     # two sets of unequal B per level and iteration
    [(0, 2), (0, 3), (1, 5), (0, 2), (0, 3)],                              # level 1 receives one set only
    [(0, 1), (0, 7)],                                                       # B = 1: the set's variance does not enter q
])
def test_host_estimator_against_ref64(plan):
    from ubteacher.engine.precise_bn import PopulationStatistics
    L, C = 2, 8
    sets = _hand_made_sets(L, C, plan)
    est = PopulationStatistics(L, C)
    for l, m, v, B in sets:
        est.update(l, m, v, B)
    ref = R.estimate(L, C, sets)
    mean, var = est.result()
    scale = np.maximum(np.abs(ref["pop_mean"]), ref["pop_sq"])
    for name, got, want in (("pop_mean", est.pop_mean, ref["pop_mean"]), ("pop_sq", est.pop_sq, ref["pop_sq"]),
                            ("running_mean", mean, ref["running_mean"]), ("running_var", var, ref["running_var"])):
        err = float(np.max(np.abs(got - want) - 1e-13 * scale))     # a level no set reached: 0 against 0
        print("%-12s largest |error| - 1e-13 * scale: %.3e" % (name, err))
        assert err <= 0.0, (name, err)
    assert np.array_equal(est.num, ref["num"])
    # one set only: the population statistics are that set's; with B images the variance is v * (B - 1) / B
    if len(plan) > 2 and plan[2] == (1, 5):
        _, m, v, B = sets[2]
        assert np.allclose(mean[1], m, rtol=1e-14, atol=0) and np.allclose(var[1], v * (B - 1) / B, rtol=1e-13, atol=0)


def test_host_estimator_refuses_an_empty_call():
    from ubteacher.engine.precise_bn import PopulationStatistics
    with pytest.raises(ValueError):
        PopulationStatistics(1, 4).update(0, np.zeros(4), np.ones(4), 0)


@pytest.mark.parametrize("max_iter,period,want", [(5, 2, [1, 3, 4]), (5, 0, [4]), (4, 2, [1, 3]), (3, 7, [2])])
def test_hook_schedule(max_iter, period, want):
    from ubteacher.engine.precise_bn import PreciseBN, hook_is_due
    assert R.fires_after(max_iter, period) == want
    assert [it for it in range(max_iter) if hook_is_due(it, max_iter, period)] == want
    fired = []
    hook = PreciseBN(period, None, None, 3)
    hook.update_stats = lambda: fired.append(it)
    for it in range(max_iter):
        assert hook.after_step(it, max_iter) == (it in want)
    assert fired == want


@pytest.mark.parametrize("norm", ["BN", "SyncBN"])
def test_hook_is_built_for_batchnorm_towers_with_the_key_on(norm):
    from ubteacher.engine.precise_bn import PreciseBN
    tr = _trainer("fcos", ["MODEL.FCOS.NORM", norm, "TEST.PRECISE_BN.ENABLED", True, "TEST.PRECISE_BN.NUM_ITER", 7, "TEST.EVAL_PERIOD", 11])
    hook = tr._precise_bn
    assert isinstance(hook, PreciseBN) and hook.model is tr.model and hook.num_iter == 7 and hook.period == 11
    assert hook._data_iter is None, "the hook's loader is built at its first update"


@pytest.mark.parametrize("kind,opts", [
    ("fcos", ["MODEL.FCOS.NORM", "BN"]),                                       # the key is off (its default)
    ("fcos", ["MODEL.FCOS.NORM", "GN", "TEST.PRECISE_BN.ENABLED", True]),
    ("fcos", ["MODEL.FCOS.NORM", "none", "TEST.PRECISE_BN.ENABLED", True]),
    ("rcnn", ["TEST.PRECISE_BN.ENABLED", True]),
])
def test_hook_is_not_built(kind, opts):
    assert _trainer(kind, opts)._precise_bn is None


def test_the_hooks_loader_is_a_train_loader_of_its_own_without_workers():
    from ubteacher.engine import UBTeacherTrainer
    seen = []

    class T(UBTeacherTrainer):
        @classmethod
        def build_train_loader(cls, cfg):
            seen.append(int(cfg.DATALOADER.NUM_WORKERS))
            return "loader"
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    cfg = _cfg("fcos", ["MODEL.FCOS.NORM", "BN", "TEST.PRECISE_BN.ENABLED", True, "DATALOADER.NUM_WORKERS", 4])
    tr = T(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=32, width=32))
    assert seen == [] and tr._build_precise_bn_loader() == "loader" and seen == [0]
    assert int(tr.cfg.DATALOADER.NUM_WORKERS) == 4


@pytest.mark.parametrize("paired", [False, True])
def test_get_bn_modules(paired, monkeypatch):
    """Two towers of `depth` convs: 2 x depth BatchNorm layer objects of width C.  The paired layout (UTV2_PAIR_TOWERS, the default) keeps
    depth i of both towers in ONE layer object of width 2C - the same 2 x depth x L modules of the reference, held by `depth` objects."""
    from ubteacher import ops
    from ubteacher.engine.precise_bn import get_bn_modules
    from ubteacher.modeling import build_model
    monkeypatch.setenv("UTV2_PAIR_TOWERS", "1" if paired else "0")
    cfg = _cfg("fcos", ["MODEL.FCOS.NORM", "BN"])
    depth = cfg.MODEL.FCOS.NUM_CLS_CONVS
    assert depth == cfg.MODEL.FCOS.NUM_BOX_CONVS and depth > 0
    bns = get_bn_modules(build_model(cfg))
    assert all(isinstance(b, ops.BatchNormReLU) for b in bns)
    if paired:
        assert len(bns) == depth and all(b.gamma.t.shape[1] == 2 * 256 for b in bns)
    else:
        assert len(bns) == 2 * depth and all(b.gamma.t.shape[1] == 256 for b in bns)
    assert sum(b.gamma.t.shape[1] for b in bns) == 2 * depth * 256
    assert get_bn_modules(build_model(_cfg("fcos", ["MODEL.FCOS.NORM", "GN"]))) == []
    assert get_bn_modules(build_model(_cfg("rcnn", []))) == []


def test_update_bn_stats_without_batchnorm_layers_does_nothing():
    from ubteacher.engine.precise_bn import update_bn_stats
    from ubteacher.modeling import build_model
    m = build_model(_cfg("fcos", ["MODEL.FCOS.NORM", "GN"]))
    before = m.flat_state().clone()
    assert update_bn_stats(m, iter(()), 3) == 0 and torch.equal(m.flat_state(), before)
