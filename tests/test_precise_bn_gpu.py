"""TEST.PRECISE_BN on the GPU: a tiny FCOS NORM "BN" student at a 96 x 128 canvas, 2 + 2 images, on a fixed list of batches.

(a) update_bn_stats against a reference made with code the parent commit already has: per batch the layers' momentum is set to 1.0, the
    training-mode forward of the same two calls (label_q + label_k, then unlabel_q) runs, the fp32 running buffers after each call are
    that call's batch mean and unbiased batch variance, and tests/precise_bn_ref64.py turns them into population statistics.
    The reference's inputs are rounded to fp32 (2^-24 relative each), the result is rounded once more:
        running_mean within 2^-22 * max |batch mean|,  running_var within 2^-21 * pop_sq     (per layer, level and channel)
    Both forwards run the same kernels under no_grad, so the comparison holds in the fp32 mode and in both 16-bit modes.
(b) nothing else moves; (c) the eval-mode head output with the new buffers against the reference's; (d) the hook's place in train_loop;
(e) NORM "GN" with the key on is the run with the key off, bit for bit; (f) "SyncBN" in a world of one rank equals "BN" bit for bit.
Every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "unbiased-teacher-v2_amd")):      # the child process of the last test runs this file as a script
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests import precise_bn_ref64 as R  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 96, 128
NUM_ITER = 3
BUFFER_KEYS = ("running_mean", "running_var", "num_batches_tracked")


def make_cfg(norm, amp=None, opts=()):
    from ubteacher.presets import get_config
    return get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "SOLVER.AMP.ENABLED", bool(amp), "MODEL.DEVICE", "cuda", "MODEL.FCOS.NORM", norm] + list(opts))


def make_trainer(norm, amp=None, opts=(), cls=None, loader=None):
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    if amp:
        os.environ["UTV2_PRECISION"] = amp
    else:
        os.environ.pop("UTV2_PRECISION", None)
    cfg = make_cfg(norm, amp, opts)
    torch.manual_seed(0)
    tr = (cls or UBTeacherTrainer)(cfg, data_loader=loader or SyntheticTwoCropLoader(cfg, height=H, width=W))
    tr.log_period = 10 ** 9
    tr.optimizer.param_groups[0]["lr"] = 1e-3
    return tr


@pytest.fixture(autouse=True)
def _precision_env():
    old = os.environ.get("UTV2_PRECISION")
    yield
    if old is None:
        os.environ.pop("UTV2_PRECISION", None)
    else:
        os.environ["UTV2_PRECISION"] = old


def fixed_batches(cfg, n=NUM_ITER, seed=7):
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    return SyntheticTwoCropLoader(cfg, height=H, width=W, seed=seed, num_batches=n).batches


def fresh(batches):
    return [tuple([dict(d) for d in part] for part in b) for b in batches]


def bn_layers(model):
    return model.proposal_generator.fcos_head.bn_layers


def buffers(model):
    """[layers, 2, L, C] fp32 on the host"""
    return torch.stack([torch.stack((b.running_mean.t, b.running_var.t)) for b in bn_layers(model)]).cpu().numpy()


def parent_reference(model, batches):
    """population statistics from momentum-1.0 training-mode forwards (what the parent commit can do) and precise_bn_ref64; the
    model's state is put back afterwards -> (list over layers of R.estimate results, max |batch mean| [layers, L, C])"""
    head = model.proposal_generator.fcos_head
    flat0, count0 = model.flat_state().clone(), head.bn_counter.value
    layers = bn_layers(model)
    streams = [[] for _ in layers]
    for b in layers:
        b.momentum = 1.0
    try:
        with torch.no_grad():
            for lq, lk, uq, _ in fresh(batches):
                for call, branch in ((lq + lk, "labeled"), ([{k: v for k, v in d.items() if k != "instances"} for d in uq], "raw")):
                    model(call, branch=branch)
                    got = buffers(model).astype(np.float64)
                    for i in range(len(layers)):
                        for l in range(got.shape[2]):
                            streams[i].append((l, got[i, 0, l], got[i, 1, l], len(call)))
    finally:
        for b in layers:
            b.momentum = 0.1
        model.flat_state().copy_(flat0)
        head.bn_counter.value = count0
    L, C = layers[0].gamma.t.shape
    refs = [R.estimate(L, C, s) for s in streams]
    maxmean = np.stack([np.max(np.stack([np.abs(m) * (np.arange(L)[:, None] == l) for l, m, _, _ in s]), axis=0) for s in streams])
    return refs, maxmean


def state_snapshot(tr):
    sd = {k: v.clone() for k, v in tr.model.state_dict().items() if not k.endswith(BUFFER_KEYS)}
    return sd, tr.model.store.mom.clone(), tr.model_teacher.flat_state().clone()


def head_eval_output(model, images):
    """eval-mode head output (logits, box) on a list of image dicts; the model's mode is put back"""
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            features, _ = model._features(images)
            big, meta, _ = model.proposal_generator._level_first(features)
            out = model.proposal_generator.fcos_head(big, meta)
            return out["logits"].float().clone(), out["box"].float().clone()
    finally:
        model.train(was)


@pytest.mark.parametrize("amp", [None, "fp16", "bf16"])
def test_update_bn_stats_against_the_parents_forward(amp):
    from ubteacher.engine.precise_bn import update_bn_stats
    tr = make_trainer("BN", amp)
    tr.iter = 1
    tr.run_step_full_semisup()                     # momentum buffers and running statistics that are not the initial ones
    model, head = tr.model, tr.model.proposal_generator.fcos_head
    batches = fixed_batches(tr.cfg)
    refs, maxmean = parent_reference(model, batches)
    ref_mean = np.stack([r["running_mean"] for r in refs])
    ref_var = np.stack([r["running_var"] for r in refs])
    pop_sq = np.stack([r["pop_sq"] for r in refs])

    # (c), first half: the eval-mode head output with the reference's buffers loaded
    probe = [{"image": d["image"]} for d in batches[0][3]]
    moving = buffers(model)
    for b, m, v in zip(bn_layers(model), ref_mean, ref_var):
        b.running_mean.t.copy_(torch.from_numpy(m.astype(np.float32)))
        b.running_var.t.copy_(torch.from_numpy(v.astype(np.float32)))
    want_logits, want_box = head_eval_output(model, probe)
    for b, mv in zip(bn_layers(model), moving):
        b.running_mean.t.copy_(torch.from_numpy(mv[0]))
        b.running_var.t.copy_(torch.from_numpy(mv[1]))

    before, count0 = state_snapshot(tr), head.bn_counter.value
    assert model.training and head.training
    n = update_bn_stats(model, iter(fresh(batches)), NUM_ITER)
    torch.cuda.synchronize()
    assert n == len(bn_layers(model)) > 0

    # (a)
    got = buffers(model).astype(np.float64)
    e_mean, b_mean = np.abs(got[:, 0] - ref_mean), 2.0 ** -22 * maxmean
    e_var, b_var = np.abs(got[:, 1] - ref_var), 2.0 ** -21 * pop_sq
    print("[%s] running_mean: largest error %.3e = %.3g of its bound; running_var: %.3e = %.3g of its bound"
          % (amp or "fp32", e_mean.max(), (e_mean / b_mean).max(), e_var.max(), (e_var / b_var).max()))
    assert bool((e_mean <= b_mean).all()), float((e_mean / b_mean).max())
    assert bool((e_var <= b_var).all()), float((e_var / b_var).max())
    assert float(np.abs(got - moving).max()) > 1e-3, "the buffers are the population statistics, not the moving averages"
    assert float(got[:, 1].min()) > 0

    # (b)
    after = state_snapshot(tr)
    assert sorted(after[0]) == sorted(before[0])
    for k in before[0]:
        assert torch.equal(after[0][k], before[0][k]), k
    assert torch.equal(after[1], before[1]), "the optimizer's momentum buffers"
    assert torch.equal(after[2], before[2]), "the teacher"
    assert model.training and head.training and all(b.training and b.momentum == 0.1 for b in bn_layers(model))
    assert head.bn_counter.value == count0 + 2 * NUM_ITER, "num_batches_tracked: once per forward call"

    # (c): the new buffers differ from the reference's by at most 2^-21 relative (above).  A BatchNorm layer turns a relative change e of
    # its variance and a change e * max |batch mean| of its mean into at most e * (|xhat| / 2 + 1) * |gamma| per output element, |xhat| < 16
    # on these maps: 9 e per layer, added over the 4 tower depths and carried by the convs as a fraction of the output's largest magnitude:
    # 36 * 2^-21 = 1.7e-5; the bound is 4 times that for the convs' own gain.  In the 16-bit modes the activations are rounded to 2^-8
    # (bf16) or 2^-11 (fp16), and a perturbed value can fall on the other side of a rounding boundary: one step of the layer's output there.
    got_logits, got_box = head_eval_output(model, probe)
    tol = 4 * 36 * 2.0 ** -21 + {None: 0.0, "fp16": 4 * 2.0 ** -11, "bf16": 4 * 2.0 ** -8}[amp]
    for name, g, w in (("logits", got_logits, want_logits), ("box", got_box, want_box)):
        err, mag = float((g - w).abs().max()), float(w.abs().max())
        print("[%s] eval head %-6s largest difference %.3e of magnitude %.3e (bound %.3e)" % (amp or "fp32", name, err, mag, tol * mag))
        assert err <= tol * mag, (name, err, tol * mag)
    model.eval()
    with torch.no_grad():
        res = model(probe)
    model.train()
    assert len(res) == len(probe) and sum(len(r["instances"]) for r in res) > 0


def test_a_loader_that_ends_early_is_an_error():
    from ubteacher.engine.precise_bn import update_bn_stats
    tr = make_trainer("BN")
    batches = fixed_batches(tr.cfg, 2)
    before = buffers(tr.model)
    with pytest.raises(RuntimeError, match="stops at 2 iterations"):
        update_bn_stats(tr.model, iter(fresh(batches)), 3)
    torch.cuda.synchronize()
    assert np.array_equal(buffers(tr.model), before), "nothing is committed"


def test_unpaired_towers_give_the_paired_statistics(monkeypatch):
    """UTV2_PAIR_TOWERS: depth i of both towers as one [P, 2C] layer, or two chains of C channels - the same statistics per reference
    module (the same sums per output channel; 1e-5 relative covers the other tile shapes of the C -> C convs)"""
    from ubteacher.engine.precise_bn import update_bn_stats
    sds = []
    for paired in ("1", "0"):
        monkeypatch.setenv("UTV2_PAIR_TOWERS", paired)
        tr = make_trainer("BN")
        assert tr.model.proposal_generator.fcos_head.paired == (paired == "1")
        update_bn_stats(tr.model, iter(fresh(fixed_batches(tr.cfg))), NUM_ITER)
        torch.cuda.synchronize()
        sds.append({k: v.cpu().double() for k, v in tr.model.state_dict().items()
                    if ".fcos_head." in k and k.endswith(BUFFER_KEYS[:2])})
    want, got = sds
    assert len(want) == 2 * 4 * 5 * 2 and sorted(want) == sorted(got)
    for k, v in got.items():
        err = float((v - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-12)
        assert err <= 1e-5, (k, err)


class _Events:
    log = []


def _recording_trainer(norm, opts, tmp_path, train_batches=None):
    """a trainer whose hook loader, checkpointer and evaluations write into _Events.log"""
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    _Events.log = []

    class Counting:
        def __init__(self, inner):
            self.inner, self.n = iter(inner), 0

        def __iter__(self):
            return self

        def __next__(self):
            self.n += 1
            return next(self.inner)

    class T(UBTeacherTrainer):
        @classmethod
        def build_train_loader(cls, cfg):
            _Events.log.append(("hook loader built", int(cfg.DATALOADER.NUM_WORKERS)))
            return SyntheticTwoCropLoader(cfg, height=H, width=W, seed=11, num_batches=2)

        @classmethod
        def test(cls, cfg, model, evaluators=None):
            _Events.log.append(("eval", buffers(model) if bn_layers(model) else None))
            return {}

    cfg = make_cfg(norm, None, ["SOLVER.MAX_ITER", 4, "TEST.EVAL_PERIOD", 2, "SOLVER.CHECKPOINT_PERIOD", 2, "TEST.PRECISE_BN.NUM_ITER", 2,
                                "OUTPUT_DIR", str(tmp_path)] + list(opts))
    loader = Counting(SyntheticTwoCropLoader(cfg, height=H, width=W, seed=3, num_batches=4))
    tr = make_trainer(norm, None, ["SOLVER.MAX_ITER", 4, "TEST.EVAL_PERIOD", 2, "SOLVER.CHECKPOINT_PERIOD", 2, "TEST.PRECISE_BN.NUM_ITER", 2,
                                   "OUTPUT_DIR", str(tmp_path)] + list(opts), cls=T, loader=loader)
    save = tr.checkpointer.save
    tr.checkpointer.save = lambda name, **kw: (_Events.log.append(("checkpoint", name)), save(name, **kw))[1]
    losses = []
    step = tr.run_step_full_semisup
    tr.run_step_full_semisup = lambda: losses.append(step().detach().clone())
    if tr._precise_bn is not None:
        update = tr._precise_bn.update_stats

        def recorded():
            before = buffers(tr.model)
            update()
            _Events.log.append(("precise_bn", tr.iter, before, buffers(tr.model)))
        tr._precise_bn.update_stats = recorded
    return tr, loader, losses


def test_hook_runs_before_the_checkpoint_and_both_evaluations(tmp_path):
    tr, loader, _ = _recording_trainer("BN", ["TEST.PRECISE_BN.ENABLED", True], tmp_path)
    tr.train_loop(0, 4)
    torch.cuda.synchronize()
    kinds = [(e[0], e[1]) if e[0] == "checkpoint" else e[0] for e in _Events.log]
    print(kinds)
    assert kinds == ["hook loader built", "precise_bn", ("checkpoint", "model_0000001"), "eval", "eval",
                     "precise_bn", ("checkpoint", "model_0000003"), ("checkpoint", "model_final"), "eval", "eval"]
    assert _Events.log[0] == ("hook loader built", 0)
    assert loader.n == 4, "the training loader yielded exactly MAX_ITER batches"
    _, it, before, committed = _Events.log[1]
    assert it == 1 and float(np.abs(committed - before).max()) > 1e-3, "the hook replaced the moving averages"
    from ubteacher.checkpoint import load_checkpoint_file
    sd = load_checkpoint_file(os.path.join(str(tmp_path), "model_0000001.pth"))["model"]
    for i, tower in enumerate(("cls_tower", "bbox_tower")):
        for d in range(4):
            for l in range(5):
                for j, kind in enumerate(BUFFER_KEYS[:2]):
                    got = sd["modelStudent.proposal_generator.fcos_head.%s.%d.%d.%s" % (tower, 3 * d + 1, l, kind)].numpy()
                    assert np.array_equal(got, committed[d, j, l, 256 * i:256 * (i + 1)]), (tower, d, l, kind)
    assert np.array_equal(_Events.log[3][1], committed), "the student's evaluation of that iteration ran on the committed statistics"
    assert tr._precise_bn.updates == 2 and tr.model.training


def test_gn_run_with_the_key_on_is_the_run_with_the_key_off(tmp_path):
    out = []
    for on in (False, True):
        d = tmp_path / ("on" if on else "off")
        tr, loader, losses = _recording_trainer("GN", ["TEST.PRECISE_BN.ENABLED", on], d)
        assert tr._precise_bn is None
        tr.train_loop(0, 4)
        torch.cuda.synchronize()
        assert loader.n == 4 and not any(e[0] in ("precise_bn", "hook loader built") for e in _Events.log)
        out.append((torch.stack(losses).cpu(), {k: v.cpu() for k, v in tr.model.state_dict().items()}, tr.model_teacher.flat_state().cpu()))
    (la, sa, ta), (lb, sb, tb) = out
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all()), (la, lb)
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(ta, tb)


def _world_of_one_child(norm, out_path):
    """fresh process: a process group of one rank with the data-parallel machinery on (UTV2_DP_SINGLE_RANK=1), update_bn_stats"""
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(s.getsockname()[1])
    s.close()
    dist.init_process_group("gloo", rank=0, world_size=1)
    torch.cuda.set_device(0)
    from ubteacher.engine.precise_bn import update_bn_stats
    tr = make_trainer(norm)
    assert tr.data_parallel and tr.model.proposal_generator.fcos_head.norm == norm
    update_bn_stats(tr.model, iter(fresh(fixed_batches(tr.cfg))), NUM_ITER)
    torch.cuda.synchronize()
    np.save(out_path, buffers(tr.model))
    dist.destroy_process_group()


def test_syncbn_in_a_world_of_one_equals_bn_bit_for_bit(tmp_path):
    from ubteacher.engine.precise_bn import update_bn_stats
    out = str(tmp_path / "syncbn.npy")
    env = dict(os.environ, UTV2_DP_SINGLE_RANK="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "UTV2_PRECISION"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "SyncBN", out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    tr = make_trainer("BN")
    update_bn_stats(tr.model, iter(fresh(fixed_batches(tr.cfg))), NUM_ITER)
    torch.cuda.synchronize()
    bn, sync = buffers(tr.model), np.load(out)
    assert float(np.abs(bn[:, 0]).max()) > 0 and np.array_equal(bn.view(np.uint32), sync.view(np.uint32))


if __name__ == "__main__":
    _world_of_one_child(sys.argv[1], sys.argv[2])
