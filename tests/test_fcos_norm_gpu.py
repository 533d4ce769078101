"""MODEL.FCOS.NORM "BN" / "SyncBN" / "none" on the GPU: the head against the reference's own FCOSHead (tests/golden/fcos_norm.npz), whole
semi-supervised steps (state, EMA, num_batches_tracked), the "BN" step as a hipGraph, and test-mode inference."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_norm.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "proposal_generator.fcos_head"
STEP_LR = 1e-3
MOVE_LR = 1e3       # see the end of test_whole_step_state_ema_and_counters


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)


def perturb_norm_params(sd, seed):      # as tests/golden/gen_golden_fcos_norm.py
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in sorted(sd):
            if re.search(r"_tower\.\d+\.\d+\.(weight|bias)$", k):
                sd[k] += 0.2 * torch.randn(sd[k].shape, generator=g)


def make_head(norm, device, seed):
    from ubteacher.modeling.fcos import FCOSHead
    from ubteacher.params import ParamStore
    from ubteacher.presets import get_config
    cfg = get_config("fcos", 1, ["MODEL.DEVICE", "cpu", "MODEL.FCOS.NORM", norm])
    store = ParamStore()
    torch.manual_seed(seed)
    head = FCOSHead(cfg, store, 256, PREFIX)
    store.finalize(torch.device(device))
    return head, store


def level_first(xs, device):
    """per-level NCHW arrays of equal batch -> the level-first [P, C] matrix"""
    return torch.cat([torch.as_tensor(x).permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs]).contiguous().to(device)


def src(gold, norm):
    """the golden's prefix for `norm`: a world-of-one SyncBN is stored as the BN arrays it equalled bit for bit"""
    return "BN" if (norm == "SyncBN" and bool(gold["SyncBN_same_as_BN"])) else norm


def check_outputs(gold, norm, call, out, meta, img0, n, R4):
    for l in range(len(meta.level_hw)):
        lg = meta.level_view(out["logits"], l)[img0:img0 + n].permute(0, 3, 1, 2)
        bx = meta.level_view(out["box"], l)[img0:img0 + n].permute(0, 3, 1, 2)
        for name, got in (("logits", lg), ("reg", bx[:, :R4]), ("std", bx[:, R4:R4 + 4]), ("ctr", bx[:, R4 + 4:R4 + 5])):
            e = relerr(got, gold["%s_%s_%s_%d" % (src(gold, norm), call, name, l)])
            assert e <= 1e-3, (norm, call, name, l, e)


def check_running(gold, norm, call, store):
    sd = store.state_dict()
    L = 5
    for tower in ("cls_tower", "bbox_tower"):
        for kind in ("running_mean", "running_var"):
            want = gold["%s_%s_%s_%s" % (src(gold, norm), call, tower, kind)]
            got = torch.stack([torch.stack([sd["%s.%s.%d.%d.%s" % (PREFIX, tower, 3 * i + 1, l, kind)] for l in range(L)]) for i in range(want.shape[0])])
            e = relerr(got, want)
            assert e <= 1e-3, (norm, call, tower, kind, e)
    nbt = {int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")}
    assert nbt == {int(gold["%s_%s_num_batches_tracked" % (src(gold, norm), call)])}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("norm", ["BN", "SyncBN", "none"])
def test_head_against_the_reference_golden(norm, fused):
    from ubteacher import ops
    ops.set_precision("fp32")
    gold = np.load(GOLD)
    seed = int(gold["seed"])
    level_hw = [tuple(int(v) for v in hw) for hw in gold["level_hw"]]
    cpu_head, cpu_store = make_head(norm, "cpu", seed)
    sd = {k: v.clone() for k, v in cpu_store.state_dict().items()}
    perturb_norm_params(sd, seed + 1)
    head, store = make_head(norm, "cuda", seed)
    store.load_state_dict(sd)
    R4 = head.R4
    xs = {c: [gold["x_%s_%d" % (c, l)] for l in range(5)] for c in ("labeled", "unlabeled", "eval")}
    with torch.no_grad():
        if fused:   # the two training calls as one batch with two statistic sets per level
            both = [np.concatenate([a, b]) for a, b in zip(xs["labeled"], xs["unlabeled"])]
            meta = ops.LevelMeta(4, level_hw)
            out = head(level_first(both, "cuda"), meta, calls=(2, 2))
            check_outputs(gold, norm, "labeled", out, meta, 0, 2, R4)
            check_outputs(gold, norm, "unlabeled", out, meta, 2, 2, R4)
            if norm != "none":
                check_running(gold, norm, "unlabeled", store)
        else:
            meta = ops.LevelMeta(2, level_hw)
            for call in ("labeled", "unlabeled"):
                out = head(level_first(xs[call], "cuda"), meta)
                check_outputs(gold, norm, call, out, meta, 0, 2, R4)
                if norm != "none":
                    check_running(gold, norm, call, store)
        before = store.flat.clone()
        head.train(False)
        meta = ops.LevelMeta(2, level_hw)
        out = head(level_first(xs["eval"], "cuda"), meta)
        check_outputs(gold, norm, "eval", out, meta, 0, 2, R4)
        assert torch.equal(store.flat, before), "eval mode writes no state"


def make_trainer(norm, amp, monkeypatch, burn=1):
    from ubteacher.data.synthetic import SyntheticTwoCropLoader
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    import bench
    if amp:
        monkeypatch.setenv("UTV2_PRECISION", amp)
    cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", burn,
                                 "SOLVER.AMP.ENABLED", bool(amp), "MODEL.DEVICE", "cuda", "MODEL.FCOS.NORM", norm])
    torch.manual_seed(0)
    tr = UBTeacherTrainer(cfg, data_loader=SyntheticTwoCropLoader(cfg, height=96, width=128))
    bench.tune_for_pseudo_labels(tr, tr._data_loader.batches[0])
    tr.log_period = 10 ** 9
    tr.optimizer.param_groups[0]["lr"] = STEP_LR
    return tr, cfg


def running(model):
    bns = model.proposal_generator.fcos_head.bn_layers
    return torch.cat([torch.cat((b.running_mean.t.reshape(-1), b.running_var.t.reshape(-1))) for b in bns]).clone()


@pytest.mark.parametrize("norm,amp", [("BN", None), ("SyncBN", None), ("none", None), ("BN", "bf16"), ("BN", "fp16")])
def test_whole_step_state_ema_and_counters(norm, amp, monkeypatch):
    tr, cfg = make_trainer(norm, amp, monkeypatch)
    keep = cfg.SEMISUPNET.EMA_KEEP_RATE
    head, thead = tr.model.proposal_generator.fcos_head, tr.model_teacher.proposal_generator.fcos_head
    f32 = np.float32

    def step():
        tr.run_step_full_semisup()
        rec = dict(tr.flush_metrics())
        tr.iter += 1
        losses = [v for k, v in rec.items() if k.startswith("loss")]
        assert losses and all(v == v and abs(v) < 1e6 for v in losses), rec
    tr.iter = 0
    step()                                       # burn-in: one forward call (labeled strong + weak views)
    if norm == "none":
        step(), step()
        assert not head.bn_layers and torch.isfinite(tr.model.flat_state()).all()
        return
    assert head.bn_counter.value == 1 and thead.bn_counter.value == 0
    s1 = running(tr.model)
    assert float((s1 - running(tr.model_teacher)).abs().max()) > 0, "the student's running statistics moved, the teacher's did not"
    step()                                       # end of burn-in: the teacher is a copy (keep_rate 0), then a fused pass (two calls)
    assert head.bn_counter.value == 3 and thead.bn_counter.value == 1
    t1 = running(tr.model_teacher)
    assert torch.equal(t1, s1), "burn-in copy: the teacher's running statistics are the student's"
    s2 = running(tr.model)
    assert float((s2 - s1).abs().max()) > 0
    step()                                       # EMA step
    want = s2.double() * (1 - keep) + t1.double() * keep
    assert relerr(running(tr.model_teacher), want) <= 1e-6
    assert head.bn_counter.value == 5
    assert thead.bn_counter.value == int(f32(3) * f32(1 - keep) + f32(1) * f32(keep))
    assert torch.isfinite(tr.model.flat_state()).all() and torch.isfinite(tr.model_teacher.flat_state()).all()
    # every level's gamma and beta receives a non-zero gradient (the gradient arena is zeroed at the start of the next backward, not
    # after the update) and moves.  The top levels of a 96 x 128 canvas hold one or two locations per image and give gamma gradients
    # of 1e-8 .. 1e-5; gamma sits at 1.0, where fp32 resolves steps of 2^-24, so at STEP_LR their update is below the spacing.  The
    # last step therefore runs at MOVE_LR, where lr * gradient of the smallest of them is thousands of spacings; the state after it is
    # of no further use and is not looked at
    params0 = [(b.gamma.t.clone(), b.beta.t.clone()) for b in head.bn_layers]
    tr.optimizer.param_groups[0]["lr"] = MOVE_LR
    tr.run_step_full_semisup()
    torch.cuda.synchronize()
    for i, (b, (g0, b0)) in enumerate(zip(head.bn_layers, params0)):
        gg, gb = b.gamma.g.abs().amax(dim=1), b.beta.g.abs().amax(dim=1)
        print("layer %d: largest |dgamma| per level %s  |dbeta| %s" % (i, [float("%.3g" % v) for v in gg], [float("%.3g" % v) for v in gb]))
        assert bool((gg > 0).all()) and bool((gb > 0).all()), (gg, gb)
        assert bool(((b.gamma.t - g0).abs().amax(dim=1) > 0).all()), "every level's gamma moved"
        assert bool(((b.beta.t - b0).abs().amax(dim=1) > 0).all()), "every level's beta moved"


def test_bn_step_as_hipgraph_replays_the_eager_step(monkeypatch):
    from ubteacher import ops
    outs = []
    try:
        for graph in (False, True):
            tr, _ = make_trainer("BN", None, monkeypatch, burn=0)
            tr.iter = 1
            recs = []
            for _ in range(5):
                (tr.run_step_graph if graph else tr.run_step_full_semisup)()
                tr.iter += 1
                recs.append(dict(tr.flush_metrics()))
            torch.cuda.synchronize()
            if graph:
                assert tr._step_graphs and all(st["graph"] is not None for st in tr._step_graphs.values())
            head = tr.model.proposal_generator.fcos_head
            outs.append((recs, running(tr.model), running(tr.model_teacher), head.bn_counter.value,
                         tr.model_teacher.proposal_generator.fcos_head.bn_counter.value))
    finally:
        ops.STEP_GRAPH[0] = False
    (ra, sa, ta, ca, cta), (rb, sb, tb, cb, ctb) = outs
    for a, b in zip(ra, rb):
        for k, v in a.items():
            if k.startswith("loss"):
                assert v == v and abs(b[k] - v) <= 1e-4 * max(abs(v), 1e-3), (k, v, b[k])
    assert relerr(sb, sa) <= 1e-4 and relerr(tb, ta) <= 1e-4
    assert (ca, cta) == (cb, ctb) == (10, cta)


def test_bn_test_mode_inference_returns_detections(monkeypatch):
    tr, _ = make_trainer("BN", None, monkeypatch, burn=0)
    tr.iter = 1
    tr.run_step_full_semisup()
    model = tr.model_teacher
    assert not model.training and not model.proposal_generator.fcos_head.training
    before = tr.model_teacher.flat_state().clone()
    batch = tr._data_loader.batches[0][3]
    with torch.no_grad():
        res = model([{"image": x["image"]} for x in batch])
    assert len(res) == len(batch) and sum(len(r["instances"]) for r in res) > 0
    assert torch.equal(tr.model_teacher.flat_state(), before)


# ---- NORM "GN" is what it was at the parent commit --------------------------------------------------------------------------------
GN_PARENT = os.path.join(os.path.dirname(GOLD), "gn_step_parent.npz")


def gn_step_record(amp):
    """one post-burn-in step of the shipped "GN" recipe from the CPU-initialised state and the batch of the step golden (fp32, or the
    fp16 build with its epilogue-fused GroupNorm statistics) -> losses, every 4001st element of the gradient arena, every 7th of its
    norm-parameter range, and the first elements of student and teacher after the step.  tests/golden/gn_step_parent.npz holds what
    the PARENT commit's sources and build returned from this function on an MI355X."""
    from tests.utv2_testutil import FixedLoader, golden_batches, golden_init_state, load_step_golden, tune_state_for_pseudo_labels
    from ubteacher.engine import UBTeacherTrainer
    from ubteacher.presets import get_config
    d = load_step_golden("fcos")
    _, sd0 = golden_init_state("fcos", d)
    prod, orac = golden_batches(d, "cuda")
    cfg = get_config("fcos", 1, ["SOLVER.IMG_PER_BATCH_LABEL", 2, "SOLVER.IMG_PER_BATCH_UNLABEL", 2, "SEMISUPNET.BURN_UP_STEP", 0,
                                 "SOLVER.AMP.ENABLED", bool(amp), "MODEL.DEVICE", "cuda"])
    assert cfg.MODEL.FCOS.NORM == "GN"
    tr = UBTeacherTrainer(cfg, data_loader=FixedLoader(prod))
    sd = tune_state_for_pseudo_labels(sd0, [x["image"] for x in orac[3]])
    tr.model.load_state_dict(sd)
    tr.model_teacher.load_state_dict(sd)
    tr.iter = 1
    tr.optimizer.param_groups[0]["lr"] = float(d["lr"])
    tr.run_step_full_semisup()
    rec = tr.flush_metrics()
    torch.cuda.synchronize()
    st = tr.model.store
    keys = sorted(k for k in rec if k.startswith("loss"))
    lo, hi = st.ranges["nodecay"]
    return {"loss_keys": np.array(keys), "loss_vals": np.array([rec[k] for k in keys], dtype=np.float64),
            "grad_sample": st.grad[::4001].cpu().numpy(), "grad_norm_params": st.grad[lo:hi:7].cpu().numpy(),
            "student_head": st.flat[:st.n_train:4001].cpu().numpy(), "teacher_head": tr.model_teacher.store.flat[::4001].cpu().numpy()}


@pytest.mark.parametrize("amp", [False, True])
def test_gn_step_is_bit_identical_to_the_parent_commit(amp, monkeypatch):
    monkeypatch.delenv("UTV2_PRECISION", raising=False)
    want = np.load(GN_PARENT)
    got = gn_step_record(amp)
    tag = "amp_" if amp else "f32_"
    assert list(got["loss_keys"]) == [str(k) for k in want[tag + "loss_keys"]]
    for k, v in got.items():
        if k != "loss_keys":
            assert v.shape == want[tag + k].shape and np.array_equal(v.view(np.uint8), want[tag + k].view(np.uint8)), k
    assert np.isfinite(got["loss_vals"]).all() and float(np.abs(got["grad_sample"]).max()) > 0


# ---- "SyncBN" on two ranks ---------------------------------------------------------------------------------------------------------
TWO_RANK_HW = [(6, 8), (3, 4), (2, 2), (1, 2), (1, 1)]


def _sync_case(seed=11):
    """(state dict of a CPU-initialised SyncBN head with perturbed norm parameters, whole batch of 4 images per level, loss weights)"""
    _, store = make_head("SyncBN", "cpu", seed)
    sd = {k: v.clone() for k, v in store.state_dict().items()}
    perturb_norm_params(sd, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    xs = [torch.randn(4, 256, h, w, generator=g) for h, w in TWO_RANK_HW]
    return sd, xs, g


def _head_forward_backward(norm, sd, xs, wl, wb):
    """training forward + backward of sum(logits * wl) + sum(box * wb) on the current device -> numpy dict"""
    from ubteacher import ops
    ops.set_precision("fp32")
    head, store = make_head(norm, "cuda", 0)
    store.load_state_dict({k.replace("SyncBN", norm): v for k, v in sd.items()})
    meta = ops.LevelMeta(xs[0].shape[0], TWO_RANK_HW)
    big = level_first(xs, "cuda").requires_grad_(True)
    out = head(big, meta)
    ((out["logits"] * wl.cuda()).sum() + (out["box"] * wb.cuda()).sum()).backward()
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    return {"logits": out["logits"].detach().cpu().numpy(), "box": out["box"].detach().cpu().numpy(), "dx": big.grad.cpu().numpy(),
            "grad": store.grad.cpu().numpy(), "running": running(types.SimpleNamespace(proposal_generator=types.SimpleNamespace(fcos_head=head))).cpu().numpy()}


def _rows_of(xs_n, img0, n):
    """row indices of images [img0, img0 + n) of a level-first matrix of xs_n images"""
    idx, r = [], 0
    for h, w in TWO_RANK_HW:
        idx += list(range(r + img0 * h * w, r + (img0 + n) * h * w))
        r += xs_n * h * w
    return idx


def _sync_worker(rank, world, port, backend, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(rank if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    sd, xs, g = _sync_case()
    P = sum(4 * h * w for h, w in TWO_RANK_HW)
    wl, wb = torch.randn(P, 80, generator=g), torch.randn(P, 80, generator=g)
    rows = _rows_of(4, 2 * rank, 2)
    res = _head_forward_backward("SyncBN", sd, [x[2 * rank:2 * rank + 2] for x in xs], wl[rows], wb[rows])
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _two_rank_syncbn(backend):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, backend, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # one rank, "BN", the whole batch: one statistic set per level over all four images
    sd, xs, g = _sync_case()
    P = sum(4 * h * w for h, w in TWO_RANK_HW)
    wl, wb = torch.randn(P, 80, generator=g), torch.randn(P, 80, generator=g)
    rm0 = np.concatenate([np.concatenate((np.zeros(5 * 512), np.ones(5 * 512)))] * 4)      # initial running statistics (paired towers: 4 layers)
    whole = _head_forward_backward("BN", sd, xs, wl, wb)
    for r in (0, 1):
        rows = _rows_of(4, 2 * r, 2)
        for k in ("logits", "box", "dx"):      # outputs and input gradients of the rank's images: the whole batch's rows
            assert relerr(res[r][k], whole[k][rows]) <= 1e-5, (r, k, relerr(res[r][k], whole[k][rows]))
    # parameter gradients: each rank holds its own conv sums and the ranks' MEAN of the norm sums, so the ranks' gradients add up to
    # the whole batch's (what the data-parallel average then halves on both sides alike)
    assert relerr(res[0]["grad"] + res[1]["grad"], whole["grad"]) <= 1e-4
    # running statistics: identical on both ranks; the mean is the whole batch's, the variance moved by the BIASED batch variance where
    # one-rank BN moves it by var * n / (n - 1): (rv_bn - rv0) = 0.1 * (var * n / (n - 1) - rv0)
    assert np.array_equal(res[0]["running"], res[1]["running"])
    n = np.repeat(np.array([4 * h * w for h, w in TWO_RANK_HW], dtype=np.float64), 512)
    got, bn = res[0]["running"].reshape(4, 2, -1).astype(np.float64), whole["running"].reshape(4, 2, -1).astype(np.float64)
    rv0 = rm0.reshape(4, 2, -1)[:, 1]
    assert relerr(got[:, 0], bn[:, 0]) <= 1e-5
    var = ((bn[:, 1] - rv0) / 0.1 + rv0) * (n - 1) / n
    assert relerr(got[:, 1], rv0 + 0.1 * (var - rv0)) <= 1e-5
    assert relerr(got[:, 1], bn[:, 1]) > 1e-3, "the biased and the unbiased running variance differ (n = 4 on the top level)"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: one rank per device over RCCL (a one-GPU test box skips it)")
def test_syncbn_two_ranks_equal_one_rank_bn_over_the_whole_batch():
    """"SyncBN" on two ranks with half the batch each against one-rank "BN" on the whole batch: head outputs, input and parameter
    gradients, and the biased running variance.  Bounds: the moments and sums are exact fp64 sums on both sides, what remains is the
    fp32 convs' summation order (1e-5 on outputs, 1e-4 on the weight gradients' split reductions over another batch size)."""
    _two_rank_syncbn("nccl")


def test_syncbn_two_ranks_on_one_gpu_over_gloo():
    """the same comparison with both ranks on ONE device over gloo (as tests/test_dp_gpu.py runs its two ranks): the W > 1 branches of
    ops.BatchNormReLU run on every test box"""
    _two_rank_syncbn("gloo")


def test_syncbn_trainer_two_ranks_stay_in_lock_step():
    """a whole data-parallel step under "SyncBN" (two ranks on one GPU over gloo): the student passes stay unfused, the BatchNorm
    all-reduces interleave with the overlapped gradient buckets in one order on both ranks, the replicas end bit-identical and finite"""
    from tests import test_dp_gpu as D
    a = _run_sync_trainer(D)
    assert a[0][0] == a[1][0] and a[0][1] == a[1][1]
    assert a[0][0][1] and a[0][1][1]


def _sync_trainer_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "unbiased-teacher-v2_amd"))
    from tests import utv2_testutil as U
    base = U.small_fcos_cfg

    def cfg(bl=2, bu=2, device="cuda"):
        c = base(bl, bu, device)
        c.defrost() if hasattr(c, "defrost") else None
        c.MODEL.FCOS.NORM = "SyncBN"
        return c
    U.small_fcos_cfg = cfg
    from tests import test_dp_gpu as D
    D._worker(rank, world, port, True, q)


def _run_sync_trainer(D):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = D._free_port()
    procs = [ctx.Process(target=_sync_trainer_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r, s, t, _l = q.get(timeout=300)
        res[r] = (s, t)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res
