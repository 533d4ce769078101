"""TEST.PRECISE_BN for the BatchNorm FCOS towers (MODEL.FCOS.NORM "BN" / "SyncBN"): before every evaluation and checkpoint the student's
running statistics are replaced by population statistics estimated from TEST.PRECISE_BN.NUM_ITER training batches.

What the reference does (engine/trainer.py:503-521 and :974-992): Detectron2's hooks.PreciseBN in front of the checkpointer when the key
is on and get_bn_modules(model) is not empty; the arithmetic is fvcore's update_bn_stats.  Neither package is part of this one, so
the rules are restated here and in DESIGN.md ("TEST.PRECISE_BN"):

[D2-recall] the hook
  * built only when TEST.PRECISE_BN.ENABLED and the model has BatchNorm layers in training mode (here: the BN / SyncBN towers; GN,
    "none" and every Faster-RCNN model have none - their BatchNorm is frozen);
  * after iteration `it` it runs when it + 1 == max_iter, or TEST.EVAL_PERIOD > 0 and (it + 1) % TEST.EVAL_PERIOD == 0;
  * it draws from a train loader of its own whose iterator lives across updates; the training loader is not advanced;
  * it updates the student only.
[fvcore-recall] update_bn_stats, per BatchNorm module (here: per level of a layer) and channel, all in fp64
  * per forward call with batch size B, batch mean m, unbiased batch variance v:
        num += B;  q = m * m + v * (B - 1) / B;  pop_mean += (m - pop_mean) * B / num;  pop_sq += (q - pop_sq) * B / num
  * after num_iters iterations running_mean = pop_mean, running_var = pop_sq - pop_mean^2; the running buffers are not written
    before, the layers normalise with batch statistics as in training, num_batches_tracked advances once per forward call;
  * a loader that ends early is an error.
The feed is this package's definition (the reference hands the loader's 4-tuple of lists to model(inputs), which preprocess_image
cannot index - DESIGN.md): one iteration = one 4-tuple, run through the student's backbone and towers as the calls a post-burn-in step
makes: call 1 = label_q + label_k, call 2 = unlabel_q; two statistic sets per level, in that order.

The estimator never leaves the device: FCOSHead.bn_statistics_pass runs conv, statistics, hip.bn_precise_update and the normalisation
per tower depth (no prediction convs, losses or autograd), and one hip.bn_precise_commit writes the buffers at the end.
PopulationStatistics is the same estimator on the host in numpy fp64: the form tools/bench_precise_bn.py's baseline uses."""
import logging
import time

import numpy as np
import torch

from .. import hip
from ..utils import comm


def get_bn_modules(model):
    """the BatchNorm layer objects whose statistics training moves (ops.BatchNormReLU, one per tower depth and [L, C] wide), or []"""
    head = getattr(getattr(model, "proposal_generator", None), "fcos_head", None)
    return list(getattr(head, "bn_layers", None) or [])


class PopulationStatistics:
    """[fvcore-recall] the estimator on the host, fp64: one instance per BatchNorm layer of `nlevels` levels x C channels"""

    def __init__(self, nlevels, C):
        self.pop_mean = np.zeros((nlevels, C), dtype=np.float64)
        self.pop_sq = np.zeros((nlevels, C), dtype=np.float64)
        self.num = np.zeros(nlevels, dtype=np.float64)

    def update(self, level, batch_mean, batch_var, batch_size):
        """one forward call of `batch_size` images on `level`: batch mean and UNBIASED batch variance per channel"""
        if batch_size < 1:
            raise ValueError("precise BN: a forward call of %r images" % (batch_size,))
        m, v, B = np.asarray(batch_mean, dtype=np.float64), np.asarray(batch_var, dtype=np.float64), float(batch_size)
        self.num[level] += B
        q = m * m + v * ((B - 1.0) / B)
        w = B / self.num[level]
        self.pop_mean[level] += (m - self.pop_mean[level]) * w
        self.pop_sq[level] += (q - self.pop_sq[level]) * w

    def result(self):
        """-> (running_mean, running_var) in fp64; the caller rounds once to fp32"""
        return self.pop_mean.copy(), self.pop_sq - self.pop_mean * self.pop_mean


def statistics_iteration(model, batch, state):
    """One iteration of the feed: the loader's 4-tuple through the student's backbone and towers as the two forward calls of a
    post-burn-in step.  Equal padded canvases: one batch with two statistic sets per level (as the trainer fuses its passes); otherwise
    - and under SyncBN on several ranks, whose all-reduces must come in one order on every rank - two passes."""
    label_q, label_k, unlabel_q, _ = batch
    calls = [list(label_q) + list(label_k), list(unlabel_q)]
    head = model.proposal_generator.fcos_head
    fuse = (model.padded_canvas(calls[0]) == model.padded_canvas(calls[1])
            and not (head.norm == "SyncBN" and comm.get_world_size() > 1))
    for group in ([calls] if fuse else [[c] for c in calls]):
        model.bn_statistics_pass(group, state)


@torch.no_grad()
def update_bn_stats(model, data_loader, num_iters=200):
    """Replace the running statistics of the model's BatchNorm layers by population statistics over `num_iters` batches of
    `data_loader` (an iterable of the train loader's 4-tuples).  Everything but those buffers and num_batches_tracked is left as it
    was.  Raises when the loader ends early.  No device-to-host read.  -> the number of BatchNorm layers updated."""
    bns = get_bn_modules(model)
    if not bns:
        return 0
    if num_iters < 1:
        raise ValueError("update_bn_stats: num_iters %r" % (num_iters,))
    L, C = bns[0].gamma.t.shape
    assert all(tuple(b.gamma.t.shape) == (L, C) for b in bns)
    state = hip.bn_precise_state(len(bns), L, C, bns[0].gamma.t.device)
    was_training = model.training
    if not was_training:
        model.train(True)
    try:
        it = iter(data_loader)
        for ind in range(num_iters):
            try:
                batch = next(it)
            except StopIteration:
                raise RuntimeError("update_bn_stats is meant to run for %d iterations, but the dataloader stops at %d iterations."
                                   % (num_iters, ind)) from None
            statistics_iteration(model, batch, state)
    finally:
        if not was_training:
            model.train(False)
    hip.bn_precise_commit(state, [b.running_mean.t for b in bns], [b.running_var.t for b in bns])
    return len(bns)


def hook_is_due(it, max_iter, eval_period):
    """[D2-recall] hooks.PreciseBN.after_step"""
    nxt = it + 1
    return nxt == max_iter or (eval_period > 0 and nxt % eval_period == 0)


class PreciseBN:
    """[D2-recall] hooks.PreciseBN.  build_loader() -> the hook's own train loader; it is built at the first update and its iterator lives
    across updates."""

    def __init__(self, period, model, build_loader, num_iter):
        self.period, self.model, self.num_iter = int(period), model, int(num_iter)
        self._build_loader = build_loader
        self._data_iter = None
        self.updates = 0

    def after_step(self, it, max_iter):
        if hook_is_due(it, max_iter, self.period):
            self.update_stats()
            return True
        return False

    def _batches(self):
        for batch in self._data_iter:      # a loader that ends makes update_bn_stats raise
            yield batch

    def update_stats(self):
        if self._data_iter is None:
            self._data_iter = iter(self._build_loader())
        logger = logging.getLogger(__name__)
        t0 = time.perf_counter()
        update_bn_stats(self.model, self._batches(), self.num_iter)
        if self.model.device.type == "cuda":
            torch.cuda.synchronize(self.model.device)      # the update's only host synchronisation: the seconds below are its wall time
        self.updates += 1
        logger.info("PreciseBN: running statistics of %d BatchNorm layers re-estimated from %d iterations in %.2f s"
                    % (len(get_bn_modules(self.model)), self.num_iter, time.perf_counter() - t0))


def build_hook(cfg, model, build_loader):
    """the hook, or None when the key is off or the model has no BatchNorm layers (NORM "GN" / "none", every Faster-RCNN model)"""
    if not cfg.TEST.PRECISE_BN.ENABLED or not get_bn_modules(model):
        return None
    return PreciseBN(cfg.TEST.EVAL_PERIOD, model, build_loader, cfg.TEST.PRECISE_BN.NUM_ITER)
