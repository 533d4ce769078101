"""BatchNorm2d + ReLU over statistic sets of a level-first [P, C] matrix, restated on torch's own batch norm (CPU): the float64 reference
of tests/test_bn_tower_kernels_gpu.py, and - run in float32 - the yardstick its fp32 tolerances are taken from.

A statistic set (row0, rows, level) is one call of the BatchNorm2d module of FPN level `level` on rows [row0, row0 + rows): the sets are
processed in order, so two sets of one level update that level's running statistics one after the other."""
import torch

EPS, MOMENTUM = 1e-5, 0.1


def bn_relu(x, gamma, beta, running_mean, running_var, sets, training=True, dy=None, dtype=torch.float64, biased_running=False):
    """x [P, C], gamma / beta / running_* [L, C] (any float dtype; computed in `dtype`).  Returns a dict of `dtype` CPU tensors: y [P, C],
    mean / rstd [S, C] (training: the batch statistics; eval: from the running ones), running_mean / running_var [L, C] after the calls,
    and with dy: dx [P, C], dgamma / dbeta [L, C].  biased_running: the running variance takes the biased batch variance (the SyncBN rule)."""
    x = x.detach().cpu().to(dtype).requires_grad_(dy is not None)
    ga = gamma.detach().cpu().to(dtype).clone().requires_grad_(dy is not None)
    be = beta.detach().cpu().to(dtype).clone().requires_grad_(dy is not None)
    rm, rv = running_mean.detach().cpu().to(dtype).clone(), running_var.detach().cpu().to(dtype).clone()
    y = torch.zeros_like(x)
    ys, means, rstds = [], [], []
    for r0, n, l in sets:
        xs = x[r0:r0 + n].t().unsqueeze(0)          # [1, C, n]: one call of level l's module
        rm_l, rv_l = rm[l].clone(), rv[l].clone()
        out, m, r = torch.native_batch_norm(xs, ga[l], be[l], rm_l, rv_l, training, MOMENTUM, EPS)
        if training:
            if biased_running:
                rv_l = rv[l] + MOMENTUM * (xs.detach().var(dim=(0, 2), unbiased=False) - rv[l])
            rm[l], rv[l] = rm_l, rv_l
        else:
            m, r = rm[l].clone(), 1.0 / torch.sqrt(rv[l] + EPS)
        ys.append((r0, n, torch.relu(out.squeeze(0).t())))
        means.append(m.detach())
        rstds.append(r.detach())
    res = dict(mean=torch.stack(means), rstd=torch.stack(rstds), running_mean=rm, running_var=rv)
    if dy is not None:
        dyd = dy.detach().cpu().to(dtype)
        sum(((yy * dyd[r0:r0 + n]).sum() for r0, n, yy in ys)).backward()
        res.update(dx=x.grad, dgamma=ga.grad, dbeta=be.grad)
    for r0, n, yy in ys:
        y[r0:r0 + n] = yy.detach()
    res["y"] = y.detach()
    return res


def ulp32(mag):
    """the fp32 unit in the last place at magnitude `mag` (a float)"""
    import math
    return 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 2.0 ** -149


def ulp_steps16(a, b):
    """distance of two 16-bit float tensors of one dtype in representable values (elementwise, int32)"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()
