"""TEST.PRECISE_BN restated in numpy float64, from the rules alone (DESIGN.md "TEST.PRECISE_BN"); shares no code with the package.

Estimator, per BatchNorm module (a level of a layer) and channel: for every forward call with batch size B, batch mean m and unbiased
batch variance v
    num += B;  q = m*m + v*(B-1)/B;  pop_mean += (m - pop_mean) * B/num;  pop_sq += (q - pop_sq) * B/num
and at the end running_mean = pop_mean, running_var = pop_sq - pop_mean^2, each rounded once to fp32.
Hook schedule: after iteration `it` the hook runs when it + 1 == max_iter, or eval_period > 0 and (it + 1) % eval_period == 0."""
import numpy as np


def estimate(nlevels, C, sets):
    """sets: iterable of (level, batch mean [C], unbiased batch variance [C], B) in the order the forward calls produce them
    -> dict(pop_mean, pop_sq [nlevels, C] fp64; num [nlevels]; running_mean, running_var fp64; and their fp32 roundings *_f32)"""
    pop_mean = np.zeros((nlevels, C), dtype=np.float64)
    pop_sq = np.zeros((nlevels, C), dtype=np.float64)
    num = np.zeros(nlevels, dtype=np.float64)
    for level, m, v, B in sets:
        m, v, B = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64), np.float64(B)
        num[level] = num[level] + B
        q = m * m + v * (B - 1.0) / B
        pop_mean[level] = pop_mean[level] + (m - pop_mean[level]) * B / num[level]
        pop_sq[level] = pop_sq[level] + (q - pop_sq[level]) * B / num[level]
    var = pop_sq - pop_mean ** 2
    return dict(pop_mean=pop_mean, pop_sq=pop_sq, num=num, running_mean=pop_mean, running_var=var,
                running_mean_f32=pop_mean.astype(np.float32), running_var_f32=var.astype(np.float32))


def moments_to_batch_stats(mean, meansq, n):
    """[mean, mean of squares] over n values -> (batch mean, unbiased batch variance): var = max(meansq - mean^2, 0) * n / (n - 1)"""
    mean, meansq = np.asarray(mean, dtype=np.float64), np.asarray(meansq, dtype=np.float64)
    var = np.maximum(meansq - mean * mean, 0.0)
    return mean, var * (np.float64(n) / (np.float64(n) - 1.0))


def fires_after(max_iter, eval_period, start_iter=0):
    """the iterations after which the hook runs"""
    return [it for it in range(start_iter, max_iter) if it + 1 == max_iter or (eval_period > 0 and (it + 1) % eval_period == 0)]
