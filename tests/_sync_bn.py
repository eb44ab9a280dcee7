"""Synchronised BatchNorm, stated in numpy: what crosses the replicas and what every replica makes of it (csrc/grad_dev.h,
include/hep.h "Synchronised BatchNorm").  float64 throughout; a shard is the rows [R_r][C] one replica holds.

  forward    per shard    S_r = sum z, Q_r = sum z^2 (over its rows), R_r
             exchanged    S = sum_r S_r, Q = sum_r Q_r, N = sum_r R_r
             everywhere   mean = S / N, var = max((Q - mean S) / N, 0), a = (z - mean) / sqrt(var + eps) gamma + beta;
                          running_mean <- (1 - m) running_mean + m mean, running_var <- (1 - m) running_var + m var N / (N - 1)
  backward   per shard    dgamma_r = sum d a x^, dbeta_r = sum d a   (this replica's parameter gradients: their SUM is the global one)
             exchanged    DG = sum_r dgamma_r, DB = sum_r dbeta_r, N
             everywhere   d z = gamma rstd (d a - (DB + x^ DG) / N)
"""
import numpy as np

MOMENTUM, EPS = 0.01, 1e-3


def shard_sums(z):
    """(S_r [C], Q_r [C], R_r) of one shard's rows z [R_r][C]."""
    z = np.asarray(z, np.float64)
    return z.sum(0), (z * z).sum(0), float(z.shape[0])


def exchange(blocks):
    """The hook: element-wise sums over the replicas' blocks (tuples of arrays / scalars)."""
    return tuple(sum(parts) for parts in zip(*blocks))


def statistics(S, Q, N, running_mean, running_var, momentum=MOMENTUM):
    """(mean, biased var, new running_mean, new running_var) from the global sums."""
    mean = S / N
    var = np.maximum((Q - mean * S) / N, 0.0)
    return mean, var, (1.0 - momentum) * running_mean + momentum * mean, (1.0 - momentum) * running_var + momentum * (var * N / (N - 1.0))


def apply(z, mean, var, gamma, beta, eps=EPS):
    """(a, x^, rstd) of one shard."""
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (np.asarray(z, np.float64) - mean) * rstd
    return xh * gamma + beta, xh, rstd


def shard_dsums(da, xh):
    """(dgamma_r [C], dbeta_r [C], R_r) of one shard."""
    return (da * xh).sum(0), da.sum(0), float(da.shape[0])


def dz(da, xh, gamma, rstd, DG, DB, N):
    """The input gradient of one shard from the global sums."""
    return gamma * rstd * (da - (DB + xh * DG) / N)


def forward_backward(shards_z, shards_da, gamma, beta, running_mean, running_var):
    """The whole exchange over a list of shards: dict(a [per shard], dz [per shard], dgamma / dbeta (the SUM of the shards' own),
    running_mean, running_var, N)."""
    S, Q, N = exchange([shard_sums(z) for z in shards_z])
    mean, var, rm, rv = statistics(S, Q, N, running_mean, running_var)
    fwd = [apply(z, mean, var, gamma, beta) for z in shards_z]
    local = [shard_dsums(da, xh) for da, (_a, xh, _r) in zip(shards_da, fwd)]
    DG, DB, N2 = exchange(local)
    assert N2 == N
    return dict(a=[f[0] for f in fwd], dz=[dz(da, xh, gamma, rstd, DG, DB, N) for da, (_a, xh, rstd) in zip(shards_da, fwd)],
                dgamma=DG, dbeta=DB, local=local, running_mean=rm, running_var=rv, N=N)
