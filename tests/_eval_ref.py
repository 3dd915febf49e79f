"""The numpy fp64 reference of ``ddpx.ops.head.eval_metrics`` and the logits its tests share."""
import numpy as np


def ref_metrics(z, t, k, m_valid=None):
    """(loss_sum, top-1 hits, top-k hits, rows, ranks) of the rows ``m < m_valid`` of ``z`` [M, C] against ``t`` [M],
    in fp64, with rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}.  A target outside [0, C) is a miss with no loss
    (rank -1 in the returned array)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    M, C = z.shape
    mv = M if m_valid is None else m_valid
    loss, h1, hk = 0.0, 0, 0
    ranks = np.full(mv, -1, dtype=np.int64)
    for m in range(mv):
        tm = int(t[m])
        if not 0 <= tm < C:
            continue
        row = z[m]
        zt = row[tm]
        r = int((row > zt).sum() + (row[:tm] == zt).sum())
        mx = row.max()
        loss += mx + np.log(np.exp(row - mx).sum()) - zt
        h1 += r == 0
        hk += r < k
        ranks[m] = r
    return loss, h1, hk, mv, ranks


def gaussian_logits(M, C, seed):
    """fp32 Gaussian logits scaled so that max |z| = 8, and uniform targets."""
    g = np.random.default_rng(seed)
    z = g.standard_normal((M, C))
    z = (z * (8.0 / np.abs(z).max())).astype(np.float32)
    return z, g.integers(0, C, size=M).astype(np.int64)


def grid_logits(M, C, seed):
    """fp32 logits from a four-value grid: most rows have ties, also with the target's logit."""
    g = np.random.default_rng(seed)
    z = g.choice(np.array([-1.5, 0.0, 0.25, 2.0], dtype=np.float32), size=(M, C))
    return z, g.integers(0, C, size=M).astype(np.int64)


def ties_at_k(z, t, k):
    """Rows where the tie rule decides the top-k hit: the target's rank is < k only because tied classes above it
    in index do not count, or >= k only because tied classes below it do."""
    z = np.asarray(z, dtype=np.float64)
    n = 0
    for m in range(z.shape[0]):
        tm = int(t[m])
        if not 0 <= tm < z.shape[1]:
            continue
        greater = int((z[m] > z[m, tm]).sum())
        tied = int((z[m] == z[m, tm]).sum()) - 1
        n += tied > 0 and greater < k <= greater + tied
    return n
