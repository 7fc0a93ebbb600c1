"""numpy restatement of the multi-neighbour plane sweep of the SGM front end
(include/smvs_hip.h, "Multi-neighbour plane sweep"): the fold of the n
neighbours' cost bytes into one volume, and the support of a winner plane among
the neighbours.  Integers only; no project imports."""
import numpy as np

NO_COST = 255


def fold_parts(costs, min_views, best_k):
    """The fold with its intermediates.  costs (n, ...) of cost bytes (any
    integer type, values 0 .. 255; 255: no cost).  Returns dict(C, m, k_eff, S):
    C the folded bytes (u8), m the number of costs per cell, k_eff the number
    averaged (0 where C is 255 by min_views), S their sum."""
    c = np.asarray(costs).astype(np.int64)
    n = c.shape[0]
    if not (1 <= min_views <= n and 0 <= best_k):
        raise ValueError("min_views in 1 .. n, best_k >= 0")
    valid = c != NO_COST
    m = valid.sum(axis=0)
    k_eff = m if best_k == 0 else np.minimum(best_k, m)
    # ascending; 255 is above every cost, so the costs come first
    ordered = np.sort(c, axis=0)
    rank = np.arange(n).reshape((n,) + (1,) * (c.ndim - 1))
    S = np.where(rank < k_eff[None], ordered, 0).sum(axis=0)
    kept = m >= min_views
    k_safe = np.maximum(k_eff, 1)
    C = np.where(kept, (2 * S + k_safe) // (2 * k_safe), NO_COST)
    return dict(C=C.astype(np.uint8), m=m, k_eff=np.where(kept, k_eff, 0), S=np.where(kept, S, 0))


def fold(costs, min_views, best_k):
    """C of the definition: per cell 255 with fewer than min_views costs, else
    the mean, rounded half up, of the best_k smallest costs (of all: best_k 0, or
    fewer than best_k costs)."""
    return fold_parts(costs, min_views, best_k)["C"]


def support(costs, argmin, support_cost):
    """Per pixel the number of neighbours whose own cost at the winner plane is
    at most support_cost (u8).  costs (n, h, w, D), argmin (h, w)."""
    c = np.asarray(costs)
    idx = np.asarray(argmin).astype(np.int64)[None, :, :, None]
    at = np.take_along_axis(c, np.broadcast_to(idx, c.shape[:3] + (1,)), axis=3)[..., 0]
    return (at.astype(np.int64) <= support_cost).sum(axis=0).astype(np.uint8)


def apply_support(depth, sup, min_support):
    """The depth map with the support test: 0 where min_support > 0 and the
    support is below it."""
    out = np.array(depth, copy=True)
    if min_support > 0:
        out[sup < min_support] = 0
    return out
