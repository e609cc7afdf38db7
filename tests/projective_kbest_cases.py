"""What tests/test_projective_kbest.py and tests/test_gpu_projective_kbest.py
share: the score batches of the k-best tests and their cached host references
(evaluation.projective_kbest_arrays).  The arrays are read-only."""
import functools
import itertools

import numpy as np

from ggnn_amd import evaluation as E

F = E.TREE_FORBIDDEN
KINDS = ("soft", "forbid", "ties")


def scores_batch(ns, v, o, kind, seed):
    """int32 [b, v, o] for graphs of ns nodes: "soft" tree_scores of softmax
    rows; "forbid" the same with 25 % of the arcs forbidden; "ties" the same
    coarsened to a few levels (multiples of 2 bits), so that many trees share a
    total."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(len(ns), v, o)) * 2.0
    p = np.exp(z - z.max(axis=2, keepdims=True))
    p = (p / p.sum(axis=2, keepdims=True)).astype(np.float32)
    s = E.tree_scores(p, np.asarray(ns, np.int32), v)
    if kind == "ties":
        step = 2 ** (E.tree_score_shift(v) + 1)
        s = np.where(s == F, F, s // step * step).astype(np.int32)
    if kind in ("forbid", "ties"):
        s = np.where(rng.random(s.shape) < 0.25, F, s).astype(np.int32)
    return s


def with_garbage(s, ns, seed=9):
    """A copy with live garbage (any int32, forbidden or not) in the rows and
    columns >= n of every graph."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-2 ** 31, 2 ** 31, size=s.shape, dtype=np.int64).astype(np.int32)
    out = s.copy()
    for k, n in enumerate(ns):
        n = max(int(n), 0)
        out[k, n:, :] = g[k, n:, :]
        out[k, :, n:] = g[k, :, n:]
    return out


@functools.lru_cache(maxsize=None)
def launch(K, P, kind):
    """(scores, n): the graphs n = 1, 2, 3, 5, P - 1, P, P + 1 at v = P + 1 (P =
    the LDS tier's largest n at this K: both tiers in one grid), a graph with a
    word that has no allowed head and a range-rule violator."""
    ns = [1, 2, 3, 5, P - 1, P, P + 1, 6, 4]
    v = P + 1
    s = scores_batch(ns, v, v + 3, kind, 100 * K + KINDS.index(kind))
    s[7, 3, :] = F                          # word 3 of the 6-node graph has no head
    s[8, 1, 0] = 2 ** 30 - 1                # S * (n - 1) >= 2^30
    n = np.asarray(ns, np.int32)
    s.setflags(write=False)
    n.setflags(write=False)
    return s, n


@functools.lru_cache(maxsize=None)
def reference(K, P, kind, single_root):
    s, n = launch(K, P, kind)
    ref = E.projective_kbest_arrays(s, n, K, single_root)
    for a in ref:
        a.setflags(write=False)
    # the batch does what it is for: both tiers return full lists, the three special graphs their statuses
    assert ref[3][0] == 0 and ref[3][7] == 2 and ref[3][8] == 2 and (ref[2][4:7] == K).all(), (ref[2], ref[3])
    return ref


def lds_maxn(K):
    """ggnn_projective_kbest_lds_maxn's rule, restated: the largest n <= 256
    with n (n + 1) / 2 * (6 K + 2) <= 38400."""
    n = 1
    while n < E.TREE_MAXV and (n + 1) * (n + 2) // 2 * (6 * K + 2) <= 38400:
        n += 1
    return n


def brute_force(s, n, single_root):
    """[(total, heads)] of every projective tree over the allowed arcs of one
    graph, n <= 6."""
    out = []
    for hs in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hs)
        if E.is_tree(h, n, single_root, s) and E.is_projective(h, n):
            out.append((E.tree_total(s, h, n), tuple(h)))
    return out
