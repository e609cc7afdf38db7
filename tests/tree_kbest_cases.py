"""What tests/test_tree_kbest.py, tests/test_gpu_tree_kbest.py and
tests/test_gpu_guard_tree_kbest.py share: the score batches of the k-best
tests over all dependency trees and their cached host references
(evaluation.tree_kbest_arrays).  The arrays are read-only.

The host list does not depend on K (the list for K is a prefix of the list for
a larger K: tests/test_tree_kbest.py checks that on the host form itself), so a
launch's reference is computed once, at the largest K asked of it so far, and
cut to the K of the test."""
import functools
import itertools

import numpy as np

from ggnn_amd import evaluation as E
from projective_kbest_cases import KINDS, scores_batch, with_garbage   # noqa: F401 (re-exported)

F = E.TREE_FORBIDDEN
MAIN_NS = (1, 2, 3, 5, 23, 33, 34, 6, 4)     # v = 34; graph 7: a word without a head, graph 8: out of range
WAVE_NS = (63, 64, 65, 66)                   # v = 66: a lane owns the columns l + 64 k


@functools.lru_cache(maxsize=None)
def launch(name, kind):
    """(scores int32 [b, v, v + 3], n int32 [b]) of the launch ``name``:
    "main": n = 1, 2, 3, 5, 23, 33, 34 at v = 34, a 6-node graph whose word 3
    has no allowed head and a 4-node range-rule violator; "wave": n = 63, 64,
    65, 66 at v = 66."""
    ns = list(MAIN_NS if name == "main" else WAVE_NS)
    v = max(ns)
    s = scores_batch(ns, v, v + 3, kind, (7 if name == "main" else 11) * 100 + KINDS.index(kind))
    if name == "main":
        s[7, 3, :] = F                          # word 3 of the 6-node graph has no head
        s[8, 1, 0] = 2 ** 30 - 1                # S * (n - 1) >= 2^30
    n = np.asarray(ns, np.int32)
    s.setflags(write=False)
    n.setflags(write=False)
    return s, n


@functools.lru_cache(maxsize=None)
def _full(name, kind, single_root, K):
    s, n = launch(name, kind)
    return E.tree_kbest_arrays(s, n, K, single_root)


def reference(name, kind, single_root, K):
    """tree_kbest_arrays' four arrays of the launch at K, read-only."""
    top = 16 if name == "main" else 2
    assert K <= top
    heads, totals, count, status = _full(name, kind, bool(single_root), top)
    ref = (np.ascontiguousarray(heads[:, :K]), np.ascontiguousarray(totals[:, :K]),
           np.minimum(count, K).astype(np.int32), status.copy())
    for a in ref:
        a.setflags(write=False)
    # the batch does what it is for
    if name == "main":
        assert ref[3][0] == 0 and ref[3][7] == 2 and ref[3][8] == 2, ref[3]
        big = slice(4, 7)
    else:
        big = slice(0, 4)
    if kind == "soft":
        assert (ref[2][big] == K).all() and (ref[3][big] == 1).all(), (ref[2], ref[3])
        if name == "main":                      # 3 nodes: two single-rooted trees, three in all
            assert count[2] == (2 if single_root else 3)
    return ref


def brute_force(s, n, single_root):
    """[(total, heads)] of every dependency tree over the allowed arcs of one
    graph, n <= 6."""
    out = []
    for hs in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hs)
        if E.is_tree(h, n, single_root, s):
            out.append((E.tree_total(s, h, n), tuple(h)))
    return out
