"""Tree-constrained decoding on the host: evaluation.tree_decode_arrays (the
host form of ggnn_tree_decode, Chu-Liu/Edmonds) against brute force over all
head vectors, the planted cycle cases, tree_scores, the counts recount, the
model's tree= keywords on a CPU device and the C ABI's validation without a
GPU.  Exact integer equality only.  The case builders are shared with
tests/test_gpu_tree_decode.py."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from decode_cases import _synthetic_raw
from ggnn_amd import evaluation as E
from ggnn_amd.model import DenseGGNNChemModel

F = E.TREE_FORBIDDEN


# ------------------------------------------------------------ case builders
def finish(s):
    """Row 0 and the diagonal of one graph's [n, n] scores are no arcs."""
    s = np.array(s, np.int32)
    s[0, :] = F
    s[np.arange(s.shape[0]), np.arange(s.shape[0])] = F
    return s


def chain(n):
    """Word i's best head is i - 1 (a tree with one ROOT child), every other arc 0."""
    s = np.zeros((n, n), np.int32)
    for i in range(1, n):
        s[i, i - 1] = 6
    return s


def two_cycle(n):
    s = chain(n)
    s[1, 2] = s[2, 1] = 8
    return finish(s)


def full_cycle(n):
    """One cycle through all words, every ROOT arc worse than any other arc."""
    s = np.zeros((n, n), np.int32)
    s[:, 0] = -5
    for i in range(1, n):
        s[i, i + 1 if i + 1 < n else 1] = 8
    return finish(s)


def nested_cycle(n):
    """Words 1 and 2 pick each other; contracted, their best arc comes from
    word 3, whose best head is word 1: a second cycle, of a supernode and a
    word.  Word 4 hangs off ROOT and the rest is a chain."""
    assert n >= 5
    s = chain(n)
    s[1:5, :] = 0
    s[1, 2] = s[2, 1] = 10
    s[3, 1] = 9
    s[1, 3] = 8
    s[2, 3] = 1
    s[4, 0] = 5
    s[1, 4] = s[2, 4] = 2
    s[3, 4] = 1
    return finish(s)


def no_root_child(n):
    """The arg-max is a cycle 1 -> n-1 -> n-2 -> ... -> 1; the ROOT arcs are second best."""
    s = chain(n)
    s[:, 0] = 5
    s[1, n - 1] = 8
    return finish(s)


def three_roots(n):
    assert n >= 4
    s = chain(n)
    s[1:4, 0] = 8
    return finish(s)


def forbidden_row(n):
    s = finish(chain(n))
    s[min(3, n - 1), :] = F
    return s


def closed_group(n):
    """Words 1 and 2 may only take each other: no empty row, yet no tree."""
    assert n >= 3
    s = finish(chain(n))
    s[1:3, :] = F
    s[1, 2] = s[2, 1] = 4
    return s


def all_ties(n):
    return finish(np.zeros((n, n), np.int32))


PLANTED = [two_cycle, full_cycle, nested_cycle, no_root_child, three_roots, forbidden_row, closed_group, all_ties]
INFEASIBLE = (forbidden_row, closed_group)


def argmax_pred(scores, n_nodes, rng=None):
    """pred [b, v, 2] as ggnn_heads_decode leaves it: the first maximum of the
    allowed scores of every word row (-1 if it has none), labels from rng (0
    without), row 0 and rows >= n at -1."""
    s = np.asarray(scores)
    b, v, o = s.shape
    pred = np.full((b, v, 2), -1, np.int32)
    for g in range(b):
        n = int(n_nodes[g])
        for i in range(1, n):
            row = s[g, i, :n].astype(np.int64)
            row[i] = F
            if (row != F).any():
                pred[g, i, 0] = int(np.argmax(np.where(row == F, -2 ** 40, row)))
            pred[g, i, 1] = 0 if rng is None else int(rng.integers(0, 12))
    return pred


def brute_force(s, n, single_root):
    """The best total over all n^(n-1) head vectors that are trees (None: no tree)."""
    best = None
    for hv in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hv)
        if E.is_tree(h, n, single_root, s):
            t = E.tree_total(s, h, n)
            best = t if best is None or t > best else best
    return best


def check_against_brute_force(s, n, single_root):
    """One graph through tree_decode_arrays: the three status rules, a tree on
    status 1 with the brute-force total, the input back otherwise."""
    pred = argmax_pred(s[None], [n])
    before = pred.copy()
    levels = []
    out, counts, status = E.tree_decode_arrays(s[None], [n], pred, single_root, levels=levels)
    assert counts is None and np.array_equal(pred, before)            # the input is not touched
    best = brute_force(s, n, single_root)
    was_tree = E.is_tree(before[0, :, 0], n, single_root, s)
    expect = 0 if was_tree else (2 if best is None else 1)
    assert status.tolist() == [expect], (status, expect, s)
    if expect == 1:
        assert E.is_tree(out[0, :, 0], n, single_root, s)
        assert E.tree_total(s, out[0, :, 0], n) == best
        assert np.array_equal(out[0, :, 1], before[0, :, 1]) and out[0, 0, 0] == -1
    else:
        assert np.array_equal(out, before)
        assert levels[0] == 0 or expect == 2
    return expect, levels[0]


# ------------------------------------------------------------------ the tests
def test_random_cases_equal_brute_force():
    rng = np.random.default_rng(20)
    seen = {0: 0, 1: 0, 2: 0}
    deepest = 0
    for case in range(360):
        n = 2 + case % 5                                              # every n in 2..6
        s = rng.integers(-8, 9, (n, n)).astype(np.int32)
        if case % 3 == 0:
            s[rng.random((n, n)) < 0.3] = F
        status, levels = check_against_brute_force(finish(s), n, bool((case // 5) & 1))
        seen[status] += 1
        deepest = max(deepest, levels)
    assert seen[0] >= 30 and seen[1] >= 100 and seen[2] >= 10, seen
    assert deepest >= 2


@pytest.mark.parametrize("single_root", [False, True])
@pytest.mark.parametrize("build", PLANTED, ids=lambda f: f.__name__)
def test_planted_cases(build, single_root):
    for n in (5, 6):
        s = build(n)
        status, levels = check_against_brute_force(s, n, single_root)
        if build in INFEASIBLE:
            assert status == 2
        elif build is three_roots:
            assert status == (1 if single_root else 0)
        elif build is all_ties:
            assert status == (1 if single_root else 0)               # every word's first maximum is ROOT
        else:
            assert status == 1
        if build is nested_cycle:
            assert levels >= 2
    if build is three_roots:
        s = build(6)
        out, _, _ = E.tree_decode_arrays(s[None], [6], argmax_pred(s[None], [6]), single_root)
        assert (out[0, 1:, 0] == 0).sum() == (1 if single_root else 3)


def test_n_below_two_and_n_two():
    s = finish(np.zeros((2, 2), np.int32))
    for single_root in (False, True):
        check_against_brute_force(s, 2, single_root)
        pred = np.full((3, 2, 2), 7, np.int32)
        out, _, status = E.tree_decode_arrays(np.stack([s, s, s]), [0, 1, 2], pred, single_root)
        assert status.tolist() == [0, 0, 1] and out[2, 1, 0] == 0     # head 7 is no arc: repaired
        assert np.array_equal(out[:2], pred[:2]) and out[2, 0, 0] == 7 and out[2, 1, 1] == 7
    blocked = s.copy()
    blocked[1, 0] = F
    assert check_against_brute_force(blocked, 2, True)[0] == 2


def test_rows_and_columns_past_n_are_ignored():
    rng = np.random.default_rng(5)
    b, v, o, n = 1, 7, 9, 5
    s = np.full((b, v, o), 1000, np.int32)
    s[0, :n, :n] = nested_cycle(n)
    pred = argmax_pred(s, [n], rng)
    pred[0, n:, :] = 3                                                # must come back untouched
    out, _, status = E.tree_decode_arrays(s, [n], pred, True)
    assert status.tolist() == [1] and np.array_equal(out[0, n:], pred[0, n:])
    assert E.tree_total(s[0], out[0, :, 0], n) == brute_force(nested_cycle(n), n, True)


def test_tree_scores():
    assert [E.tree_score_shift(v) for v in (4, 40, 198, 256)] == [16, 12, 7, 6]
    for v in (4, 40, 198, 256):                                       # the exactness contract of ggnn_tree_decode
        k = E.tree_score_shift(v)
        assert 150 * 2 ** k * v * (v + 1) <= 2 ** 30 and (k == 16 or 150 * 2 ** (k + 1) * v * (v + 1) > 2 ** 30)
    v, o = 6, 9
    k = E.tree_score_shift(v)
    p = np.full((2, v, o), 0.25, np.float32)
    denormal = np.float32(2.0 ** -149)
    p[0, 1, 2], p[0, 1, 3], p[0, 1, 4], p[0, 2, 1], p[0, 2, 3], p[0, 2, 4] = 0, np.nan, np.inf, denormal, 1, -np.inf
    p[0, 3, 1] = -0.5
    n = [6, 3]
    q = E.tree_scores(p, n, v)
    assert q.dtype == np.int32 and q.shape == p.shape
    assert (q[0, 1, 2:5] == F).all() and q[0, 2, 4] == F and q[0, 3, 1] == F
    assert q[0, 2, 1] == -149 * 2 ** k and q[0, 2, 3] == 0 and q[0, 1, 0] == -2 * 2 ** k
    assert q.min(initial=0, where=q != F) >= -150 * 2 ** k           # the clamp's floor is never passed
    for g in range(2):
        for i in range(v):
            for j in range(o):
                dead = i == 0 or i == j or i >= n[g] or j >= n[g]
                assert (q[g, i, j] == F) == (dead or not (np.isfinite(p[g, i, j]) and p[g, i, j] > 0))
    # rint of log2(p) * 2^k
    x = np.float32(0.3)
    p[:] = x
    assert E.tree_scores(p, n, v)[0, 1, 0] == int(np.rint(np.log2(np.float64(x)) * 2 ** k))
    # the torch form (the GPU path's plumbing) gives the same integers
    from ggnn_amd.heads import tree_scores, tree_score_shift
    rng = np.random.default_rng(0)
    p = rng.random((3, v, o)).astype(np.float32)
    p[1, 2, 0], p[2, 1, 3], p[0, 4, 4], p[0, 2, 1] = 0, np.nan, np.inf, denormal
    assert np.array_equal(tree_scores(torch.from_numpy(p), torch.tensor([6, 4, 2]), v).numpy(),
                          E.tree_scores(p, [6, 4, 2], v))
    assert [tree_score_shift(u) for u in (4, 40, 198, 256)] == [16, 12, 7, 6]


def test_counts_are_recounted_for_repaired_graphs_only():
    rng = np.random.default_rng(9)
    builds = [two_cycle, chain, closed_group, nested_cycle]
    b, v, o = len(builds), 8, 8
    n = [8, 7, 6, 8]
    s = np.full((b, v, o), 50, np.int32)
    for g, f in enumerate(builds):
        s[g, :n[g], :n[g]] = finish(f(n[g]))
    pred = argmax_pred(s, n, rng)
    gold = np.full((b, v, 2), -1, np.int32)
    for g in range(b):
        for i in range(1, n[g]):
            if i != 4:                                                # a row without gold is not counted
                gold[g, i] = (i - 1 if rng.random() < 0.7 else 0, pred[g, i, 1] if rng.random() < 0.6 else 13)
    counts = rng.integers(20, 30, (b, 5)).astype(np.int32)
    out, c, status = E.tree_decode_arrays(s, n, pred, True, gold, counts)
    assert status.tolist() == [1, 0, 2, 1]
    for g in range(b):
        if status[g] != 1:
            assert np.array_equal(c[g], counts[g]) and np.array_equal(out[g], pred[g])
            continue
        has = gold[g, 1:, 0] >= 0
        uas = sum(1 for i in range(1, v) if gold[g, i, 0] >= 0 and out[g, i, 0] == gold[g, i, 0])
        las = sum(1 for i in range(1, v) if gold[g, i, 0] >= 0 and (out[g, i] == gold[g, i]).all())
        assert c[g].tolist() == [counts[g, 0], las, uas, counts[g, 3], counts[g, 4]] and has.sum() == n[g] - 2
    with pytest.raises(ValueError):
        E.tree_decode_arrays(s, n, pred, True, gold, None)
    with pytest.raises(ValueError):
        E.tree_decode_arrays(s[:, :, :7], n, pred, True)


# ------------------------------------------------------------- the CPU model
def _synthetic_model():
    """tests/test_gpu_decode.py::_synthetic_model on a CPU device, its forward a
    numpy stand-in seeded by the staged batch (as tests/test_decode.py does)."""
    m = DenseGGNNChemModel(params={"hidden_size": 64, "num_timesteps": 2, "batch_size": 5,
                                   "compact_adjacency": True, "hip_graphs": False},
                           num_edge_types=6, output_size_edges=12, pos_size=46, vocab_size=200, max_nodes=40,
                           seed=0, embedding_sizes=dict(loc=16, pos=8, word=24, edge=16), device="cpu")

    def build_loss(task_id=0):
        ph = m.placeholders
        b, v = int(ph["num_graphs"]), int(ph["num_vertices"])
        o, oe = m.params["output_size"], m.output_size_edges
        wi = np.asarray(ph["word_inputs"]).astype(np.int64)
        rng = np.random.default_rng(int((wi * np.arange(1, wi.size + 1).reshape(wi.shape)).sum()) % (2 ** 31))
        cv = np.round(rng.random((b, v * o)) * 0.98 + 0.01, 2).astype(np.float32)
        peaked = rng.random(b) < 0.4                                  # some graphs with a tree as arg-max
        for g in np.flatnonzero(peaked):
            t = cv[g].reshape(v, o)
            for i in range(1, v):
                t[i, i - 1] = 1.0
        cv_e = np.round(rng.random((b, v * oe)) * 0.98 + 0.01, 2).astype(np.float32)
        m.ops["computed_values"] = torch.from_numpy(cv)
        m.ops["computed_values_edges"] = torch.from_numpy(cv_e)
        m.ops["loss"] = torch.tensor(float(cv.sum() + cv_e.sum()) / (b * v))
        return m.ops["loss"]
    m.build_loss = build_loss
    return m


def check_tree_predictions(m, feed, staged_scores):
    """predict_batch(tree=True) of a feed against predict_batch(): the three
    properties of the issue.  staged_scores(m, n_nodes, v) -> int32 [b, v, o]
    numpy scores of the batch the model holds.  Returns the status counts."""
    plain = m.predict_batch(dict(feed))
    p = m.predict_batch(dict(feed), tree=True)
    b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
    assert plain["tree_status"] is None
    status = p["tree_status"]
    assert status.shape == (b,) and status.dtype == np.int32
    assert np.array_equal(p["labels"], plain["labels"]) and np.array_equal(p["n_nodes"], plain["n_nodes"])
    s = staged_scores(m, p["n_nodes"], v)
    for g in range(b):
        n = int(p["n_nodes"][g])
        was_tree = E.is_tree(plain["heads"][g], n, True, s[g])
        if status[g] == 2:
            assert np.array_equal(p["heads"][g], plain["heads"][g])
            continue
        assert E.is_tree(p["heads"][g], n, True, s[g]) and (p["heads"][g, n:] == -1).all()
        assert (status[g] == 0) == was_tree
        if was_tree:
            assert np.array_equal(p["heads"][g], plain["heads"][g])
        else:
            pred = np.stack([plain["heads"][g], plain["labels"][g]], axis=1)[None]
            host, _, st = E.tree_decode_arrays(s[g][None], [n], pred, True)
            assert st[0] == 1
            assert E.tree_total(s[g], p["heads"][g], n) == E.tree_total(s[g], host[0, :, 0], n)
    return [int((status == k).sum()) for k in (0, 1, 2)]


def _host_scores(m, n_nodes, v):
    b, o = len(n_nodes), m.params["output_size"]
    return E.tree_scores(m.ops["computed_values"].numpy().reshape(b, v, o), n_nodes, v)


def test_model_tree_keywords_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    data = m.process_raw_graphs(raw, False)
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        seen += check_tree_predictions(m, feed, _host_scores)
    assert seen[0] > 0 and seen[1] > 0, seen
    plain, parsed = m.parse(raw), m.parse(raw, tree=True)
    changed = 0
    for d, a, t in zip(raw, plain, parsed):
        n = len(d["node_features"])
        assert len(t) == n - 1 and [x[1] for x in t] == [x[1] for x in a]
        assert E.is_tree([-1] + [x[0] for x in t], n, True)
        changed += a != t
    assert changed == seen[1]
    multi = m.parse(raw, tree=True, single_root=False)
    assert all(E.is_tree([-1] + [x[0] for x in t], len(d["node_features"]), False) for d, t in zip(raw, multi))
    # evaluate_batch / score_epoch: the scores of predict_batch(tree=True)'s heads
    with pytest.raises(ValueError):
        m.evaluate_batch(next(iter(m.make_minibatch_iterator(data, False))), tree=True)
    graphs, las, uas = 0, 0.0, 0.0
    for feed in m.make_minibatch_iterator(data, False):
        got = m.evaluate_batch(dict(feed), on_device=True, tree=True)
        r = m._decode_forward(dict(feed), True, True, True)
        p = m.predict_batch(dict(feed), tree=True)
        assert np.array_equal(r["pred"][:, :, 0], p["heads"])
        per_graph = [E.graph_scores_from_lists(r["pred"][g], r["gold"][g]) for g in range(r["b"])]
        assert got == tuple(sum(x[c] for x in per_graph) / r["b"] for c in range(3))
        graphs += r["b"]
        las += got[0] * r["b"]
        uas += got[1] * r["b"]
    ref = m.score_epoch(data)
    assert m.decode_stats["repaired_graphs"] == 0 and m.decode_stats["infeasible_graphs"] == 0
    got = m.score_epoch(data, tree=True)
    assert m.decode_stats["repaired_graphs"] == seen[1] and m.decode_stats["infeasible_graphs"] == seen[2]
    assert got[0] == ref[0] and got[3] == ref[3] and got[5] == ref[5]
    assert got[1:3] == (las / graphs, uas / graphs)          # (_epoch's order of additions)
    assert m.score_epoch(data)[:4] == ref[:4]


# ------------------------------------------------------------------- the ABI
def test_tree_decode_rejects_bad_arguments_without_gpu(lib):
    """ggnn_tree_decode validates on the host before any launch."""
    from ggnn_amd import _lib
    P = ctypes.c_void_p
    x = P(256)                                        # never dereferenced: every call below fails validation
    ok = dict(b=2, v=30, o=150, s=x, n=x, single=1, pred=x, gold=None, counts=None, status=x)
    for change, word in ((dict(o=0), b"1..1024"), (dict(o=1025), b"1..1024"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(b=0), b">= 1"), (dict(s=None), b"NULL"),
                         (dict(n=None), b"NULL"), (dict(pred=None), b"NULL"), (dict(status=None), b"NULL"),
                         (dict(gold=x), b"together"), (dict(counts=x), b"together"), (dict(single=2), b"0 or 1")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_tree_decode(ctypes.byref(d), a["s"], a["o"], a["n"], a["single"], a["pred"], a["gold"],
                                  a["counts"], a["status"], None, 0, None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
    assert lib.ggnn_tree_decode(None, x, 150, x, 1, x, None, None, x, None, 0, None) == -1
    assert lib.ggnn_tree_decode_workspace_bytes(256, 256) >= 0
    assert {"ggnn_tree_decode", "ggnn_tree_decode_workspace_bytes"} <= set(_lib.EXPORTED)
    assert _lib.TREE_MAXV == E.TREE_MAXV == 256 and _lib.TREE_FORBIDDEN == F == -2 ** 31
