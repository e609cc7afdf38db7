"""Projective decoding on the host: evaluation.projective_decode_arrays (the
host form of ggnn_projective_decode, Eisner's algorithm) against brute force
over all head vectors, the planted crossing cases, the dev set's gold trees,
the MST of tree_decode_arrays, the counts recount, the model's
tree="projective" keyword on a CPU device and the C ABI's validation without
a GPU.  Exact integer equality only.  The case builders are shared with
tests/test_gpu_projective_decode.py."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from test_tree_decode import (F, _host_scores, _synthetic_model, _synthetic_raw, argmax_pred, chain, closed_group,
                              finish, forbidden_row, two_cycle)


# ------------------------------------------------------------ case builders
def crossing_heads(n):
    """1 -> 3, 2 -> 0, 3 -> 2, k -> k - 1 for k >= 4: a single-rooted tree whose
    arcs 3 -> 1 and 0 -> 2 cross."""
    assert n >= 5
    h = [-1, 3, 0, 2] + list(range(3, n - 1))
    assert E.is_tree(h, n, True) and not E.is_projective(h, n)
    return h


def crossing_tree(n, seed=0):
    """100 on the crossing tree's arcs, 0..8 elsewhere."""
    s = np.random.default_rng(900 + n + seed).integers(0, 9, (n, n)).astype(np.int32)
    for i, h in enumerate(crossing_heads(n)[1:], 1):
        s[i, h] = 100
    return finish(s)


def only_crossing_tree(n):
    """The crossing tree's arcs are the only allowed ones."""
    s = np.full((n, n), F, np.int32)
    for i, h in enumerate(crossing_heads(n)[1:], 1):
        s[i, h] = 100
    return s


def out_of_range(n):
    """One allowed score of 2^30: S * (n - 1) >= 2^30."""
    s = two_cycle(n)
    s[n - 1, 1] = 2 ** 30                                             # (words 1 and 2 still pick each other)
    return s


def brute_force_projective(s, n, single_root):
    """The best total over all n^(n-1) head vectors that are projective trees
    (None: there is none)."""
    best = None
    for hv in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hv)
        if E.is_tree(h, n, single_root, s) and E.is_projective(h, n):
            t = E.tree_total(s, h, n)
            best = t if best is None or t > best else best
    return best


def run_one(s, n, single_root, pred=None):
    pred = argmax_pred(s[None], [n]) if pred is None else pred
    before = pred.copy()
    out, counts, status = E.projective_decode_arrays(s[None], [n], pred, single_root)
    assert counts is None and np.array_equal(pred, before)            # the input is not touched
    return before, out, int(status[0])


def check_against_brute_force(s, n, single_root):
    before, out, status = run_one(s, n, single_root)
    best = brute_force_projective(s, n, single_root)
    h0 = before[0, :, 0]
    was = E.is_tree(h0, n, single_root, s) and E.is_projective(h0, n)
    expect = 0 if was else (2 if best is None else 1)
    assert status == expect, (status, expect, s)
    if expect == 1:
        assert E.is_tree(out[0, :, 0], n, single_root, s) and E.is_projective(out[0, :, 0], n)
        assert E.tree_total(s, out[0, :, 0], n) == best
        assert np.array_equal(out[0, :, 1], before[0, :, 1]) and out[0, 0, 0] == -1
    else:
        assert np.array_equal(out, before)
    return expect, best is None


# ------------------------------------------------------------------ the tests
def test_is_projective():
    assert E.is_projective([-1], 1) and E.is_projective([-1, 0], 2) and E.is_projective([-1, 2, 0], 3)
    assert E.is_projective([-1, 0, 1, 2, 3], 5) and E.is_projective([-1, 2, 0, 2, 3], 5)
    assert not E.is_projective([-1, 3, 0, 2], 4)                      # 3 -> 1 crosses 0 -> 2
    assert E.is_projective([-1, 0, 3, 0, 3], 5)                       # (2, 3) and (3, 4) share an endpoint
    assert not E.is_projective([-1, 3, 4, 0, 0], 5)                   # (1, 3) and (2, 4)
    assert not E.is_projective([-1, 2, 0, 0, 1], 5)                   # (0, 3) and (1, 4)
    assert E.is_projective([-1, 2, 0, 0, 1], 3)                       # only the first n words count
    for n in (5, 6, 9):
        assert not E.is_projective(crossing_heads(n), n)


def test_random_cases_equal_brute_force():
    rng = np.random.default_rng(21)
    seen = {0: 0, 1: 0, 2: 0}
    cases = infeasible = 0
    for case in range(340):
        n = 2 + case % 5                                              # every n in 2..6
        s = rng.integers(-8, 9, (n, n)).astype(np.int32)
        s[rng.random((n, n)) < 0.25] = F
        status, none = check_against_brute_force(finish(s), n, bool((case // 5) & 1))
        seen[status] += 1
        cases += 1
        infeasible += none
    assert cases >= 300 and infeasible >= 0.05 * cases, (cases, infeasible)
    assert seen[1] >= 100 and seen[2] >= 15, seen


@pytest.mark.parametrize("single_root", [False, True])
@pytest.mark.parametrize("n", [5, 6, 9, 17])
def test_planted_crossing_cases(n, single_root):
    s = crossing_tree(n)
    pred = argmax_pred(s[None], [n])
    assert pred[0, 1:, 0].tolist() == crossing_heads(n)[1:]           # the arg-max is the crossing tree
    mst, _, st = E.tree_decode_arrays(s[None], [n], pred, single_root)
    assert st.tolist() == [0]
    _, out, status = run_one(s, n, single_root, pred)
    assert status == 1
    h = out[0, :, 0]
    assert E.is_tree(h, n, single_root, s) and E.is_projective(h, n)
    assert E.tree_total(s, h, n) < E.tree_total(s, mst[0, :, 0], n) == 100 * (n - 1)
    if n <= 6:
        assert E.tree_total(s, h, n) == brute_force_projective(s, n, single_root)
    # the same arcs as the only allowed ones: no projective tree
    s = only_crossing_tree(n)
    pred = argmax_pred(s[None], [n])
    assert E.tree_decode_arrays(s[None], [n], pred, single_root)[2].tolist() == [0]
    before, out, status = run_one(s, n, single_root, pred)
    assert status == 2 and np.array_equal(out, before)
    # the range rule, and the infeasible cases of the MST suite
    for build in (out_of_range, closed_group, forbidden_row):
        s = build(n)
        before, out, status = run_one(s, n, single_root)
        assert status == 2 and np.array_equal(out, before), build.__name__


def test_range_rule_is_a_threshold():
    """S * (n - 1) < 2^30 is decoded, S * (n - 1) >= 2^30 is not."""
    n = 5
    for top, expect in ((2 ** 28 - 1, 1), (2 ** 28, 2), (-(2 ** 28) + 1, 1), (-(2 ** 28), 2)):
        s = two_cycle(n)
        s[4, 1] = top
        assert run_one(s, n, True)[2] == expect, top
    s = two_cycle(n)
    s[0, 3] = s[3, 3] = 2 ** 30                                       # no arcs: not counted
    assert run_one(s, n, True)[2] == 1


def _dev_sentences(count):
    from ggnn_amd.batching import DATA_DIR, TRAIN_WITH_DEV, read_btb_json
    return read_btb_json(os.path.join(DATA_DIR, TRAIN_WITH_DEV["train_file"]))[:count]


def test_gold_trees_of_the_dev_set():
    rng = np.random.default_rng(4)
    for d in _dev_sentences(200):
        n = len(d["node_features"])
        gold = np.array([-1] + [t[0] for t in d["targets"]], np.int32)
        assert len(gold) == n and E.is_tree(gold, n, True) and E.is_projective(gold, n)
        s = rng.integers(0, 9, (n, n)).astype(np.int32)
        s[np.arange(1, n), gold[1:]] = 100                            # peaked: the optimum is unique
        s = finish(s)
        pred = np.zeros((1, n, 2), np.int32)
        pred[0, :, 0] = gold
        _, out, status = run_one(s, n, True, pred)
        assert status == 0 and np.array_equal(out, pred)
        if n < 3:
            continue
        for _ in range(20):                                           # one head corrupted: no projective tree
            h = gold.copy()
            i = int(rng.integers(1, n))
            h[i] = (gold[i] + 1 + int(rng.integers(0, n - 1))) % n
            if not (E.is_tree(h, n, True, s) and E.is_projective(h, n)):
                break
        else:
            raise AssertionError("no corruption found")
        pred[0, :, 0] = h
        _, out, status = run_one(s, n, True, pred)
        assert status == 1 and np.array_equal(out[0, :, 0], gold)


def test_projective_total_against_the_mst():
    rng = np.random.default_rng(31)
    total = lower = 0
    for case in range(24):
        n = int(rng.integers(8, 40))
        s = finish(rng.integers(0, 9, (n, n)))
        single_root = bool(case & 1)
        pred = argmax_pred(s[None], [n])
        mst, _, st = E.tree_decode_arrays(s[None], [n], pred, single_root)
        _, out, status = run_one(s, n, single_root, pred)
        assert st[0] in (0, 1) and status in (0, 1)
        a, b = E.tree_total(s, out[0, :, 0], n), E.tree_total(s, mst[0, :, 0], n)
        assert E.is_projective(out[0, :, 0], n) and E.is_tree(out[0, :, 0], n, single_root, s)
        assert a <= b
        total += 1
        lower += a < b
    assert lower >= total / 2, (lower, total)
    # with forbidden arcs and negative scores
    for case in range(40):
        n = int(rng.integers(3, 12))
        s = rng.integers(-8, 9, (n, n)).astype(np.int32)
        s[rng.random((n, n)) < 0.2] = F
        s = finish(s)
        pred = argmax_pred(s[None], [n])
        mst, _, st = E.tree_decode_arrays(s[None], [n], pred, True)
        _, out, status = run_one(s, n, True, pred)
        if st[0] == 2:
            assert status == 2                                        # no tree at all: no projective one
        elif status != 2:
            assert E.tree_total(s, out[0, :, 0], n) <= E.tree_total(s, mst[0, :, 0], n)


def test_counts_are_recounted_for_repaired_graphs_only():
    rng = np.random.default_rng(9)
    builds = [crossing_tree, chain, closed_group, two_cycle]
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
    out, c, status = E.projective_decode_arrays(s, n, pred, True, gold, counts)
    assert status.tolist() == [1, 0, 2, 1]
    for g in range(b):
        if status[g] != 1:
            assert np.array_equal(c[g], counts[g]) and np.array_equal(out[g], pred[g])
            continue
        uas = sum(1 for i in range(1, v) if gold[g, i, 0] >= 0 and out[g, i, 0] == gold[g, i, 0])
        las = sum(1 for i in range(1, v) if gold[g, i, 0] >= 0 and (out[g, i] == gold[g, i]).all())
        assert c[g].tolist() == [counts[g, 0], las, uas, counts[g, 3], counts[g, 4]]
    with pytest.raises(ValueError):
        E.projective_decode_arrays(s, n, pred, True, gold, None)
    with pytest.raises(ValueError):
        E.projective_decode_arrays(s[:, :, :7], n, pred, True)


def test_rows_and_columns_past_n_are_ignored():
    rng = np.random.default_rng(5)
    b, v, o, n = 1, 9, 11, 6
    s = np.full((b, v, o), 2 ** 30, np.int32)                         # (would break the range rule if read)
    s[0, :n, :n] = crossing_tree(n)
    pred = argmax_pred(s, [n], rng)
    pred[0, n:, :] = 3                                                # must come back untouched
    out, _, status = E.projective_decode_arrays(s, [n], pred, True)
    assert status.tolist() == [1] and np.array_equal(out[0, n:], pred[0, n:])
    assert E.tree_total(s[0], out[0, :, 0], n) == brute_force_projective(crossing_tree(n), n, True)


def test_n_below_two_and_n_two():
    s = finish(np.zeros((2, 2), np.int32))
    for single_root in (False, True):
        check_against_brute_force(s, 2, single_root)
        pred = np.full((3, 2, 2), 7, np.int32)
        out, _, status = E.projective_decode_arrays(np.stack([s, s, s]), [0, 1, 2], pred, single_root)
        assert status.tolist() == [0, 0, 1] and out[2, 1, 0] == 0     # head 7 is no arc: repaired
        assert np.array_equal(out[:2], pred[:2]) and out[2, 0, 0] == 7 and out[2, 1, 1] == 7
    blocked = s.copy()
    blocked[1, 0] = F
    assert check_against_brute_force(blocked, 2, True)[0] == 2


# ------------------------------------------------------------- the CPU model
def check_projective_predictions(m, feed, staged_scores):
    """predict_batch(tree="projective") of a feed against predict_batch().
    staged_scores(m, n_nodes, v) -> int32 [b, v, o] numpy scores of the batch
    the model holds.  Returns the status counts."""
    plain = m.predict_batch(dict(feed))
    p = m.predict_batch(dict(feed), tree="projective")
    b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
    status = p["tree_status"]
    assert status.shape == (b,) and status.dtype == np.int32
    assert np.array_equal(p["labels"], plain["labels"]) and np.array_equal(p["n_nodes"], plain["n_nodes"])
    s = staged_scores(m, p["n_nodes"], v)
    for g in range(b):
        n = int(p["n_nodes"][g])
        was = E.is_tree(plain["heads"][g], n, True, s[g]) and E.is_projective(plain["heads"][g], n)
        if status[g] == 2:
            assert np.array_equal(p["heads"][g], plain["heads"][g])
            continue
        assert E.is_tree(p["heads"][g], n, True, s[g]) and E.is_projective(p["heads"][g], n)
        assert (p["heads"][g, n:] == -1).all() and (status[g] == 0) == was
        if was:
            assert np.array_equal(p["heads"][g], plain["heads"][g])
        else:
            pred = np.stack([plain["heads"][g], plain["labels"][g]], axis=1)[None]
            host, _, st = E.projective_decode_arrays(s[g][None], [n], pred, True)
            assert st[0] == 1
            assert E.tree_total(s[g], p["heads"][g], n) == E.tree_total(s[g], host[0, :, 0], n)
    return [int((status == k).sum()) for k in (0, 1, 2)]


def test_model_projective_keyword_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    data = m.process_raw_graphs(raw, False)
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        seen += check_projective_predictions(m, feed, _host_scores)
    assert seen[0] > 0 and seen[1] > 0 and seen[2] == 0, seen
    plain, parsed = m.parse(raw), m.parse(raw, tree="projective")
    for d, a, t in zip(raw, plain, parsed):
        n = len(d["node_features"])
        assert len(t) == n - 1 and [x[1] for x in t] == [x[1] for x in a]
        h = [-1] + [x[0] for x in t]
        assert E.is_tree(h, n, True) and E.is_projective(h, n)
    assert sum(a != t for a, t in zip(plain, parsed)) == seen[1]
    multi = m.parse(raw, tree="projective", single_root=False)
    for d, t in zip(raw, multi):
        h = [-1] + [x[0] for x in t]
        assert E.is_tree(h, len(d["node_features"]), False) and E.is_projective(h, len(d["node_features"]))
    first = next(iter(m.make_minibatch_iterator(data, False)))
    for bad in ("mst", "Projective", 1, 2, None):
        with pytest.raises(ValueError):
            m.predict_batch(dict(first), tree=bad)
        with pytest.raises(ValueError):
            m.parse(raw[:2], tree=bad)
        with pytest.raises(ValueError):
            m.evaluate_batch(dict(first), on_device=True, tree=bad)
        with pytest.raises(ValueError):
            m.score_epoch(data, tree=bad)
    with pytest.raises(ValueError):
        m.evaluate_batch(dict(first), tree="projective")              # needs on_device=True
    # evaluate_batch / score_epoch: the scores of predict_batch(tree="projective")'s heads
    graphs, las, uas = 0, 0.0, 0.0
    for feed in m.make_minibatch_iterator(data, False):
        got = m.evaluate_batch(dict(feed), on_device=True, tree="projective")
        r = m._decode_forward(dict(feed), True, "projective", True)
        p = m.predict_batch(dict(feed), tree="projective")
        assert np.array_equal(r["pred"][:, :, 0], p["heads"])
        per_graph = [E.graph_scores_from_lists(r["pred"][g], r["gold"][g]) for g in range(r["b"])]
        assert got == tuple(sum(x[c] for x in per_graph) / r["b"] for c in range(3))
        graphs += r["b"]
        las += got[0] * r["b"]
        uas += got[1] * r["b"]
    ref = m.score_epoch(data)
    got = m.score_epoch(data, tree="projective")
    assert m.decode_stats["repaired_graphs"] == seen[1] and m.decode_stats["infeasible_graphs"] == seen[2]
    assert set(m.decode_stats) == {"graphs", "fallback_graphs", "d2h_bytes", "repaired_graphs", "infeasible_graphs"}
    assert got[0] == ref[0] and got[3] == ref[3] and got[5] == ref[5]
    assert got[1:3] == (las / graphs, uas / graphs)                   # (_epoch's order of additions)
    assert m.score_epoch(data)[:4] == ref[:4]


# ------------------------------------------------------------------- the ABI
def test_projective_decode_rejects_bad_arguments_without_gpu(lib):
    """ggnn_projective_decode validates on the host before any launch."""
    from ggnn_amd import _lib
    P = ctypes.c_void_p
    x = P(256)                                        # never dereferenced: every call below fails validation
    ok = dict(b=2, v=30, o=150, s=x, n=x, single=1, pred=x, gold=None, counts=None, status=x, ws=None, ws_bytes=0)
    L = _lib.PROJ_LDS_MAXN
    need = 2 * 8 * (L + 1) * (L + 2)
    for change, word in ((dict(o=0), b"1..1024"), (dict(o=1025), b"1..1024"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(b=0), b">= 1"), (dict(s=None), b"NULL"),
                         (dict(n=None), b"NULL"), (dict(pred=None), b"NULL"), (dict(status=None), b"NULL"),
                         (dict(gold=x), b"together"), (dict(counts=x), b"together"), (dict(single=2), b"0 or 1"),
                         (dict(v=L + 1), b"workspace"), (dict(v=L + 1, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=L + 1, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_projective_decode(ctypes.byref(d), a["s"], a["o"], a["n"], a["single"], a["pred"], a["gold"],
                                        a["counts"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
    assert lib.ggnn_projective_decode(None, x, 150, x, 1, x, None, None, x, None, 0, None) == -1
    assert lib.ggnn_projective_decode_workspace_bytes(2, L + 1) == need
    assert lib.ggnn_projective_decode_workspace_bytes(256, L) == 0
    assert lib.ggnn_projective_decode_workspace_bytes(3, 256) == 3 * 8 * 256 * 257
    assert {"ggnn_projective_decode", "ggnn_projective_decode_workspace_bytes"} <= set(_lib.EXPORTED)
    assert L == E.PROJ_LDS_MAXN and 8 * L * (L + 1) <= 160 * 1024 and L < _lib.TREE_MAXV
