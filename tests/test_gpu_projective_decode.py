"""ggnn_projective_decode on the GPU against its host form
(evaluation.projective_decode_arrays): status, totals, untouched outputs,
counts and reproducibility at both storage tiers, and the model's
tree="projective" keyword against host scores of the returned heads.  Exact
integer and bit equality only; under ties the device's tree may differ from the
host's, its total may not."""
import numpy as np
import pytest

from decode_cases import _batch_bytes, _device_scores, _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from ggnn_amd._lib import PROJ_LDS_MAXN as L
from test_projective_decode import check_projective_predictions, crossing_tree, only_crossing_tree, out_of_range
from test_tree_decode import F, argmax_pred, closed_group, finish, forbidden_row

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 150),                       # the smallest bucket
          (3, 8, 8),                         # v = o
          (2, 64, 64),                       # exact wave width
          (2, 65, 150),                      # one past it
          (3, L, max(L, 150)),               # the largest graphs with tables in LDS
          (3, L + 1, max(L + 1, 150)),       # both storage tiers in one grid
          (2, 198, 198),                     # the largest reference bucket
          (1, 256, 256)]                     # GGNN_TREE_MAXV
BIG = 2 ** 30                                # rows and columns >= n: never read (would break the range rule)


def _node_counts(v):
    """2, an interior value and v; around PROJ_LDS_MAXN also L - 1, L, L + 1
    and one short graph."""
    out = [v, 5] if v == L + 1 else [v]      # (first: n = L + 1 and n = 5 share a launch)
    out += [2, max(2, min(v - 1, v // 2 + 1))]
    if v in (L, L + 1):
        out += [x for x in (L - 1, L) if x < v]
    return list(dict.fromkeys(out))


def _launches(shape):
    """The launches of a shape as lists of b (n, kind): every node count as a
    dense random graph, as a random graph with 25 % forbidden arcs, as a tree
    peaked on a projective tree (the fast path) and, n >= 5, as the planted
    crossing tree; graph 1 of every launch (b = 1: launches of their own) is
    infeasible or out of range."""
    b, v, o = shape
    counts = _node_counts(v)
    jobs = [(n, "dense") for n in counts] + [(n, "sparse") for n in counts]
    jobs += [(n, "crossing_tree") for n in counts if n >= 5] + [(n, "peaked_projective") for n in counts[:2]]
    bad = ["only_crossing_tree", "closed_group", "forbidden_row", "out_of_range"]
    out = []
    per = max(1, b - 1)
    for k in range(-(-len(jobs) // per)):
        part = jobs[k * per:(k + 1) * per]
        part += jobs[:per - len(part)]
        if b > 1:
            part.insert(1, (counts[k % len(counts)], bad[k % len(bad)]))
        out.append(part)
    if b == 1:
        out += [[(counts[k % len(counts)], bad[k])] for k in range(len(bad))]
    return out


def _graph(n, kind, rng):
    if kind == "dense":
        return finish(rng.integers(0, 9, (n, n)))
    if kind == "sparse":
        s = rng.integers(-8, 9, (n, n)).astype(np.int32)
        s[rng.random((n, n)) < 0.25] = F
        return finish(s)
    if kind == "peaked_projective":
        s = rng.integers(0, 9, (n, n)).astype(np.int32)
        h = E.random_projective_heads(n, rng)
        s[np.arange(1, n), h[1:]] = 100
        return finish(s)
    if n == 2:                                # the planted cases need more words: the one arc forbidden
        s = finish(np.zeros((2, 2), np.int32))
        s[1, 0] = F
        return s
    if n < 5 and kind in ("crossing_tree", "only_crossing_tree"):
        kind = "closed_group"
    return {"crossing_tree": crossing_tree, "only_crossing_tree": only_crossing_tree, "closed_group": closed_group,
            "forbidden_row": forbidden_row, "out_of_range": out_of_range}[kind](n)


_REFERENCE = {}


def _reference(shape, k):
    """One launch's inputs and both host results (single_root False / True),
    computed once and left unchanged."""
    key = (shape, k)
    if key not in _REFERENCE:
        b, v, o = shape
        part = _launches(shape)[k]
        rng = np.random.default_rng(9000 + 100 * v + k)
        n = np.asarray([x[0] for x in part], np.int32)
        kinds = [x[1] for x in part]
        s = np.full((b, v, o), BIG, np.int32)
        for g in range(b):
            s[g, :n[g], :n[g]] = _graph(int(n[g]), kinds[g], rng)
        pred = argmax_pred(s, n, rng)
        gold = np.full((b, v, 2), -1, np.int32)
        for g in range(b):
            m = int(n[g])
            pred[g, m:] = 7                                           # must come back untouched
            gold[g, 1:m, 0] = rng.integers(0, m, m - 1)
            gold[g, 1:m, 1] = np.where(rng.random(m - 1) < 0.5, pred[g, 1:m, 1], 12)
            if m > 3:
                gold[g, 3] = -1                                       # a row without gold is not counted
        counts = rng.integers(300, 400, (b, 5)).astype(np.int32)
        host = {sr: E.projective_decode_arrays(s, n, pred, sr, gold, counts) for sr in (False, True)}
        for a in (s, n, pred, gold, counts) + host[False] + host[True]:
            a.setflags(write=False)
        _REFERENCE[key] = (s, n, kinds, pred, gold, counts, host)
    return _REFERENCE[key]


def _launch(torch, s, n, pred, single_root, gold=None, counts=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    pred, gold, counts = t(pred), t(gold), t(counts)
    status = OutputHeads(64).projective_decode(t(s), t(n), pred, gold, counts, single_root)
    torch.cuda.synchronize()
    assert status.dtype == torch.int32
    return pred.cpu().numpy(), None if counts is None else counts.cpu().numpy(), status.cpu().numpy()


ALL_LAUNCHES = [(shape, k) for shape in SHAPES for k in range(len(_launches(shape)))]


def test_the_launches_cover_the_issue():
    for shape in SHAPES:
        b, v, o = shape
        seen = set()
        for part in _launches(shape):
            assert len(part) == b
            seen |= {x[0] for x in part if x[1] == "dense"}
            assert b == 1 or part[1][1] in ("only_crossing_tree", "closed_group", "forbidden_row", "out_of_range")
        assert {2, v} <= seen and any(2 < x < v for x in seen)
        if v == L:
            assert {L - 1, L} <= seen
        if v == L + 1:
            assert {L - 1, L, L + 1} <= seen
            assert any({L + 1, 5} <= {x[0] for x in part} for part in _launches(shape))


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_kernel_equals_host_projective_decode(shape, k):
    torch = _torch()
    b, v, o = shape
    s, n, kinds, pred, gold, counts, host = _reference(shape, k)
    for single_root in (False, True):
        h_pred, h_counts, h_status = host[single_root]
        for g, what in enumerate(kinds):                              # the cases are what they claim to be
            if what in ("only_crossing_tree", "closed_group", "forbidden_row", "out_of_range"):
                assert h_status[g] == 2, (what, n[g])
            elif what == "peaked_projective":
                assert h_status[g] == 0
            elif what == "crossing_tree" and n[g] >= 5:
                assert h_status[g] == 1
        for with_gold in (True, False):
            got, c, status = _launch(torch, s, n, pred, single_root, gold if with_gold else None,
                                     counts if with_gold else None)
            assert np.array_equal(status, h_status), (status, h_status, kinds, n)
            assert np.array_equal(got[:, :, 1], pred[:, :, 1]) and np.array_equal(got[:, 0], pred[:, 0])
            for g in range(b):
                m = int(n[g])
                assert np.array_equal(got[g, m:], pred[g, m:])
                if status[g] != 1:
                    assert got[g].tobytes() == pred[g].tobytes()
                    continue
                assert E.is_tree(got[g, :, 0], m, single_root, s[g]), (g, kinds[g])
                assert E.is_projective(got[g, :, 0], m), (g, kinds[g])
                assert E.tree_total(s[g], got[g, :, 0], m) == E.tree_total(s[g], h_pred[g, :, 0], m), (g, kinds[g])
            if not with_gold:
                assert c is None
                continue
            for g in range(b):
                if status[g] != 1:
                    assert np.array_equal(c[g], counts[g])
                    continue
                # (the device's tree may differ from the host's under ties: recount its own heads)
                has = gold[g, 1:, 0] >= 0
                hit_h = has & (got[g, 1:, 0] == gold[g, 1:, 0])
                las = int((hit_h & (got[g, 1:, 1] == gold[g, 1:, 1])).sum())
                assert c[g].tolist() == [counts[g, 0], las, int(hit_h.sum()), counts[g, 3], counts[g, 4]]
                if np.array_equal(got[g], h_pred[g]):
                    assert np.array_equal(c[g], h_counts[g])


def test_the_projective_optimum_is_below_the_mst():
    """The host forms alone: on the suite's dense random graphs with 8 <= n <=
    70 the best projective tree scores strictly less than the MST."""
    total = lower = 0
    for shape in SHAPES:
        for k in range(len(_launches(shape))):
            part = _launches(shape)[k]
            if not any(kind == "dense" and 8 <= m <= 70 for m, kind in part):
                continue
            s, n, kinds, pred, _, _, host = _reference(shape, k)
            mst, _, _ = E.tree_decode_arrays(s, n, pred, True)
            for g, what in enumerate(kinds):
                if what == "dense" and 8 <= n[g] <= 70:
                    total += 1
                    a = E.tree_total(s[g], host[True][0][g, :, 0], n[g])
                    c = E.tree_total(s[g], mst[g, :, 0], n[g])
                    assert a <= c
                    lower += a < c
    assert total >= 3 and lower >= total / 2, (total, lower)


@pytest.mark.parametrize("shape", [(2, 65, 150), (3, L + 1, max(L + 1, 150))], ids=["lds", "both-tiers"])
def test_two_launches_give_identical_bytes(shape):
    torch = _torch()
    s, n, _, pred, gold, counts, _ = _reference(shape, 0)
    a = _launch(torch, s, n, pred, True, gold, counts)
    b = _launch(torch, s, n, pred, True, gold, counts)
    assert (a[2] == 1).any()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    s = torch.zeros(2, 4, 6, dtype=torch.int32, device=dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    pred = torch.zeros(2, 4, 2, dtype=torch.int32, device=dev)
    for bad in (dict(scores=s.float()), dict(scores=s.cpu()), dict(n_nodes=n.long()), dict(pred=pred[:, :3]),
                dict(gold=pred), dict(scores=torch.zeros(2, 8, 6, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            oh.projective_decode(**dict(dict(scores=s, n_nodes=n, pred=pred), **bad))
    # a workspace too small for graphs above PROJ_LDS_MAXN nodes
    v = L + 1
    s = torch.zeros(2, v, v, dtype=torch.int32, device=dev)
    pred = torch.zeros(2, v, 2, dtype=torch.int32, device=dev)
    need = 2 * 8 * v * (v + 1)
    with pytest.raises(ValueError):
        oh.projective_decode(s, n, pred, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        oh.projective_decode(s, n, pred, workspace=torch.empty(need, dtype=torch.int32, device=dev))
    status = oh.projective_decode(s, n, pred, workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1, 1]                            # all heads 0: three ROOT children


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_model_projective_keyword(graphs):
    torch = _torch()
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    data = m.process_raw_graphs(raw, False)
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        seen += check_projective_predictions(m, feed, _device_scores)
    assert seen[1] > 0 and seen[2] == 0, seen                         # an untrained model: repairs, all feasible
    plain, parsed = m.parse(raw), m.parse(raw, tree="projective")
    for d, a, t in zip(raw, plain, parsed):
        n = len(d["node_features"])
        assert len(t) == n - 1 and [x[1] for x in t] == [x[1] for x in a]
        h = [-1] + [x[0] for x in t]
        assert E.is_tree(h, n, True) and E.is_projective(h, n)
    assert sum(a != t for a, t in zip(plain, parsed)) == seen[1]
    with pytest.raises(ValueError):
        m.parse(raw[:2], tree="eisner")
    # evaluate_batch / score_epoch: host scores of the returned heads
    tot = [0, 0.0, 0.0, 0.0]
    for feed in m.make_minibatch_iterator(data, False):
        gold = m._decode_forward(dict(feed), True)["gold"].cpu().numpy()   # the decode's gold lists
        p = m.predict_batch(dict(feed), tree="projective")
        pred = np.stack([p["heads"], p["labels"]], axis=2)
        b = int(feed["num_graphs"])
        host = [0.0, 0.0, 0.0]
        for g in range(b):                                            # (scores_from_counts' order of additions)
            x = E.graph_scores_from_lists(pred[g], gold[g])
            for c in range(3):
                host[c] += x[c]
        host = tuple(x / b for x in host)
        assert m.evaluate_batch(dict(feed), on_device=True, tree="projective") == host
        tot[0] += b
        for c in range(3):
            tot[1 + c] += host[c] * b
    plain = m.score_epoch(data)
    torch.cuda.synchronize()
    st = m.decode_stats
    assert st["repaired_graphs"] == 0 and st["infeasible_graphs"] == 0
    assert st["d2h_bytes"] == _batch_bytes(m, data, 5)                # the loss and [b, 5] counts, as before
    mst = m.score_epoch(data, tree=True)
    torch.cuda.synchronize()
    assert m.decode_stats["d2h_bytes"] == _batch_bytes(m, data, 6) and m.decode_stats["repaired_graphs"] > 0
    got = m.score_epoch(data, tree="projective")
    torch.cuda.synchronize()
    st = m.decode_stats
    assert st["repaired_graphs"] == seen[1] and st["graphs"] == tot[0] and st["fallback_graphs"] == 0, st
    assert got[1:4] == (tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0]), (got, tot)
    assert got[0] == plain[0] and got[3] == plain[3] and got[5] == plain[5]
    assert mst[0] == plain[0] and mst[3] == plain[3] and mst[5] == plain[5]
    # fetched per batch: the loss, [b, 5] counts and [b] status
    assert st["d2h_bytes"] == _batch_bytes(m, data, 6)
    assert m.score_epoch(data)[:4] == plain[:4]
