"""ggnn_tree_decode on the GPU against its host form
(evaluation.tree_decode_arrays): status, totals, untouched outputs, counts and
reproducibility, and the model's tree= keywords against host scores of the
returned heads.  Exact integer and bit equality only; under ties the device's
tree may differ from the host's, its total may not."""
import numpy as np
import pytest

from decode_cases import _device_scores, _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from test_tree_decode import (F, all_ties, argmax_pred, check_tree_predictions, closed_group, finish, forbidden_row,
                              full_cycle, nested_cycle, no_root_child, three_roots, two_cycle)

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 150),      # the smallest bucket
          (3, 8, 8),        # v = o
          (2, 64, 64),      # exact wave width
          (2, 130, 150),    # partial third lane chunk
          (2, 198, 198)]    # the largest reference bucket
CYCLES = [two_cycle, full_cycle, nested_cycle, no_root_child, three_roots, all_ties]
RANDOM_LAUNCHES = 3


def _n_vectors(b, v):
    """Three launches per shape: together every graph count of 2, an interior
    value and v occurs (tests/test_gpu_decode.py::_n_vectors, padded to b)."""
    mid = max(2, min(v - 1, v // 2 + 1))
    return [([2, mid, v] + [v] * b)[:b], ([v, mid, 2] + [mid] * b)[:b], ([v, mid, v] + [2] * b)[:b]]


def _launches(shape):
    """The launches of a shape: RANDOM_LAUNCHES with random graphs, then (v >= 6)
    the planted cycle cases; graph 1 of every launch has no tree."""
    b, v, o = shape
    out = [("random", k) for k in range(RANDOM_LAUNCHES)]
    if v >= 6:
        out += [("planted", k) for k in range(-(-len(CYCLES) // (b - 1)))]
    return out


def _infeasible(n, k):
    if n == 2:
        s = finish(np.zeros((2, 2), np.int32))
        s[1, 0] = F
        return s
    return closed_group(n) if (k & 1) or n == 3 else forbidden_row(n)


def _case(shape, kind, k):
    """(scores [b, v, o], n [b], single_root, kinds [b]) of one launch.  Rows
    and columns >= n hold large values that must be ignored."""
    b, v, o = shape
    rng = np.random.default_rng(7000 + 100 * v + 10 * k + (kind == "planted"))
    s = np.full((b, v, o), 1000, np.int32)
    kinds = []
    if kind == "random":
        n = _n_vectors(b, v)[k]
        single_root = k != 1
    else:
        big, mid = v, max(6, v // 2 + 1)
        n = [big if (g + k) & 1 else mid for g in range(b)]
        single_root = True
    cycles = iter(CYCLES[k * (b - 1):] + CYCLES)
    for g in range(b):
        if g == 1:
            block, what = _infeasible(n[g], k), "infeasible"
        elif kind == "random":
            block, what = finish(rng.integers(0, 9, (n[g], n[g]))), "random"
        else:
            build = next(cycles)
            block, what = build(n[g]), build.__name__
        s[g, :n[g], :n[g]] = block
        kinds.append(what)
    return s, np.asarray(n, np.int32), single_root, kinds


_REFERENCE = {}


def _reference(shape, kind, k):
    """One launch's inputs and host results, computed once and left unchanged."""
    key = (shape, kind, k)
    if key not in _REFERENCE:
        b, v, o = shape
        s, n, single_root, kinds = _case(shape, kind, k)
        rng = np.random.default_rng(11 + v + k)
        pred = argmax_pred(s, n, rng)
        gold = np.full((b, v, 2), -1, np.int32)
        for g in range(b):
            m = int(n[g])
            gold[g, 1:m, 0] = rng.integers(0, m, m - 1)
            gold[g, 1:m, 1] = np.where(rng.random(m - 1) < 0.5, pred[g, 1:m, 1], 12)
            if m > 3:
                gold[g, 3] = -1                                       # a row without gold is not counted
        counts = rng.integers(300, 400, (b, 5)).astype(np.int32)
        levels = []
        host = E.tree_decode_arrays(s, n, pred, single_root, gold, counts, levels=levels)
        for a in (s, n, pred, gold, counts) + host:
            a.setflags(write=False)
        _REFERENCE[key] = (s, n, single_root, kinds, pred, gold, counts, host, levels)
    return _REFERENCE[key]


def _launch(torch, s, n, pred, single_root, gold=None, counts=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    pred, gold, counts = t(pred), t(gold), t(counts)
    status = OutputHeads(64).tree_decode(t(s), t(n), pred, gold, counts, single_root)
    torch.cuda.synchronize()
    assert status.dtype == torch.int32
    return pred.cpu().numpy(), None if counts is None else counts.cpu().numpy(), status.cpu().numpy()


ALL_LAUNCHES = [(shape,) + launch for shape in SHAPES for launch in _launches(shape)]


@pytest.mark.parametrize("shape,kind,k", ALL_LAUNCHES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_kernel_equals_host_tree_decode(shape, kind, k):
    torch = _torch()
    b, v, o = shape
    s, n, single_root, kinds, pred, gold, counts, (h_pred, h_counts, h_status), levels = _reference(shape, kind, k)
    assert h_status[1] == 2                                           # one infeasible graph per launch
    if kind == "planted":
        for g, what in enumerate(kinds):
            if what == "nested_cycle":
                assert levels[g] >= 2 and h_status[g] == 1
            elif what not in ("infeasible",):
                assert h_status[g] == 1, (what, h_status)
    with_gold = not (kind == "random" and k == 1)
    got, c, status = _launch(torch, s, n, pred, single_root, gold if with_gold else None,
                             counts if with_gold else None)
    assert np.array_equal(status, h_status), (status, h_status, kinds)
    assert np.array_equal(got[:, :, 1], pred[:, :, 1]) and np.array_equal(got[:, 0], pred[:, 0])
    for g in range(b):
        m = int(n[g])
        assert np.array_equal(got[g, m:], pred[g, m:])
        if status[g] != 1:
            assert got[g].tobytes() == pred[g].tobytes()
            continue
        assert E.is_tree(got[g, :, 0], m, single_root, s[g]), (g, kinds[g])
        assert E.tree_total(s[g], got[g, :, 0], m) == E.tree_total(s[g], h_pred[g, :, 0], m), (g, kinds[g])
    if not with_gold:
        assert c is None
        return
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


def test_the_random_graphs_are_hard_enough():
    """The host form alone: of the suite's random graphs with n >= 8, at least
    40 % are no trees under arg-max and at least 15 % need nested contractions."""
    total = broken = nested = 0
    for shape in SHAPES:
        for k in range(RANDOM_LAUNCHES):
            _, n, _, kinds, _, _, _, (_, _, status), levels = _reference(shape, "random", k)
            for g, what in enumerate(kinds):
                if what == "random" and n[g] >= 8:
                    total += 1
                    broken += status[g] != 0
                    nested += levels[g] >= 2
    assert total >= 10
    assert broken >= 0.4 * total and nested >= 0.15 * total, (total, broken, nested)


def test_two_launches_give_identical_bytes():
    torch = _torch()
    s, n, single_root, _, pred, gold, counts, _, _ = _reference((2, 130, 150), "random", 2)
    a = _launch(torch, s, n, pred, single_root, gold, counts)
    b = _launch(torch, s, n, pred, single_root, gold, counts)
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
            oh.tree_decode(**dict(dict(scores=s, n_nodes=n, pred=pred), **bad))


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_predict_batch_and_parse_return_trees(graphs):
    _torch()
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    data = m.process_raw_graphs(raw, False)
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        seen += check_tree_predictions(m, feed, _device_scores)
    assert seen[1] > 0 and seen[2] == 0, seen                         # an untrained model: repairs, all feasible
    plain, parsed = m.parse(raw), m.parse(raw, tree=True)
    for d, a, t in zip(raw, plain, parsed):
        n = len(d["node_features"])
        assert len(t) == n - 1 and [x[1] for x in t] == [x[1] for x in a]
        assert E.is_tree([-1] + [x[0] for x in t], n, True)
    assert sum(a != t for a, t in zip(plain, parsed)) == seen[1]


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_evaluate_batch_and_score_epoch_score_the_tree_heads(graphs):
    torch = _torch()
    m = _synthetic_model(graphs)
    data = m.process_raw_graphs(_synthetic_raw(), False)
    with pytest.raises(ValueError):
        m.evaluate_batch(next(iter(m.make_minibatch_iterator(data, False))), tree=True)
    tot = [0, 0.0, 0.0, 0.0]
    for feed in m.make_minibatch_iterator(data, False):
        r = m._decode_forward(dict(feed), True)                       # the decode's gold lists
        gold = r["gold"].cpu().numpy()
        p = m.predict_batch(dict(feed), tree=True)
        pred = np.stack([p["heads"], p["labels"]], axis=2)
        b = int(feed["num_graphs"])
        per_graph = [E.graph_scores_from_lists(pred[g], gold[g]) for g in range(b)]
        host = [0.0, 0.0, 0.0]
        for x in per_graph:                                           # (scores_from_counts' order of additions)
            for c in range(3):
                host[c] += x[c]
        host = tuple(x / b for x in host)
        assert m.evaluate_batch(dict(feed), on_device=True, tree=True) == host
        tot[0] += b
        for c in range(3):
            tot[1 + c] += host[c] * b
    plain = m.score_epoch(data)
    assert m.decode_stats["repaired_graphs"] == 0 and m.decode_stats["infeasible_graphs"] == 0
    got = m.score_epoch(data, tree=True)
    torch.cuda.synchronize()
    st = m.decode_stats
    assert st["repaired_graphs"] > 0 and st["graphs"] == tot[0] and st["fallback_graphs"] == 0, st
    assert got[1:4] == (tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0]), (got, tot)
    assert got[0] == plain[0] and got[3] == plain[3] and got[5] == plain[5]
    # fetched per batch: the loss, [b, 5] counts and [b] status
    assert st["d2h_bytes"] == sum(4 + 4 * 6 * int(f["num_graphs"]) for f in m.make_minibatch_iterator(data, False))


def test_score_epoch_without_the_keyword_is_unchanged():
    """score_epoch(data) on the first 40 dev sentences at batch 20 still returns
    run_epoch's loss and scores and fetches the loss and [b, 5] counts only."""
    torch = _torch()
    from ggnn_amd.batching import TRAIN_WITH_DEV, wsj_model_sizes
    from ggnn_amd.model import DenseGGNNChemModel
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20,
                                   "compact_adjacency": True}, seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False, restrict=40)
    ref = m.run_epoch("valid", data, False)
    got = m.score_epoch(data)
    torch.cuda.synchronize()
    assert got[:4] == (ref[0], ref[5], ref[6], ref[16]) and got[5] == ref[4]
    st = m.decode_stats
    assert st["graphs"] == 40 and st["fallback_graphs"] == 0 and st["repaired_graphs"] == 0, st
    assert st["d2h_bytes"] == sum(4 + 4 * 5 * cv.shape[0] for cv in ref[8])
    tree = m.score_epoch(data, tree=True)
    torch.cuda.synchronize()
    assert tree[0] == got[0] and tree[3] == got[3] and m.decode_stats["repaired_graphs"] > 0
