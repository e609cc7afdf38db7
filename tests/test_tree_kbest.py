"""The host form of ggnn_tree_kbest (evaluation.tree_kbest_arrays) against
brute-force enumeration of all dependency trees (n = 2..6, both root modes,
tree_scores scores, 25 % forbidden arcs and a tie-heavy copy, K = 1, 3, 8, 16),
rank 0 against tree_decode_arrays made to run, the prefix property, the edge
statuses, garbage in the padding, the batches of tests/tree_kbest_cases.py, the
model's kbest_family / family keywords on a CPU device through HostDecoder
(the default family untouched), the two backends' signatures, the library's
host-side checks and the header's byte formula."""
import ctypes
import inspect

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from test_tree_decode import _synthetic_model, _synthetic_raw
from tree_kbest_cases import F, KINDS, brute_force, launch, reference, scores_batch, with_garbage

KS = (1, 3, 8, 16)


def _small_cases():
    for n in range(2, 7):
        for kind in KINDS:
            for rep in range(4):
                yield n, kind, scores_batch([n], 7, 8, kind, 1000 * n + 10 * rep + KINDS.index(kind))


def test_host_form_equals_brute_force_and_the_tree_decode():
    graphs = cases = fewer = none = tied = 0
    for n, kind, s in _small_cases():
        for single_root in (True, False):
            trees = brute_force(s[0], n, single_root)
            want = sorted((t for t, _ in trees), reverse=True)
            tied += len(set(want[:16])) < len(want[:16])
            pred = np.full((1, 7, 2), -1, np.int32)                  # no heads: the tree pass runs
            best, _, best_status = E.tree_decode_arrays(s, [n], pred, single_root)
            graphs += 1
            for K in KS:
                heads, totals, count, status = E.tree_kbest_arrays(s, [n], K, single_root)
                assert heads.shape == (1, K, 7) and totals.shape == (1, K) and count.shape == status.shape == (1,)
                assert all(a.dtype == np.int32 for a in (heads, totals, count, status))
                c = int(count[0])
                assert c == min(K, len(trees)) and status[0] == (1 if c else 2)
                assert totals[0, :c].tolist() == want[:c]
                assert (totals[0, c:] == F).all() and (heads[0, c:] == -1).all()
                assert (heads[0, :, 0] == -1).all() and (heads[0, :, n:] == -1).all()
                assert len({tuple(h) for h in heads[0, :c]}) == c
                for r in range(c):
                    h = heads[0, r]
                    assert E.is_tree(h, n, single_root, s[0])
                    assert E.tree_total(s[0], h, n) == totals[0, r]
                if c == 0:
                    assert best_status[0] == 2
                else:
                    assert best_status[0] == 1 and heads[0, 0, 1:n].tolist() == best[0, 1:n, 0].tolist()   # ties included
                cases += 1
                fewer += 0 < len(trees) < K
                none += not trees
    assert graphs == 120 and cases == 480 and fewer > 0 and none > 0 and tied > 0, (graphs, cases, fewer, none, tied)


def test_k4_is_a_prefix_of_k16():
    ns = [6, 5, 9, 12]
    for kind in KINDS:
        s = scores_batch(ns, 12, 12, kind, 7)
        for single_root in (True, False):
            a = E.tree_kbest_arrays(s, ns, 4, single_root)
            c = E.tree_kbest_arrays(s, ns, 16, single_root)
            assert np.array_equal(a[0], c[0][:, :4]) and np.array_equal(a[1], c[1][:, :4])
            assert np.array_equal(a[2], np.minimum(c[2], 4)) and np.array_equal(a[3], c[3])
            assert (c[2] > 4).any()
            live = c[1][:, 1:] != F
            assert (c[1].astype(np.int64)[:, :-1][live] >= c[1].astype(np.int64)[:, 1:][live]).all()   # best first


def test_edge_statuses_and_bad_arguments():
    s = scores_batch([1, 0, 4, 4, 2], 5, 6, "soft", 3)
    s[3, 2, 1] = -(2 ** 30 - 1)                     # |S| * (n - 1) >= 2^30
    heads, totals, count, status = E.tree_kbest_arrays(s, [1, 0, 4, 4, 2], 3)
    assert status.tolist() == [0, 0, 1, 2, 1] and count.tolist() == [0, 0, 3, 0, 1]
    assert (heads[[0, 1, 3]] == -1).all() and (totals[[0, 1, 3]] == F).all()
    assert heads[4, 0].tolist() == [-1, 0, -1, -1, -1] and totals[4, 0] == s[4, 1, 0]
    s[3, 2, 1] = 2 ** 30 // 3 - 1                   # the largest score a 4-node graph may hold
    assert E.tree_kbest_arrays(s, [1, 0, 4, 4, 2], 3)[3][3] == 1
    for bad in (dict(K=0), dict(K=17), dict(scores=s.astype(np.int64)), dict(scores=s[:, :, :4]), dict(n_nodes=[1, 2])):
        with pytest.raises(ValueError):
            E.tree_kbest_arrays(**dict(dict(scores=s, n_nodes=[1, 0, 4, 4, 2], K=2), **bad))


def test_garbage_in_the_padding_changes_nothing():
    ns = [3, 1, 6, 8, 5]
    for kind in KINDS:
        s = scores_batch(ns, 8, 10, kind, 11)
        dirty = with_garbage(s, ns)
        assert not np.array_equal(s, dirty)
        for single_root in (True, False):
            for a, c in zip(E.tree_kbest_arrays(s, ns, 8, single_root), E.tree_kbest_arrays(dirty, ns, 8, single_root)):
                assert a.tobytes() == c.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_batches_are_what_the_gpu_tests_need(kind):
    """The references of both GPU launches, whose own assertions (the special
    graphs' statuses, full lists for n >= 23 with the soft kind) run inside
    ``reference``: a kind or seed that stops doing its job fails here, on the
    CPU."""
    s, n = launch("wave", kind)
    assert s.shape == (4, 66, 69) and n.tolist() == [63, 64, 65, 66]
    s, n = launch("main", kind)
    assert s.shape == (9, 34, 37) and n.tolist() == [1, 2, 3, 5, 23, 33, 34, 6, 4]
    for single_root in (True, False):
        heads, totals, count, status = reference("wave", kind, single_root, 2)
        assert heads.shape == (4, 2, 66) and (status == 1).all() and (count >= 1).all()
        for K in (1, 2, 16):
            heads, totals, count, status = reference("main", kind, single_root, K)
            assert heads.shape == (9, K, 34) and totals.shape == (9, K)
            assert status.tolist()[4:] == [1, 1, 1, 2, 2] and status[0] == 0 and (count[4:7] >= 1).all()
            assert (count <= K).all() and (heads[:, :, 0] == -1).all()


def _irregular_first_graph(m):
    """The model's stand-in forward with word 1 of every batch's first graph
    given an all-zero row of head probabilities (no prediction: irregular)."""
    inner = m.build_loss

    def build_loss(task_id=0):
        loss = inner(task_id)
        b, v = int(m.placeholders["num_graphs"]), int(m.placeholders["num_vertices"])
        cv = m.ops["computed_values"].numpy().reshape(b, v, -1)
        cv[0, 1, :] = 0.0
        return loss
    m.build_loss = build_loss
    return m


def _same_dict(a, c):
    assert set(a) == set(c)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == c[k].dtype and a[k].tobytes() == c[k].tobytes(), k
        else:
            assert a[k] is c[k] or a[k] == c[k], k


def test_model_keywords_on_a_cpu_device():
    m = _irregular_first_graph(_synthetic_model())
    raw = _synthetic_raw()
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o, K = m.params["output_size"], 3
    regular_seen = irregular_seen = 0
    for feed in list(m.make_minibatch_iterator(data, False))[:2]:
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        plain = m.predict_batch(dict(feed))
        # the default family is untouched: with and without the new keyword
        _same_dict(m.predict_batch(dict(feed), kbest=K), m.predict_batch(dict(feed), kbest=K, kbest_family="projective"))
        _same_dict(m.predict_batch(dict(feed), kbest_family="nonprojective"), plain)      # kbest = 0: nothing added
        p = m.predict_batch(dict(feed), kbest=K, kbest_family="nonprojective")
        assert set(p) - set(plain) == {"kbest_heads", "kbest_count", "kbest_status", "kbest_log_prob"}
        assert p["kbest_heads"].shape == (b, K, v) and p["kbest_heads"].dtype == np.int32
        assert p["kbest_count"].shape == (b,) == p["kbest_status"].shape
        assert p["kbest_count"].dtype == np.int32 == p["kbest_status"].dtype
        assert p["kbest_log_prob"].shape == (b, K) and p["kbest_log_prob"].dtype == np.float32
        assert np.array_equal(p["heads"], plain["heads"])
        n = p["n_nodes"]
        probs = m.ops["computed_values"].numpy().reshape(b, v, o)
        s = E.tree_scores(probs, n, v)
        regular = E.decode_arrays(probs, m.ops["computed_values_edges"].numpy().reshape(b, v, -1), n)[2][:, 4] == 1
        assert not regular[0]
        heads, totals, count, status = E.tree_kbest_arrays(s, np.where(regular, n, 0), K, True)
        assert np.array_equal(p["kbest_heads"], heads) and np.array_equal(p["kbest_count"], count)
        assert np.array_equal(p["kbest_status"], np.where(regular, status, 2))
        scale = np.log(2.0) / 2.0 ** E.tree_score_shift(v)
        q = m.predict_batch(dict(feed), tree="mbr", kbest=K, kbest_family="nonprojective")   # never the marginals' scores
        assert np.array_equal(q["kbest_heads"], heads)
        tree = m.predict_batch(dict(feed), tree=True)
        for g in range(b):
            c = int(count[g])
            if not regular[g]:
                assert c == 0 and p["kbest_status"][g] == 2 and (p["kbest_heads"][g] == -1).all()
                assert (p["kbest_log_prob"][g] == -np.inf).all()
                irregular_seen += 1
                continue
            regular_seen += 1
            assert c == K and p["kbest_status"][g] == 1
            want = (totals[g, :c].astype(np.float64) * scale).astype(np.float32)
            assert np.array_equal(p["kbest_log_prob"][g, :c], want)
            assert tree["tree_status"][g] in (0, 1)
            assert np.array_equal(p["kbest_heads"][g, 0], tree["heads"][g])         # the first entry is tree=True's
        for bad in ("all", "mbr", True, None, 1):
            with pytest.raises(ValueError):
                m.predict_batch(dict(feed), kbest=K, kbest_family=bad)
    assert regular_seen > 0 and irregular_seen > 0


def test_fills_when_the_masks_are_not_in_closed_form():
    m = _synthetic_model()
    raw = _synthetic_raw()
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    feed = dict(next(iter(m.make_minibatch_iterator(data, False))))
    b, v, K = int(feed["num_graphs"]), int(feed["num_vertices"]), 2
    mask = np.array(feed["node_mask"], np.float32)
    mask.reshape(b, v, -1)[0, 1, 0] = 0.0            # not get_mask's closed form: nothing is attempted
    feed["node_mask"] = mask
    p = m.predict_batch(feed, kbest=K, kbest_family="nonprojective")
    assert (p["kbest_heads"] == -1).all() and p["kbest_heads"].shape == (b, K, v)
    assert (p["kbest_count"] == 0).all() and (p["kbest_status"] == 2).all()
    assert (p["kbest_log_prob"] == -np.inf).all() and p["kbest_log_prob"].shape == (b, K)


def test_parse_kbest_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    empty = dict(raw[0], graph=[], targets=[], node_features=[0], node_features_target=[0], words_index=[0])
    raw = raw[:3] + [empty] + raw[3:6]
    trees, log_probs = m.parse_kbest(raw, 3, family="nonprojective")
    parsed = m.parse(raw, tree=True)
    assert len(trees) == len(raw) == len(log_probs)
    for d, t, lp, one in zip(raw, trees, log_probs, parsed):
        if len(d["graph"]) == 0:
            assert t == [] and lp == []
            continue
        n = len(d["node_features"])
        assert len(t) == 3 == len(lp) and lp == sorted(lp, reverse=True) and all(np.isfinite(lp))
        assert len({tuple(h for h, _ in tree) for tree in t}) == 3
        for tree in t:
            assert len(tree) == n - 1 and E.is_tree([-1] + [a for a, _ in tree], n, True)
        assert t[0] == one                                           # parse(tree=True)'s tree, parse's form
    assert m.parse_kbest(raw[:3], 2) == m.parse_kbest(raw[:3], 2, family="projective")     # the default
    assert m.parse_kbest(raw[:3], 2, True, "projective")[0] != m.parse_kbest(raw[:3], 2, True, "nonprojective")[0]
    for bad in ("tree", None, True):
        with pytest.raises(ValueError):
            m.parse_kbest(raw, 2, family=bad)
    with pytest.raises(ValueError):
        m.parse_kbest(raw, 17, family="nonprojective")


def test_decode_chain_routes_by_family():
    from ggnn_amd.decoding import HostDecoder, decode_chain
    rng = np.random.default_rng(4)
    b, v, o, oe = 3, 7, 9, 4
    n = np.asarray([7, 5, 1], np.int32)
    probs = rng.random((b, v, o)).astype(np.float32) + 0.01
    probs_e = rng.random((b, v, oe)).astype(np.float32) + 0.01
    probs[:, :, v:] = 0
    for g in range(b):
        probs[g, n[g]:] = 0
        probs[g, :, n[g]:] = 0
        probs[g, 0] = 0
        probs[g, np.arange(v), np.arange(v)] = 0
    args = (HostDecoder(), probs, probs_e, n, None, False, True)
    default, named = decode_chain(*args, kbest=4), decode_chain(*args, kbest=4, kbest_family="projective")
    _same_dict({k: x for k, x in default.items() if x is not None}, {k: x for k, x in named.items() if x is not None})
    got = decode_chain(*args, kbest=4, kbest_family="nonprojective")
    assert set(got) == set(default)
    s = E.tree_scores(probs, n, v)
    regular = got["counts"][:, 4] == 1
    want = E.tree_kbest_arrays(s, np.where(regular, n, 0), 4, True)
    for key, a in zip(("kbest_heads", "kbest_total", "kbest_count"), want):
        assert got[key].tobytes() == a.tobytes(), key
    assert np.array_equal(got["kbest_status"], np.where(regular, want[3], 2))
    assert got["kbest_count"][0] == 4 and not np.array_equal(got["kbest_heads"], default["kbest_heads"])
    assert set(decode_chain(*args, kbest_family="nonprojective")) == set(decode_chain(*args))
    with pytest.raises(ValueError):
        decode_chain(*args, kbest=4, kbest_family="both")


def test_host_decoder_and_output_heads_rank_alike():
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    params = ("scores", "n_nodes", "K", "single_root")
    dev = inspect.signature(OutputHeads.tree_kbest).parameters
    host = inspect.signature(HostDecoder.tree_kbest).parameters
    want = ["self"] + list(params)
    assert list(dev)[:len(want)] == want and list(host) == want
    for p in params:
        assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), p
    assert dev["single_root"].default is True
    assert list(dev)[len(want):] == ["workspace"] and dev["workspace"].default is None
    assert list(dev) == list(inspect.signature(OutputHeads.projective_kbest).parameters)
    s = scores_batch([5, 1], 5, 7, "soft", 2)
    heads, totals, count, status = HostDecoder().tree_kbest(s, [5, 1], 3)
    assert all(a.dtype == np.int32 for a in (heads, totals, count, status))
    assert heads.shape == (2, 3, 5) and count.tolist() == [3, 0] and status.tolist() == [1, 0]


def test_tree_kbest_rejects_bad_arguments_without_gpu(lib):
    """ggnn_tree_kbest validates on the host before any launch; the workspace
    is the header's formula."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    need = 2 * 4 * (3 * (2 * 20 + 16) + 16)           # b = 2, v = 20, K = 3
    ok = dict(b=2, v=20, o=150, s=x, n=x, single=1, k=3, heads=x, totals=x, count=x, status=x, ws=x, ws_bytes=need)
    for change, word in ((dict(k=0), b"K must"), (dict(k=17), b"K must"), (dict(o=19), b"v 20 > o 19"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(o=1025), b"1..1024"), (dict(b=0), b">= 1"),
                         (dict(single=2), b"0 or 1"), (dict(s=None), b"NULL"), (dict(n=None), b"NULL"),
                         (dict(heads=None), b"NULL"), (dict(totals=None), b"NULL"), (dict(count=None), b"NULL"),
                         (dict(status=None), b"NULL"), (dict(ws=None), b"workspace"),
                         (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=None, ws_bytes=0), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_tree_kbest(ctypes.byref(d), a["s"], a["o"], a["n"], a["single"], a["k"], a["heads"], a["totals"],
                                 a["count"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
        assert b"tree_kbest" in lib.ggnn_last_error()
    assert lib.ggnn_tree_kbest(None, x, 150, x, 1, 3, x, x, x, x, x, need, None) == -1
    size = lib.ggnn_tree_kbest_workspace_bytes
    assert size(2, 20, 3) == need
    assert size(0, 256, 1) == 0 == size(1, 256, 0) == size(1, 256, 17) == size(1, 0, 1)
    assert all(size(b, v, K) == b * 4 * (K * (2 * v + 16) + 16) for b in (1, 7) for v in (1, 40, 256) for K in (1, 2, 16))
    assert {"ggnn_tree_kbest", "ggnn_tree_kbest_workspace_bytes"} <= set(_lib.EXPORTED)
