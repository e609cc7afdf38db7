"""The host form of ggnn_projective_kbest (evaluation.projective_kbest_arrays)
against brute-force enumeration (n = 2..6, both root modes, 25 % forbidden
arcs, tree_scores scores and a tie-heavy copy, K = 1, 3, 8, 16), rank 0 against
_eisner bit for bit, the prefix property, the edge statuses, garbage in the
padding, the model's kbest keyword and parse_kbest on a CPU device through
HostDecoder, the two backends' signatures, the library's host-side checks and
the header's constants."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from ggnn_amd import evaluation as E
from projective_kbest_cases import F, KINDS, brute_force, lds_maxn, scores_batch, with_garbage
from test_tree_decode import _synthetic_model, _synthetic_raw

KS = (1, 3, 8, 16)


def _small_cases():
    for n in range(2, 7):
        for kind in ("forbid", "ties"):
            for rep in range(3):
                yield n, kind, scores_batch([n], 7, 8, kind, 1000 * n + 10 * rep + KINDS.index(kind))


def test_host_form_equals_brute_force_and_eisner():
    cases = fewer = none = tied = 0
    for n, kind, s in _small_cases():
        for single_root in (True, False):
            trees = brute_force(s[0], n, single_root)
            want = sorted((t for t, _ in trees), reverse=True)
            best = E._eisner(s[0], n, single_root)
            tied += len(set(want)) < len(want)
            for K in KS:
                heads, totals, count, status = E.projective_kbest_arrays(s, [n], K, single_root)
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
                    assert E.is_tree(h, n, single_root, s[0]) and E.is_projective(h, n)
                    assert E.tree_total(s[0], h, n) == totals[0, r]
                if best is None:
                    assert status[0] == 2 and c == 0
                else:
                    assert heads[0, 0, :n].tolist() == best          # ties included
                cases += 1
                fewer += 0 < len(trees) < K
                none += not trees
    assert cases == 240 and fewer > 0 and none > 0 and tied > 0, (cases, fewer, none, tied)


def test_k4_is_a_prefix_of_k16():
    ns = [6, 5, 9, 12]
    for kind in KINDS:
        s = scores_batch(ns, 12, 12, kind, 7)
        for single_root in (True, False):
            a = E.projective_kbest_arrays(s, ns, 4, single_root)
            c = E.projective_kbest_arrays(s, ns, 16, single_root)
            assert np.array_equal(a[0], c[0][:, :4]) and np.array_equal(a[1], c[1][:, :4])
            assert np.array_equal(a[2], np.minimum(c[2], 4)) and np.array_equal(a[3], c[3])
            assert (c[2] > 4).any()
            live = c[1].astype(np.int64)[:, :-1][c[1][:, 1:] != F]
            assert (live >= c[1].astype(np.int64)[:, 1:][c[1][:, 1:] != F]).all()       # best first


def test_edge_statuses_and_bad_arguments():
    s = scores_batch([1, 0, 4, 4, 2], 5, 6, "soft", 3)
    s[3, 2, 1] = -(2 ** 30 - 1)                     # |S| * (n - 1) >= 2^30
    heads, totals, count, status = E.projective_kbest_arrays(s, [1, 0, 4, 4, 2], 3)
    assert status.tolist() == [0, 0, 1, 2, 1] and count.tolist() == [0, 0, 3, 0, 1]
    assert (heads[[0, 1, 3]] == -1).all() and (totals[[0, 1, 3]] == F).all()
    assert heads[4, 0].tolist() == [-1, 0, -1, -1, -1] and totals[4, 0] == s[4, 1, 0]
    s[3, 2, 1] = 2 ** 30 // 3 - 1                   # the largest score a 4-node graph may hold
    assert E.projective_kbest_arrays(s, [1, 0, 4, 4, 2], 3)[3][3] == 1
    for bad in (dict(K=0), dict(K=17), dict(scores=s.astype(np.int64)), dict(scores=s[:, :, :4]), dict(n_nodes=[1, 2])):
        with pytest.raises(ValueError):
            E.projective_kbest_arrays(**dict(dict(scores=s, n_nodes=[1, 0, 4, 4, 2], K=2), **bad))


def test_garbage_in_the_padding_changes_nothing():
    ns = [3, 1, 6, 8, 5]
    for kind in KINDS:
        s = scores_batch(ns, 8, 10, kind, 11)
        dirty = with_garbage(s, ns)
        assert not np.array_equal(s, dirty)
        for single_root in (True, False):
            for a, c in zip(E.projective_kbest_arrays(s, ns, 8, single_root),
                            E.projective_kbest_arrays(dirty, ns, 8, single_root)):
                assert a.tobytes() == c.tobytes()


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


def test_model_keywords_on_a_cpu_device():
    m = _irregular_first_graph(_synthetic_model())
    raw = _synthetic_raw()
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o, K = m.params["output_size"], 5
    regular_seen = irregular_seen = 0
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        plain = m.predict_batch(dict(feed))
        assert not any(k.startswith("kbest") for k in plain)
        assert set(m.predict_batch(dict(feed), kbest=0)) == set(plain)
        p = m.predict_batch(dict(feed), kbest=K)
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
        heads, totals, count, status = E.projective_kbest_arrays(s, np.where(regular, n, 0), K, True)
        assert np.array_equal(p["kbest_heads"], heads) and np.array_equal(p["kbest_count"], count)
        assert np.array_equal(p["kbest_status"], np.where(regular, status, 2))
        scale = np.log(2.0) / 2.0 ** E.tree_score_shift(v)
        proj = m.predict_batch(dict(feed), tree="projective")
        for mode in ("projective", "projective-mbr", "mbr", True):      # never an MBR mode's marginal scores
            q = m.predict_batch(dict(feed), tree=mode, kbest=K)
            assert np.array_equal(q["kbest_heads"], heads) and np.array_equal(q["heads"],
                                                                              m.predict_batch(dict(feed), tree=mode)["heads"])
        for g in range(b):
            c = int(count[g])
            if not regular[g]:
                assert c == 0 and p["kbest_status"][g] == 2 and (p["kbest_heads"][g] == -1).all()
                assert (p["kbest_log_prob"][g] == -np.inf).all()
                irregular_seen += 1
                continue
            regular_seen += 1
            assert 1 <= c <= K and p["kbest_status"][g] == 1 and (p["kbest_log_prob"][g, c:] == -np.inf).all()
            want = (totals[g, :c].astype(np.float64) * scale).astype(np.float32)
            assert np.array_equal(p["kbest_log_prob"][g, :c], want)
            # rank 0 against tree="projective": totals, not heads (the arg-max may differ among equals)
            assert proj["tree_status"][g] in (0, 1)
            best = np.float32(E.tree_total(s[g], proj["heads"][g], int(n[g])) * scale)
            assert p["kbest_log_prob"][g, 0] == best
        for bad in (-1, 17):
            with pytest.raises(ValueError):
                m.predict_batch(dict(feed), kbest=bad)
    assert regular_seen > 0 and irregular_seen > 0


def test_parse_kbest_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    empty = dict(raw[0], graph=[], targets=[], node_features=[0], node_features_target=[0], words_index=[0])
    raw = raw[:3] + [empty] + raw[3:8]
    trees, log_probs = m.parse_kbest(raw, 4)
    parsed = m.parse(raw, tree="projective")
    assert len(trees) == len(raw) == len(log_probs)
    for d, t, lp, one in zip(raw, trees, log_probs, parsed):
        if len(d["graph"]) == 0:
            assert t == [] and lp == []
            continue
        n = len(d["node_features"])
        assert len(t) == 4 == len(lp) and lp == sorted(lp, reverse=True) and all(np.isfinite(lp))
        assert len({tuple(h for h, _ in tree) for tree in t}) == 4
        for tree in t:
            h = [-1] + [a for a, _ in tree]
            assert len(tree) == n - 1 and E.is_tree(h, n, True) and E.is_projective(h, n)
            assert [x[1] for x in tree] == [x[1] for x in one]           # parse's labels, parse's form
    assert m.parse_kbest(raw, 4) == (trees, log_probs)
    multi, _ = m.parse_kbest(raw[:3], 2, single_root=False)
    assert all(E.is_tree([-1] + [a for a, _ in tree], len(d["node_features"]), False)
               for d, t in zip(raw[:3], multi) for tree in t)
    with pytest.raises(ValueError):
        m.parse_kbest(raw, 17)


def test_host_decoder_and_output_heads_rank_alike():
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    params = ("scores", "n_nodes", "K", "single_root")
    dev = inspect.signature(OutputHeads.projective_kbest).parameters
    host = inspect.signature(HostDecoder.projective_kbest).parameters
    want = ["self"] + list(params)
    assert list(dev)[:len(want)] == want and list(host) == want
    for p in params:
        assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), p
    assert dev["single_root"].default is True
    assert list(dev)[len(want):] == ["workspace"] and dev["workspace"].default is None
    s = scores_batch([5, 1], 5, 7, "soft", 2)
    heads, totals, count, status = HostDecoder().projective_kbest(s, [5, 1], 3)
    assert all(a.dtype == np.int32 for a in (heads, totals, count, status))
    assert heads.shape == (2, 3, 5) and count.tolist() == [3, 0] and status.tolist() == [1, 0]


def test_projective_kbest_rejects_bad_arguments_without_gpu(lib):
    """ggnn_projective_kbest validates on the host before any launch; the
    header's constants are the binding's and the host form's."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    P = lib.ggnn_projective_kbest_lds_maxn(3)
    need = 2 * 2 * (P + 1) * (P + 2) * (6 * 3 + 2)    # b = 2, K = 3, v = P + 1
    ok = dict(b=2, v=20, o=150, s=x, n=x, single=1, k=3, heads=x, totals=x, count=x, status=x, ws=None, ws_bytes=0)
    for change, word in ((dict(k=0), b"K must"), (dict(k=17), b"K must"), (dict(o=19), b"v 20 > o 19"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(o=1025), b"1..1024"), (dict(b=0), b">= 1"),
                         (dict(single=2), b"0 or 1"), (dict(s=None), b"NULL"), (dict(n=None), b"NULL"),
                         (dict(heads=None), b"NULL"), (dict(totals=None), b"NULL"), (dict(count=None), b"NULL"),
                         (dict(status=None), b"NULL"), (dict(v=P + 1, o=256), b"workspace"),
                         (dict(v=P + 1, o=256, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=P + 1, o=256, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_projective_kbest(ctypes.byref(d), a["s"], a["o"], a["n"], a["single"], a["k"], a["heads"],
                                       a["totals"], a["count"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
        assert b"projective_kbest" in lib.ggnn_last_error()
    assert lib.ggnn_projective_kbest(None, x, 150, x, 1, 3, x, x, x, x, None, 0, None) == -1
    size, maxn = lib.ggnn_projective_kbest_workspace_bytes, lib.ggnn_projective_kbest_lds_maxn
    assert size(2, P + 1, 3) == need and size(256, P, 3) == 0
    assert size(0, 256, 1) == 0 == size(1, 256, 0) == size(1, 256, 17)
    assert size(3, 256, 2) == 3 * 2 * 256 * 257 * 14
    assert [maxn(k) for k in (1, 2, 16)] == [97, 73, 27] and maxn(0) == 0 == maxn(17)
    assert all(maxn(k) == lds_maxn(k) for k in range(1, 17))
    assert all(maxn(k) >= maxn(k + 1) for k in range(1, 16))
    assert {"ggnn_projective_kbest", "ggnn_projective_kbest_workspace_bytes",
            "ggnn_projective_kbest_lds_maxn"} <= set(_lib.EXPORTED)
    header = (Path(__file__).resolve().parents[1] / "include" / "ggnn.h").read_text()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert const("GGNN_KBEST_MAX") == 16 == _lib.KBEST_MAX == E.KBEST_MAX
