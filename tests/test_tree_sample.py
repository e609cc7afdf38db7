"""Sampling dependency trees on the host: evaluation.tree_sample_arrays (the
host form of ggnn_tree_sample: conditional sampling on the matrix-tree inverse)
against brute force over all trees (the forced form's probabilities are the
exact weight / Z), the contract of its samples over the table of the GPU test,
the float32 form against the float64 one under the explained-difference rule of
tests/tree_sample_cases.py, the independence of a sample from num_samples, the
host Philox against Random123's known answers, the model's sample_trees /
predict_batch(samples=) on a CPU device, the two backends' signatures and the C
ABI's validation without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from ggnn_amd._lib import SAMPLE_LDS_MAXN as L
from test_tree_decode import _synthetic_model, _synthetic_raw
from test_tree_marginals import brute_force
from tree_sample_cases import (ALL_LAUNCHES, DIFFER_SHARE, K, PHILOX_KAT, SEED, check_samples, differing, reference,
                               sample_reference, unexplained)


def test_forced_probabilities_equal_brute_force():
    """n = 2..6, both root modes, 25 % zeros, three seeds: following every tree
    of the brute force, the product of the conditional probabilities is the
    tree's weight / Z within 1e-12 and the products sum to 1; a head vector
    that is no tree of the distribution has probability 0."""
    feasible = 0
    for seed in range(3):
        rng = np.random.default_rng(700 + seed)
        for n in range(2, 7):
            for single_root in (False, True):
                p = (0.05 + rng.random((n, n + 2))).astype(np.float32)
                p[rng.random(p.shape) < 0.25] = 0
                _, _, trees = brute_force(p, n, single_root)
                if not trees:
                    assert (E.tree_sample_arrays(p[None], [n], 2, seed, single_root)[2] == 2).all()
                    continue
                feasible += 1
                z = sum(w for _, w in trees)
                forced = np.asarray([h for h, _ in trees])[None]
                heads, log_prob, status, _ = E.tree_sample_arrays(p[None], [n], len(trees), seed, single_root,
                                                                  forced=forced)
                assert (status == 1).all() and np.array_equal(heads[0, :, 1:], forced[0, :, 1:])
                got = np.exp(log_prob[0])
                assert np.abs(got - np.asarray([w for _, w in trees]) / z).max() <= 1e-12, (seed, n, single_root)
                assert abs(got.sum() - 1) <= 1e-12, (seed, n, single_root)
                if n >= 3:
                    bad = np.zeros((1, n), np.int64)
                    bad[0, 1], bad[0, 2] = 2, 1                         # words 1 and 2 take each other
                    assert E.tree_sample_arrays(p[None], [n], 1, seed, single_root, forced=bad)[1][0, 0] == -np.inf
                    if single_root:                                     # two ROOT children
                        assert E.tree_sample_arrays(p[None], [n], 1, seed, True,
                                                    forced=np.zeros((1, n), np.int64))[1][0, 0] == -np.inf
    assert feasible >= 20


@pytest.mark.parametrize("single_root", [False, True], ids=["multi", "single"])
def test_table_samples_are_trees_of_the_distribution(single_root):
    """Every drawn sample of the table is a tree over allowed arcs with the
    right root count, its log_prob is sum ln p - ln Z of tree_marginals_arrays
    to 1e-10, the statuses of the n < 2 and infeasible graphs pass through, a
    NaN and the padding's positive junk are never read as arcs."""
    drawn = passed = 0
    for shape, k in ALL_LAUNCHES:
        p, n, kinds, allowed, host = reference(shape, k)
        _, logz, _, m_status, _ = host[single_root]
        heads, log_prob, status, margin = sample_reference(shape, k, single_root)
        assert heads.dtype == np.int32 and status.dtype == np.int32 and heads.shape == (shape[0], K, shape[1])
        check_samples(p, n, allowed, m_status, single_root, heads, log_prob, status)
        assert ((status == 1) == (m_status == 1)[:, None]).all(), (shape, k)     # float64: no dead end
        for g, s in np.argwhere(status == 1):
            m = int(n[g])
            want = np.log(p[g, np.arange(1, m), heads[g, s, 1:m]].astype(np.float64)).sum() - float(logz[g])
            assert abs(log_prob[g, s] - want) <= 1e-10, (shape, k, g, s)
            assert margin[g, s] > 0
        drawn += int((status == 1).sum())
        passed += int((status != 1).sum())
    assert drawn > 400 and passed > 100


def test_float32_form_returns_the_float64_trees():
    """The gate on the inputs: the float32 host form returns the float64 form's
    tree on all but at most 2 % of the table's samples, and every differing
    sample is explained (its margin is below the graph's bar).  Measured: 1 of
    1124, margin 1.8e-7 against a bar of 9.1e-3."""
    total = differ = 0
    for shape, k in ALL_LAUNCHES:
        p, n = reference(shape, k)[:2]
        for single_root in (False, True):
            cond = reference(shape, k)[4][single_root][4]
            heads, _, status, margin = sample_reference(shape, k, single_root)
            got = E.tree_sample_arrays(p, n, K, SEED, single_root, np.float32)
            assert np.array_equal(got[2], status), (shape, k, single_root)
            diff = differing(heads, got[0], status)
            assert not unexplained(diff, margin, n, cond), (shape, k, single_root, unexplained(diff, margin, n, cond))
            total += int((status == 1).sum())
            differ += int(diff.sum())
    print("float32 host form: %d of %d samples differ" % (differ, total))
    assert differ <= DIFFER_SHARE * total


def test_samples_do_not_depend_on_num_samples_and_seeds_differ():
    rng = np.random.default_rng(5)
    p = (0.05 + rng.random((3, 9, 11))).astype(np.float32)
    n = [9, 6, 2]
    for single_root in (False, True):
        four = E.tree_sample_arrays(p, n, 4, 11, single_root)
        eight = E.tree_sample_arrays(p, n, 8, 11, single_root)
        for a, c in zip(four, eight):
            assert np.array_equal(a, c[:, :4])
        other = E.tree_sample_arrays(p, n, 8, 12, single_root)
        assert not np.array_equal(eight[0], other[0])
        assert len({tuple(h) for h in eight[0][0]}) > 1                # the samples of one graph differ
        assert np.array_equal(E.tree_sample_arrays(p, n, 4, 11 + 2 ** 64, single_root)[0], four[0])   # mod 2^64
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            E.tree_sample_arrays(p, n, bad, 0)


def test_host_philox_known_answers():
    for counter, key, want in PHILOX_KAT:
        assert E.philox4x32_10(counter, key) == want
    u = E.sample_uniform(SEED, 3, 2, 1)
    x = E.philox4x32_10((1, 2, 3, 0x40000000), (SEED & 0xFFFFFFFF, SEED >> 32))[0]
    assert u == (x >> 8) * 2.0 ** -24 and 0 <= u < 1 and np.float32(u) == u


def test_model_sample_trees_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    plain = m.parse(raw)
    trees, log_probs = m.sample_trees(raw, 3)
    assert len(trees) == len(raw) == len(log_probs)
    for d, a, t, lp in zip(raw, plain, trees, log_probs):
        n = len(d["node_features"])
        assert len(t) == 3 == len(lp)
        for tree, x in zip(t, lp):
            assert len(tree) == n - 1 and E.is_tree([-1] + [h for h, _ in tree], n, True)
            assert [l for _, l in tree] == [l for _, l in a]            # the labels: the arg-max's
            assert x <= 0.0 and np.isfinite(x)
    assert m.sample_trees(raw, 3) == (trees, log_probs)
    assert m.sample_trees(raw, 3, seed=1)[0] != trees
    multi = m.sample_trees(raw, 2, single_root=False)[0]
    assert all(E.is_tree([-1] + [h for h, _ in tree], len(d["node_features"]), False)
               for d, t in zip(raw, multi) for tree in t)
    assert m.sample_trees([], 2) == ([], [])
    # predict_batch: samples = 0 returns today's keys, K > 0 the host form's arrays on the fetched probabilities
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)   # (as sample_trees numbers them)
    o = m.params["output_size"]
    for i, feed in enumerate(m.make_minibatch_iterator(data, False)):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p0 = m.predict_batch(dict(feed), samples=0)
        assert set(p0) == {"heads", "labels", "n_nodes", "sentences_id", "tree_status"}
        p = m.predict_batch(dict(feed), samples=3, sample_seed=i)
        assert set(p) == set(p0) | {"sampled_heads", "sample_log_prob", "sample_status"}
        assert np.array_equal(p["heads"], p0["heads"])
        probs = m.ops["computed_values"].numpy().reshape(b, v, o)
        heads, log_prob, status, _ = E.tree_sample_arrays(probs, p["n_nodes"], 3, i, True)
        assert np.array_equal(p["sampled_heads"], heads) and p["sampled_heads"].dtype == np.int32
        assert np.array_equal(p["sample_log_prob"], log_prob.astype(np.float32))
        assert p["sample_log_prob"].dtype == np.float32 and np.array_equal(p["sample_status"], status)
        with_mbr = m.predict_batch(dict(feed), tree="mbr", samples=3, sample_seed=i)
        assert np.array_equal(with_mbr["sampled_heads"], heads)
        for g, k in enumerate(p["sentences_id"]):                       # batch i of sample_trees drew with seed + i
            n = int(p["n_nodes"][g])
            assert [[h for h, _ in tree] for tree in trees[k]] == [list(map(int, x[1:n])) for x in heads[g]]
    with pytest.raises(ValueError):
        m.predict_batch(dict(feed), samples=-1)


def test_host_decoder_and_output_heads_sample_alike():
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    params = ("probs_head", "n_nodes", "num_samples", "seed", "single_root", "marginals")
    dev = inspect.signature(OutputHeads.tree_sample).parameters
    host = inspect.signature(HostDecoder.tree_sample).parameters
    want = ["self"] + list(params)
    assert list(dev)[:len(want)] == want and list(host) == want
    for p in params:
        assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), p
    assert dev["seed"].default == 0 and dev["single_root"].default is True and dev["marginals"].default is None
    assert list(dev)[len(want):] == ["workspace"] and dev["workspace"].default is None
    rng = np.random.default_rng(2)
    p = rng.random((2, 5, 7)).astype(np.float32)
    heads, log_prob, status = HostDecoder().tree_sample(p, [5, 1], 3)
    assert heads.dtype == np.int32 and log_prob.dtype == np.float32 and status.dtype == np.int32
    assert heads.shape == (2, 3, 5) and (status == [[1] * 3, [0] * 3]).all() and (heads[1] == -1).all()


def test_tree_sample_rejects_bad_arguments_without_gpu(lib):
    """ggnn_tree_sample validates on the host before any launch."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    need = 2 * 3 * 4 * L * (L | 1)                    # b = 2, K = 3, v = L + 1
    ok = dict(b=2, v=30, o=150, p=x, n=x, single=1, marg=x, logz=x, mstat=x, k=3, heads=x, lp=x, status=x, ws=None,
              ws_bytes=0)
    for change, word in ((dict(k=0), b"num_samples"), (dict(k=4097), b"num_samples"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(marg=None), b"marg"),
                         (dict(o=1025), b"1..1024"), (dict(b=0), b">= 1"), (dict(single=2), b"0 or 1"),
                         (dict(p=None), b"NULL"), (dict(n=None), b"NULL"), (dict(logz=None), b"NULL"),
                         (dict(mstat=None), b"NULL"), (dict(heads=None), b"NULL"), (dict(lp=None), b"NULL"),
                         (dict(status=None), b"NULL"),
                         (dict(v=L + 1, o=256), b"workspace"),
                         (dict(v=L + 1, o=256, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=L + 1, o=256, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_tree_sample(ctypes.byref(d), a["p"], a["o"], a["n"], a["single"], a["marg"], a["logz"],
                                  a["mstat"], a["k"], 7, a["heads"], a["lp"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
        assert b"tree_sample" in lib.ggnn_last_error()
    assert lib.ggnn_tree_sample(None, x, 150, x, 1, x, x, x, 3, 7, x, x, x, None, 0, None) == -1
    assert lib.ggnn_tree_sample_workspace_bytes(2, L + 1, 3) == need
    assert lib.ggnn_tree_sample_workspace_bytes(256, L, 4096) == 0
    assert lib.ggnn_tree_sample_workspace_bytes(0, 256, 1) == 0 == lib.ggnn_tree_sample_workspace_bytes(1, 256, 0)
    assert lib.ggnn_tree_sample_workspace_bytes(3, 256, 2) == 3 * 2 * 4 * 255 * 255
    assert {"ggnn_tree_sample", "ggnn_tree_sample_workspace_bytes"} <= set(_lib.EXPORTED)
    assert L == E.SAMPLE_LDS_MAXN == _lib.LAPL_LDS_MAXN and _lib.SAMPLE_MAX == E.SAMPLE_MAX == 4096
