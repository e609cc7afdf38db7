"""Sampling projective dependency trees on the host:
evaluation.projective_sample_arrays (the host form of ggnn_projective_sample: a
top-down walk over the inside tables of the projective marginals) against
brute force over all projective trees (the forced form's probabilities are the
exact weight / Z), the contract of its samples over the table of the GPU test,
the independence of a sample from num_samples, the float32 form against the
float64 one under the explained-difference rule of
tests/projective_sample_cases.py, one small distribution, the Philox counter
layout, the model's keywords on a CPU device, the two backends' signatures and
the C ABI's validation without a GPU."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from projective_sample_cases import (ALL_LAUNCHES, CHUNK, DIFFER_SHARE, K, SEED, P, check_samples, differing, flat_five,
                                     reference, sample_reference, unexplained)
from test_projective_marginals import brute_force
from test_tree_decode import _synthetic_model, _synthetic_raw


def test_forced_probabilities_equal_brute_force():
    """n = 2..6, both root modes, 25 % zeros, three seeds: following every
    projective tree of the brute force, the product of the conditional
    probabilities is the tree's weight / Z within 1e-12 and the products sum
    to 1; a crossing tree and a non-tree have probability 0."""
    feasible = 0
    for seed in range(3):
        rng = np.random.default_rng(900 + seed)
        for n in range(2, 7):
            for single_root in (False, True):
                p = (0.05 + rng.random((n, n + 2))).astype(np.float32)
                p[rng.random(p.shape) < 0.25] = 0
                _, _, trees = brute_force(p, n, single_root)
                if not trees:
                    out = E.projective_sample_arrays(p[None], [n], 2, seed, single_root)
                    assert (out[2] == 2).all() and out[4][0] == -np.inf
                    continue
                feasible += 1
                z = sum(w for _, w in trees)
                forced = np.asarray([h for h, _ in trees])[None]
                heads, log_prob, status, _, logz = E.projective_sample_arrays(p[None], [n], len(trees), seed,
                                                                              single_root, forced=forced)
                assert (status == 1).all() and np.array_equal(heads[0, :, 1:], forced[0, :, 1:])
                assert abs(logz[0] - np.log(z)) <= 1e-12
                got = np.exp(log_prob[0])
                assert np.abs(got - np.asarray([w for _, w in trees]) / z).max() <= 1e-12, (seed, n, single_root)
                assert abs(got.sum() - 1) <= 1e-12, (seed, n, single_root)
                force = lambda h: E.projective_sample_arrays(p[None], [n], 1, seed, single_root,
                                                             forced=np.asarray([h]))[1][0, 0]
                if n >= 3:
                    assert force([-1, 2, 1] + [0] * (n - 3)) == -np.inf              # words 1 and 2 take each other
                if n >= 5:
                    crossing = [-1, 3, 4, 0, 0] + [0] * (n - 5)                      # 1 <- 3 crosses 2 <- 4
                    assert E.is_tree(crossing, n, False) and not E.is_projective(crossing, n)
                    assert force(crossing) == -np.inf
                if single_root and n >= 3:                                           # two ROOT children
                    assert force([-1] + [0] * (n - 1)) == -np.inf
    assert feasible >= 20


@pytest.mark.parametrize("single_root", [False, True], ids=["multi", "single"])
def test_table_samples_are_projective_trees_of_the_distribution(single_root):
    """Every drawn sample of the table is a projective tree over allowed arcs
    with the right root count, its log_prob is sum ln p - ln Z of
    projective_marginals_arrays to 1e-10, the statuses and logz of the n < 2
    and infeasible graphs are the marginals', a NaN and the padding's positive
    junk are never read as arcs."""
    drawn = passed = 0
    for shape, k in ALL_LAUNCHES:
        p, n, kinds, allowed, host = reference(shape, k)
        _, logz, _, m_status, _ = host[single_root]
        heads, log_prob, status, margin, s_logz = sample_reference(shape, k, single_root)
        assert heads.dtype == np.int32 and status.dtype == np.int32 and heads.shape == (shape[0], K, shape[1])
        check_samples(p, n, allowed, m_status, single_root, heads, log_prob, status)
        assert (status == m_status[:, None]).all(), (shape, k)                   # float64: no dead end
        assert np.array_equal(s_logz, logz)
        for g, s in np.argwhere(status == 1):
            m = int(n[g])
            want = np.log(p[g, np.arange(1, m), heads[g, s, 1:m]].astype(np.float64)).sum() - float(logz[g])
            assert abs(log_prob[g, s] - want) <= 1e-10, (shape, k, g, s)
            assert margin[g, s] > 0
        drawn += int((status == 1).sum())
        passed += int((status != 1).sum())
    assert drawn > 300 and passed > 100


def test_float32_form_returns_the_float64_trees():
    """The reference alone within the cap: the float32 host form returns the
    float64 form's tree on all but at most 2 % of the table's samples, and
    every differing sample is explained (its margin is below the graph's
    bar).  Measured: 0 of 824."""
    total = differ = 0
    for shape, k in ALL_LAUNCHES:
        p, n = reference(shape, k)[:2]
        for single_root in (False, True):
            span_max = reference(shape, k)[4][single_root][4]
            heads, _, status, margin, _ = sample_reference(shape, k, single_root)
            got = E.projective_sample_arrays(p, n, K, SEED, single_root, np.float32)
            assert np.array_equal(got[2], status), (shape, k, single_root)
            diff = differing(heads, got[0], status)
            bad = unexplained(diff, margin, n, span_max)
            assert not bad, (shape, k, single_root, bad)
            total += int((status == 1).sum())
            differ += int(diff.sum())
    print("float32 host form: %d of %d samples differ" % (differ, total))
    assert differ <= DIFFER_SHARE * total


def test_samples_do_not_depend_on_num_samples_and_seeds_differ():
    rng = np.random.default_rng(5)
    p = (0.05 + rng.random((3, 9, 11))).astype(np.float32)
    n = [9, 6, 2]
    for single_root in (False, True):
        four = E.projective_sample_arrays(p, n, 4, 11, single_root)
        eight = E.projective_sample_arrays(p, n, 8, 11, single_root)
        for a, c in zip(four[:4], eight[:4]):
            assert np.array_equal(a, c[:, :4])
        assert np.array_equal(four[4], eight[4])
        other = E.projective_sample_arrays(p, n, 8, 12, single_root)
        assert not np.array_equal(eight[0], other[0])
        assert len({tuple(h) for h in eight[0][0]}) > 1                # the samples of one graph differ
        assert np.array_equal(E.projective_sample_arrays(p, n, 4, 11 + 2 ** 64, single_root)[0], four[0])   # mod 2^64
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            E.projective_sample_arrays(p, n, bad, 0)


def test_flat_five_node_distribution():
    """4096 samples of the flat 5-node graph contain every projective tree of
    the brute-force list, both root modes, and nothing else."""
    p, n = flat_five()
    for single_root, count in ((False, 55), (True, 30)):
        trees = {tuple(h) for h, _ in brute_force(p[0], 5, single_root)[2]}
        assert len(trees) == count
        heads, _, status, _, _ = E.projective_sample_arrays(p, n, 4096, 3, single_root)
        assert (status == 1).all()
        assert {tuple(map(int, h)) for h in heads[0]} == trees


def test_philox_counter_layout():
    """The draw of item (kind, s, t) in sample 2 of graph 3: counter (kind <<
    16 | s << 8 | t, sample, graph, 0x50000000), key = the seed, low word
    first; a stream of its own beside ggnn_tree_sample's."""
    u = E.projective_sample_uniform(SEED, 3, 2, 4, 5, 200)
    x = E.philox4x32_10((4 << 16 | 5 << 8 | 200, 2, 3, 0x50000000), (SEED & 0xFFFFFFFF, SEED >> 32))[0]
    assert u == (x >> 8) * 2.0 ** -24 and 0 <= u < 1 and np.float32(u) == u
    assert E.PROJ_SAMPLE_STREAM == 0x50000000 != E.SAMPLE_STREAM
    assert E.philox4x32_10((0, 0, 0, 0x50000000), (0, 0))[0] == 0xb1993afb
    assert E.projective_sample_uniform(0, 0, 0, 0, 0, 0) == (0xb1993afb >> 8) * 2.0 ** -24


def test_model_keywords_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    trees, log_probs = m.sample_trees(raw, 3, family="projective")
    assert len(trees) == len(raw) == len(log_probs)
    for d, t, lp in zip(raw, trees, log_probs):
        n = len(d["node_features"])
        assert len(t) == 3 == len(lp)
        for tree, x in zip(t, lp):
            h = [-1] + [a for a, _ in tree]
            assert len(tree) == n - 1 and E.is_tree(h, n, True) and E.is_projective(h, n)
            assert x <= 0.0 and np.isfinite(x)
    assert m.sample_trees(raw, 3, family="projective") == (trees, log_probs)
    assert m.sample_trees(raw, 3) == m.sample_trees(raw, 3, family="nonprojective")      # the default: today's trees
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o = m.params["output_size"]
    for i, feed in enumerate(m.make_minibatch_iterator(data, False)):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p0 = m.predict_batch(dict(feed), samples=3, sample_seed=i)
        p = m.predict_batch(dict(feed), samples=3, sample_seed=i, sample_family="projective")
        assert set(p) == set(p0) and np.array_equal(p["heads"], p0["heads"])
        probs = m.ops["computed_values"].numpy().reshape(b, v, o)
        heads, log_prob, status, _, _ = E.projective_sample_arrays(probs, p["n_nodes"], 3, i, True)
        assert np.array_equal(p["sampled_heads"], heads) and p["sampled_heads"].dtype == np.int32
        assert np.array_equal(p["sample_log_prob"], log_prob.astype(np.float32))
        assert p["sample_log_prob"].dtype == np.float32 and np.array_equal(p["sample_status"], status)
        ref = E.tree_sample_arrays(probs, p["n_nodes"], 3, i, True)
        assert np.array_equal(p0["sampled_heads"], ref[0])
        with pytest.raises(ValueError):
            m.predict_batch(dict(feed), samples=3, sample_family="eisner")
        with pytest.raises(ValueError):
            m.predict_batch(dict(feed), sample_family=True)
    with pytest.raises(ValueError):
        m.sample_trees(raw, 3, family="all")
    from ggnn_amd.decoding import HostDecoder, decode_chain
    with pytest.raises(ValueError):
        decode_chain(HostDecoder(), None, None, None, None, False, sample_family="other")


def test_host_decoder_and_output_heads_sample_alike():
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    params = ("probs_head", "n_nodes", "num_samples", "seed", "single_root")
    dev = inspect.signature(OutputHeads.projective_sample).parameters
    host = inspect.signature(HostDecoder.projective_sample).parameters
    want = ["self"] + list(params)
    assert list(dev)[:len(want)] == want and list(host) == want
    for p in params:
        assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), p
    assert dev["seed"].default == 0 and dev["single_root"].default is True
    assert list(dev)[len(want):] == ["workspace"] and dev["workspace"].default is None
    rng = np.random.default_rng(2)
    p = rng.random((2, 5, 7)).astype(np.float32)
    heads, log_prob, status, logz = HostDecoder().projective_sample(p, [5, 1], 3)
    assert heads.dtype == np.int32 and log_prob.dtype == np.float32 and status.dtype == np.int32
    assert logz.dtype == np.float32 and logz[1] == 0
    assert heads.shape == (2, 3, 5) and (status == [[1] * 3, [0] * 3]).all() and (heads[1] == -1).all()


def test_projective_sample_rejects_bad_arguments_without_gpu(lib):
    """ggnn_projective_sample validates on the host before any launch; the
    header's constants are the binding's and the host form's."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    chunks = -(-3 // CHUNK)
    need = 2 * chunks * 8 * (P + 1) * (P + 2)         # b = 2, K = 3, v = P + 1
    ok = dict(b=2, v=30, o=150, p=x, n=x, single=1, k=3, heads=x, lp=x, status=x, logz=x, ws=None, ws_bytes=0)
    for change, word in ((dict(k=0), b"num_samples"), (dict(k=4097), b"num_samples"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(o=1025), b"1..1024"), (dict(b=0), b">= 1"),
                         (dict(single=2), b"0 or 1"), (dict(p=None), b"NULL"), (dict(n=None), b"NULL"),
                         (dict(heads=None), b"NULL"), (dict(lp=None), b"NULL"), (dict(status=None), b"NULL"),
                         (dict(v=P + 1, o=256), b"workspace"),
                         (dict(v=P + 1, o=256, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=P + 1, o=256, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_projective_sample(ctypes.byref(d), a["p"], a["o"], a["n"], a["single"], a["k"], 7, a["heads"],
                                        a["lp"], a["status"], a["logz"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
        assert b"projective_sample" in lib.ggnn_last_error()
    assert lib.ggnn_projective_sample(None, x, 150, x, 1, 3, 7, x, x, x, x, None, 0, None) == -1
    size = lib.ggnn_projective_sample_workspace_bytes
    assert size(2, P + 1, 3) == need
    assert size(256, P, 4096) == 0
    assert size(0, 256, 1) == 0 == size(1, 256, 0)
    assert size(3, 256, CHUNK) == 3 * 8 * 256 * 257 and size(3, 256, CHUNK + 1) == 2 * 3 * 8 * 256 * 257
    assert {"ggnn_projective_sample", "ggnn_projective_sample_workspace_bytes"} <= set(_lib.EXPORTED)
    header = (Path(__file__).resolve().parents[1] / "include" / "ggnn.h").read_text()
    const = lambda name: int(re.search(r"#define %s (\d+)" % name, header).group(1))
    assert const("GGNN_PROJ_SAMPLE_LDS_MAXN") == P == _lib.PROJ_SAMPLE_LDS_MAXN == E.PROJ_SAMPLE_LDS_MAXN
    assert const("GGNN_PROJ_SAMPLE_CHUNK") == CHUNK == _lib.PROJ_SAMPLE_CHUNK == E.PROJ_SAMPLE_CHUNK
    assert P == _lib.PROJ_LDS_MAXN                    # the projective decode's tier: the same four tables
