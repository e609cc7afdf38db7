"""Projective arc marginals on the host: evaluation.projective_marginals_arrays
(the host form of ggnn_projective_marginals, an inside and an explicit outside
pass in log space) against brute force over all head vectors, its invariants
(row sums, ROOT column, d logZ / d ln psi = marginal), the MBR tree of its
integer scores, its float32 form against the error bar of the GPU test, the
model's tree="projective-mbr" / confidence keywords on a CPU device and the C
ABI's validation without a GPU.  The case builders and the bar are shared with
tests/test_gpu_projective_marginals.py."""
import ctypes
import itertools

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from test_projective_decode import only_crossing_tree
from test_tree_decode import F, _synthetic_model, _synthetic_raw, closed_group, forbidden_row

SCALE = 2.0 ** 20


# ------------------------------------------------------------ case builders
def probs_of_scores(s, o=None):
    """Probabilities whose allowed arcs are those of integer scores [n, n]:
    2^(s / 4) / 64 where s is allowed, 0 elsewhere; float32 [n, o]."""
    n = s.shape[0]
    p = np.zeros((n, n if o is None else o), np.float32)
    p[:, :n] = np.where(s == F, 0, np.exp2(np.where(s == F, 0, s) / 4.0) / 64)
    return p


def random_probs(n, o, kind, rng):
    """One graph's float32 [n, o] head probabilities of the issue's kinds."""
    u = rng.random((n, o))
    if kind == "flat":
        p = u
    elif kind == "sparse":
        p = np.where(rng.random((n, o)) < 0.25, 0, u)
    elif kind == "peaked":
        p = 0.05 * u
        h = E.random_projective_heads(n, rng)
        p[np.arange(1, n), h[1:]] = 0.9
    elif kind == "tiny":
        p = u ** 40 + 1e-38
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def brute_force(p, n, single_root):
    """(ln Z, marginals [n, n], the projective trees as (heads, weight)) over
    all n^(n-1) head vectors, float64; (None, None, []) without a tree."""
    s = E.tree_scores(p[None], [n], n)[0]
    trees = []
    for hv in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hv)
        if E.is_tree(h, n, single_root, s) and E.is_projective(h, n):
            trees.append((h, float(np.prod([float(p[i, h[i]]) for i in range(1, n)], dtype=np.float64))))
    if not trees:
        return None, None, []
    z = sum(w for _, w in trees)
    m = np.zeros((n, n))
    for h, w in trees:
        for i in range(1, n):
            m[i, h[i]] += w
    return np.log(z), m / z, trees


def marg_bar(n, span_max):
    """The issue's error bar of a marginal at fp32 tables: 4 n (log2 n + 4 +
    span_max) 2^-24 (a quarter of it for ln Z)."""
    return 4 * n * (np.log2(n) + 4 + span_max) * 2.0 ** -24


def check_passthrough(p, out, g=0):
    marg, logz, scores, status, _ = out
    assert status[g] in (0, 2)
    assert marg[g].astype(np.float32).tobytes() == np.asarray(p, np.float32).tobytes()
    assert (scores[g] == F).all()


# ------------------------------------------------------------------ the tests
def test_random_cases_equal_brute_force():
    rng = np.random.default_rng(31)
    cases = feasible = infeasible = 0
    for case in range(160):
        n = 2 + case % 5                                              # every n in 2..6
        single_root = bool((case // 5) & 1)
        o = n + (case % 3)
        p = rng.random((n, o)).astype(np.float32)
        p[rng.random((n, o)) < 0.25] = 0
        logz, m, _ = brute_force(p, n, single_root)
        out = E.projective_marginals_arrays(p[None], [n], single_root)
        marg, lz, scores, status, span_max = out
        assert marg.dtype == np.float64 and scores.dtype == np.int32 and status.dtype == np.int32
        cases += 1
        if logz is None:
            infeasible += 1
            assert status[0] == 2 and lz[0] == -np.inf
            check_passthrough(p, out)
            continue
        feasible += 1
        assert status[0] == 1
        assert abs(lz[0] - logz) <= 1e-12
        assert np.abs(marg[0, :n, :n] - m).max() <= 1e-12
        allowed = E.tree_scores(p[None], [n], n)[0] != F
        assert (marg[0][~allowed] == 0).all() and (scores[0][~allowed] == F).all()
        assert np.array_equal(scores[0][allowed], np.rint(marg[0][allowed].astype(np.float32) * SCALE).astype(np.int32))
        assert np.isfinite(span_max[0]) and span_max[0] >= 0
    assert cases >= 100 and feasible >= 100 and infeasible >= 5, (cases, feasible, infeasible)


@pytest.mark.parametrize("single_root", [False, True])
@pytest.mark.parametrize("case", [only_crossing_tree, closed_group, forbidden_row])
def test_cases_without_a_projective_tree(case, single_root):
    for n in (5, 6):
        p = probs_of_scores(case(n), n + 3)
        p[0, :] = 0.5                                                 # row 0, columns >= n: never arcs
        p[:, n:] = 0.25
        assert brute_force(p, n, single_root)[0] is None
        out = E.projective_marginals_arrays(p[None], [n], single_root)
        assert out[3][0] == 2 and out[1][0] == -np.inf
        check_passthrough(p, out)


def test_n_below_two_nan_and_padding():
    rng = np.random.default_rng(5)
    p = rng.random((3, 6, 8)).astype(np.float32)
    p[2, 2, 1] = np.nan                                               # an arc that is simply not allowed
    p[2, 4:, :] = np.inf                                              # rows >= n are never read
    out = E.projective_marginals_arrays(p, [1, 0, 4], True)
    marg, logz, scores, status, _ = out
    assert status.tolist() == [0, 0, 1] and logz[0] == 0 and logz[1] == 0
    check_passthrough(p[0], out, 0)
    check_passthrough(p[1], out, 1)
    assert np.isfinite(marg[2]).all() and marg[2, 2, 1] == 0 and scores[2, 2, 1] == F
    assert (marg[2, 4:] == 0).all() and (marg[2, :, 4:] == 0).all() and (marg[2, 0] == 0).all()
    q = np.where(np.isfinite(p[2, :4, :4]), p[2, :4, :4], 0)
    lz, m, _ = brute_force(q, 4, True)
    assert abs(logz[2] - lz) <= 1e-12 and np.abs(marg[2, :4, :4] - m).max() <= 1e-12
    with pytest.raises(ValueError):
        E.projective_marginals_arrays(p[:, :, :5], [1, 0, 4])         # v > o
    with pytest.raises(ValueError):
        E.projective_marginals_arrays(p, [1, 0])


@pytest.mark.parametrize("single_root", [False, True])
@pytest.mark.parametrize("n", [12, 40])
def test_invariants(n, single_root):
    rng = np.random.default_rng(100 + n)
    for kind in ("flat", "sparse", "peaked", "tiny"):
        p = random_probs(n, n + 5, kind, rng)
        marg, logz, scores, status, _ = E.projective_marginals_arrays(p[None], [n], single_root)
        assert status[0] == 1
        assert np.abs(marg[0, 1:n].sum(axis=1) - 1).max() <= 1e-10
        assert (marg[0] >= 0).all() and (marg[0] <= 1).all()
        if single_root:
            assert abs(marg[0, :, 0].sum() - 1) <= 1e-10
        # d ln Z / d ln psi(arc) = marg(arc): a central difference, step 1e-6.  (p is float32; the step is
        # taken on a float64 copy of the potentials through the inside-outside routine itself.)
        psi, ok = E._arc_log_potentials(p, n, np.dtype(np.float64))
        arcs = np.argwhere(ok)
        for i, j in arcs[rng.choice(len(arcs), 5, replace=False)]:
            z = []
            for step in (1e-6, -1e-6):
                q = psi.copy()
                q[i, j] += step
                z.append(E._inside_outside(q, n, single_root)[0])
            assert abs((z[0] - z[1]) / 2e-6 - marg[0, i, j]) <= 1e-7, (kind, i, j)


def test_the_mbr_tree_of_the_integer_scores():
    rng = np.random.default_rng(77)
    checked = 0
    for case in range(60):
        n = 3 + case % 4                                              # 3..6
        single_root = bool((case // 4) & 1)
        p = rng.random((n, n)).astype(np.float32)
        p[rng.random((n, n)) < 0.2] = 0
        marg, _, scores, status, _ = E.projective_marginals_arrays(p[None], [n], single_root)
        if status[0] != 1:
            continue
        _, _, trees = brute_force(p, n, single_root)
        best = max(sum(marg[0, i, h[i]] for i in range(1, n)) for h, _ in trees)
        assert np.abs(scores[0][scores[0] != F]).max() * (n - 1) < 2 ** 30    # the projective pass's range rule
        pred = np.full((1, n, 2), -1, np.int32)                       # no tree: Eisner always runs
        out, _, st = E.projective_decode_arrays(scores, [n], pred, single_root)
        assert st[0] == 1
        h = out[0, :, 0]
        assert E.is_tree(h, n, single_root, scores[0]) and E.is_projective(h, n)
        assert sum(marg[0, i, h[i]] for i in range(1, n)) >= best - n * 2.0 ** -20
        checked += 1
    assert checked >= 40


@pytest.mark.parametrize("n", [12, 40, 97, 129])
def test_float32_host_form_stays_within_the_bar(n):
    rng = np.random.default_rng(200 + n)
    for kind in ("flat", "peaked", "tiny"):
        p = random_probs(n, n, kind, rng)
        ref = E.projective_marginals_arrays(p[None], [n], True)
        got = E.projective_marginals_arrays(p[None], [n], True, np.float32)
        assert got[0].dtype == np.float32 and ref[3][0] == 1 and got[3][0] == 1
        bar = marg_bar(n, ref[4][0])
        err = np.abs(got[0].astype(np.float64) - ref[0]).max()
        print(n, kind, "marg err", err, "bar", bar, "logz err", abs(float(got[1][0]) - ref[1][0]))
        assert err <= bar and abs(float(got[1][0]) - ref[1][0]) <= bar / 4


def test_arc_confidence_arrays():
    rng = np.random.default_rng(3)
    marg = rng.random((2, 5, 7))
    pred = np.full((2, 5, 2), -1, np.int32)
    pred[0, :, 0] = [3, 2, 0, -1, 1]
    pred[1, :, 0] = [0, 0, 1, 2, 3]
    conf = E.arc_confidence_arrays(marg, [5, 3], pred)
    assert conf.dtype == np.float32 and conf.shape == (2, 5)
    assert conf[0].tolist() == [0, np.float32(marg[0, 1, 2]), np.float32(marg[0, 2, 0]), 0, np.float32(marg[0, 4, 1])]
    assert conf[1].tolist() == [0, np.float32(marg[1, 1, 0]), np.float32(marg[1, 2, 1]), 0, 0]


# ------------------------------------------------------------- the CPU model
def check_mbr_parse(m, raw):
    """The issue's model checks that hold on any device; returns the
    per-sentence (n, mbr heads, projective heads) and the confidences."""
    plain = m.parse(raw)
    proj, proj_conf = m.parse(raw, tree="projective", confidence=True)
    mbr, conf = m.parse(raw, tree="projective-mbr", confidence=True)
    again, plain_conf = m.parse(raw, confidence=True)
    assert again == plain and proj == m.parse(raw, tree="projective") and mbr == m.parse(raw, tree="projective-mbr")
    for d, a, t, c, pt, pc, ac in zip(raw, plain, mbr, conf, proj, proj_conf, plain_conf):
        n = len(d["node_features"])
        assert len(t) == n - 1 == len(c) == len(pc) == len(ac)
        assert [x[1] for x in t] == [x[1] for x in a]
        h = [-1] + [x[0] for x in t]
        assert E.is_tree(h, n, True) and E.is_projective(h, n)
        assert all(0.0 <= x <= 1.0 for x in c + pc + ac)
        assert sum(c) >= sum(pc) - n * 2.0 ** -20                     # MBR: the most expected-correct heads
    with pytest.raises(ValueError):
        m.parse(raw, tree=True, confidence=True)
    with pytest.raises(ValueError):
        m.parse(raw, tree="eisner")
    return mbr, conf


def test_model_mbr_and_confidence_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    check_mbr_parse(m, raw)
    data = m.process_raw_graphs(raw, False)
    o = m.params["output_size"]
    graphs, las, uas = 0, 0.0, 0.0
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p = m.predict_batch(dict(feed), tree="projective-mbr", confidence=True)
        assert set(p) == {"heads", "labels", "n_nodes", "sentences_id", "tree_status", "head_confidence",
                          "log_partition"}
        assert "head_confidence" not in m.predict_batch(dict(feed), tree="projective-mbr")
        probs = m.ops["computed_values"].numpy().reshape(b, v, o)
        marg, logz, scores, status, _ = E.projective_marginals_arrays(probs, p["n_nodes"], True)
        assert (status == 1).all() and (p["tree_status"] != 2).all()
        seen += [int((p["tree_status"] == k).sum()) for k in (0, 1, 2)]
        pred = np.stack([p["heads"], p["labels"]], axis=2)
        assert p["head_confidence"].dtype == np.float32 and p["head_confidence"].shape == (b, v)
        assert np.array_equal(p["head_confidence"], E.arc_confidence_arrays(marg.astype(np.float32), p["n_nodes"], pred))
        assert np.array_equal(p["log_partition"], logz.astype(np.float32))
        for g in range(b):
            n = int(p["n_nodes"][g])
            arg = np.full((1, v, 2), -1, np.int32)
            host, _, st = E.projective_decode_arrays(scores[g][None], [n], arg, True)
            assert st[0] == 1
            assert E.tree_total(scores[g], p["heads"][g], n) == E.tree_total(scores[g], host[0, :, 0], n)
        with pytest.raises(ValueError):
            m.predict_batch(dict(feed), tree=True, confidence=True)
        # evaluate_batch: host scores of the returned heads
        got = m.evaluate_batch(dict(feed), on_device=True, tree="projective-mbr")
        r = m._decode_forward(dict(feed), True, "projective-mbr", True)
        assert np.array_equal(r["pred"][:, :, 0], p["heads"])
        per_graph = [E.graph_scores_from_lists(r["pred"][g], r["gold"][g]) for g in range(b)]
        assert got == tuple(sum(x[c] for x in per_graph) / b for c in range(3))
        graphs += b
        las += got[0] * b
        uas += got[1] * b
    assert seen[1] > 0 and seen[2] == 0, seen
    ref = m.score_epoch(data)
    got = m.score_epoch(data, tree="projective-mbr")
    assert m.decode_stats["repaired_graphs"] == seen[1] and m.decode_stats["infeasible_graphs"] == 0
    assert got[0] == ref[0] and got[3] == ref[3] and got[5] == ref[5]
    assert got[1:3] == (las / graphs, uas / graphs)
    assert m.score_epoch(data)[:4] == ref[:4]


# ------------------------------------------------------------------- the ABI
def test_projective_marginals_rejects_bad_arguments_without_gpu(lib):
    """ggnn_projective_marginals / ggnn_arc_confidence validate on the host
    before any launch."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    y = ctypes.c_void_p(512)
    M = _lib.MARG_LDS_MAXN
    need = 2 * 14 * (M + 1) * (M + 2)
    ok = dict(b=2, v=30, o=150, p=x, n=x, single=1, marg=y, logz=x, scores=None, status=x, ws=None, ws_bytes=0)
    for change, word in ((dict(o=0), b"1..1024"), (dict(o=1025), b"1..1024"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(b=0), b">= 1"), (dict(p=None), b"NULL"),
                         (dict(n=None), b"NULL"), (dict(marg=None), b"NULL"), (dict(logz=None), b"NULL"),
                         (dict(status=None), b"NULL"), (dict(single=2), b"0 or 1"), (dict(marg=x), b"alias"),
                         (dict(v=M + 1), b"workspace"), (dict(v=M + 1, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=M + 1, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_projective_marginals(ctypes.byref(d), a["p"], a["o"], a["n"], a["single"], a["marg"], a["logz"],
                                           a["scores"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
    assert lib.ggnn_projective_marginals(None, x, 150, x, 1, y, x, None, x, None, 0, None) == -1
    d = _lib.dims(2, 30, 64, 1, 1)
    for args, word in (((x, 29, x, x, x), b"v 30 > o 29"), ((None, 150, x, x, x), b"NULL"),
                       ((x, 150, None, x, x), b"NULL"), ((x, 150, x, None, x), b"NULL"),
                       ((x, 150, x, x, None), b"NULL"), ((x, 2000, x, x, x), b"1..1024")):
        assert lib.ggnn_arc_confidence(ctypes.byref(d), *args, None) == -1 and word in lib.ggnn_last_error()
    assert lib.ggnn_projective_marginals_workspace_bytes(2, M + 1) == need
    assert lib.ggnn_projective_marginals_workspace_bytes(256, M) == 0
    assert lib.ggnn_projective_marginals_workspace_bytes(3, 256) == 3 * 14 * 256 * 257
    assert {"ggnn_projective_marginals", "ggnn_projective_marginals_workspace_bytes",
            "ggnn_arc_confidence"} <= set(_lib.EXPORTED)
    # seven fp32 tables and the row maxima fill the 160 KiB of a CU at M, not at M + 1
    assert M == E.MARG_LDS_MAXN and 14 * M * (M + 1) + 1032 <= 160 * 1024 < 14 * (M + 1) * (M + 2) + 1032
    assert M < _lib.TREE_MAXV
