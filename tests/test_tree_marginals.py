"""Arc marginals over all dependency trees on the host:
evaluation.tree_marginals_arrays (the host form of ggnn_tree_marginals, the
matrix-tree theorem with np.linalg) against brute force over all head vectors,
its invariants (row sums, ROOT column, the projective marginals below four
nodes, d logZ / d ln p = marginal), the structurally infeasible graphs, the MBR
tree of its integer scores, the table of the GPU test (the cap on its error bar
and the float32 host form inside it), the model's tree="mbr" /
confidence="nonprojective" keywords on a CPU device, the two backends'
signatures and the C ABI's validation without a GPU.  The case builders, the
table and the bar are shared with tests/test_gpu_tree_marginals.py.

Error bar (an fp32 elimination with partial pivoting at growth factor 1, first
order): a marginal is off by at most bar = n * cond * 2^-24, cond the 1-norm
condition number of the graph's normalised matrix in float64; ln Z by bar / 4 +
|ln Z| * 2^-23 (its own rounding to fp32 on top); a row sum by n * 2^-20 + bar.
The cap is a condition on the table, not a measurement: every status-1 graph of
it has bar <= 2^-6."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

from ggnn_amd import evaluation as E
from ggnn_amd._lib import LAPL_LDS_MAXN as L
from test_projective_marginals import SCALE, check_passthrough, probs_of_scores, random_probs
from test_tree_decode import F, _synthetic_model, _synthetic_raw, closed_group, forbidden_row

CAP = 2.0 ** -6


# ------------------------------------------------------------ case builders
def probs_of_kind(n, o, kind, rng):
    """One graph's float32 [n, o] head probabilities: the four kinds of the
    projective tests and "cyclic": 0.9 on arcs that close the words into
    4-cycles (the last group: what is left of them), 0.05 u elsewhere."""
    if kind != "cyclic":
        return random_probs(n, o, kind, rng)
    p = 0.05 * rng.random((n, o))
    for lo in range(1, n, 4):
        group = list(range(lo, min(lo + 4, n)))
        if len(group) > 1:
            for k, i in enumerate(group):
                p[i, group[(k + 1) % len(group)]] = 0.9
    return p.astype(np.float32)


def weighted_closed_group(n, rng):
    """Words 1..3 may only take each other, with random unequal weights; every
    other word may take anything: no tree, and no pivot need be exactly 0."""
    assert n >= 5
    p = (0.1 + rng.random((n, n))).astype(np.float32)
    p[1:4, :] = 0
    p[1:4, 1:4] = (0.1 + rng.random((3, 3))).astype(np.float32)
    return p


def two_root_children(n):
    """Words 1 and 2 may only take ROOT and every other word only word 1 or 2:
    every tree has two ROOT children."""
    assert n >= 3
    p = np.zeros((n, n), np.float32)
    p[1, 0], p[2, 0] = 0.7, 0.4
    for i in range(3, n):
        p[i, 1 + i % 2] = 0.5
        p[i, 2 - i % 2] = 0.25
    return p


def brute_force(p, n, single_root):
    """(ln Z, marginals [n, n], the trees as (heads, weight)) over all n^(n-1)
    head vectors that are dependency trees, float64; (None, None, []) without
    one."""
    s = E.tree_scores(p[None], [n], n)[0]
    trees = []
    for hv in itertools.product(range(n), repeat=n - 1):
        h = [-1] + list(hv)
        if E.is_tree(h, n, single_root, s):
            trees.append((h, float(np.prod([float(p[i, h[i]]) for i in range(1, n)], dtype=np.float64))))
    if not trees:
        return None, None, []
    z = sum(w for _, w in trees)
    m = np.zeros((n, n))
    for h, w in trees:
        for i in range(1, n):
            m[i, h[i]] += w
    return np.log(z), m / z, trees


def lapl_bar(n, cond):
    """The issue's error bar of a marginal: n * cond * 2^-24."""
    return n * cond * 2.0 ** -24


# ------------------------------------------------- the table of the GPU test
SHAPES = [(4, 4, 150),                       # the smallest bucket
          (3, 8, 8),                         # v = o
          (2, 64, 64),                       # exact wave width
          (2, 65, 150),                      # one past it
          (3, L, max(L, 150)),               # the largest graphs with the matrix in LDS
          (3, L + 1, max(L + 1, 150)),       # both storage tiers in one grid
          (1, 256, 256)]                     # GGNN_TREE_MAXV
KINDS = ("flat", "sparse", "peaked", "tiny", "cyclic")


def node_counts(v):
    """2 (no elimination), 3 (the first pivot choice), an interior value and v;
    around LAPL_LDS_MAXN also L - 1, L and one short graph."""
    out = [v, 5] if v == L + 1 else [v]      # (first: n = L + 1 and n = 5 share a launch)
    out += [2, 3, max(2, min(v - 1, v // 2 + 1))]
    if v in (L, L + 1):
        out += [x for x in (L - 1, L) if x < v]
    return [x for x in dict.fromkeys(out) if x <= v]


def launches(shape):
    """The launches of a shape as lists of b (n, kind): every node count with
    every kind of input; graph 1 of every launch (b = 1: launches of their
    own) has no tree."""
    b, v, o = shape
    counts = node_counts(v)
    if b == 1:                                # (one graph per launch: every kind at v, the other counts flat)
        jobs = [(v, kind) for kind in KINDS] + [(n, "flat") for n in counts[1:]]
    else:
        jobs = [(n, kind) for kind in KINDS for n in counts]
    out = []
    per = max(1, b - 1)
    for k in range(-(-len(jobs) // per)):
        part = jobs[k * per:(k + 1) * per]
        part += jobs[:per - len(part)]
        if b > 1:
            part.insert(1, (counts[k % len(counts)], "infeasible"))
        out.append(part)
    if b == 1:
        out += [[(n, "infeasible")] for n in (v, 2)]
    return out


def _infeasible(n, o, k, rng):
    if n == 2:
        return np.zeros((2, o), np.float32)
    if n < 5:
        return probs_of_scores(closed_group(n), o)
    if k % 3 == 2:
        p = np.zeros((n, o), np.float32)
        p[:, :n] = weighted_closed_group(n, rng)
        return p
    return probs_of_scores((closed_group, forbidden_row)[k % 3](n), o)


_REFERENCE = {}
# the launches whose first seed drew a graph above the cap (small "tiny" graphs: two words that all but choose
# each other, or no word near ROOT under single_root) take a later one
RESEEDED = {((4, 4, 150), 3): 1, ((3, 8, 8), 6): 1, ((3, L + 1, max(L + 1, 150)), 11): 1,
            ((3, L + 1, max(L + 1, 150)), 12): 1}


def reference(shape, k):
    """One launch's input and both host results in float64 (single_root False /
    True), computed once and left unchanged.  Graph 0 carries a NaN in a row <
    n; rows and columns >= n hold positive values that must never be read as
    arcs."""
    key = (shape, k)
    if key not in _REFERENCE:
        b, v, o = shape
        part = launches(shape)[k]
        rng = np.random.default_rng(9000 + 100 * v + k + 100000 * RESEEDED.get(key, 0))
        n = np.asarray([x[0] for x in part], np.int32)
        kinds = [x[1] for x in part]
        p = (0.01 + rng.random((b, v, o))).astype(np.float32)         # (padding: plain positive numbers)
        for g in range(b):
            m = int(n[g])
            p[g, :m, :] = _infeasible(m, o, k, rng) if kinds[g] == "infeasible" else probs_of_kind(m, o, kinds[g], rng)
            p[g, :m, m:] = 0.01 + rng.random((m, o - m))              # columns >= n: positive junk
        m = int(n[0])
        if m >= 3:
            p[0, 2, 1] = np.nan                                       # an arc that is simply not allowed
        else:
            p[0, 0, 1] = np.nan                                       # row 0 < n: never an arc
        host = {sr: E.tree_marginals_arrays(p, n, sr) for sr in (False, True)}
        allowed = E.tree_scores(p, n, v) != F
        for a in (p, n, allowed) + host[False] + host[True]:
            a.setflags(write=False)
        _REFERENCE[key] = (p, n, kinds, allowed, host)
    return _REFERENCE[key]


ALL_LAUNCHES = [(shape, k) for shape in SHAPES for k in range(len(launches(shape)))]
launch_ids = lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


# ------------------------------------------------------------------ the tests
def test_random_cases_equal_brute_force():
    rng = np.random.default_rng(41)
    cases = feasible = infeasible = 0
    for case in range(160):
        n = 2 + case % 5                                              # every n in 2..6
        single_root = bool((case // 5) & 1)
        o = n + (case % 3)
        p = rng.random((n, o)).astype(np.float32)
        p[rng.random((n, o)) < 0.25] = 0
        logz, m, _ = brute_force(p, n, single_root)
        out = E.tree_marginals_arrays(p[None], [n], single_root)
        marg, lz, scores, status, cond = out
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
        assert np.isfinite(cond[0]) and cond[0] >= 1 and (n >= 3 or cond[0] == 1)
    assert cases >= 100 and feasible >= 100 and infeasible >= 5, (cases, feasible, infeasible)


def test_n_below_two_nan_and_padding():
    rng = np.random.default_rng(5)
    p = rng.random((3, 6, 8)).astype(np.float32)
    p[2, 2, 1] = np.nan                                               # an arc that is simply not allowed
    p[2, 4:, :] = np.inf                                              # rows >= n are never read
    out = E.tree_marginals_arrays(p, [1, 0, 4], True)
    marg, logz, scores, status, cond = out
    assert status.tolist() == [0, 0, 1] and logz[0] == 0 and logz[1] == 0 and cond[0] == 1
    check_passthrough(p[0], out, 0)
    check_passthrough(p[1], out, 1)
    assert np.isfinite(marg[2]).all() and marg[2, 2, 1] == 0 and scores[2, 2, 1] == F
    assert (marg[2, 4:] == 0).all() and (marg[2, :, 4:] == 0).all() and (marg[2, 0] == 0).all()
    q = np.where(np.isfinite(p[2, :4, :4]), p[2, :4, :4], 0)
    lz, m, _ = brute_force(q, 4, True)
    assert abs(logz[2] - lz) <= 1e-12 and np.abs(marg[2, :4, :4] - m).max() <= 1e-12
    with pytest.raises(ValueError):
        E.tree_marginals_arrays(p[:, :, :5], [1, 0, 4])               # v > o
    with pytest.raises(ValueError):
        E.tree_marginals_arrays(p, [1, 0])


@pytest.mark.parametrize("single_root", [False, True])
@pytest.mark.parametrize("n", [12, 40])
def test_invariants(n, single_root):
    rng = np.random.default_rng(300 + n)
    for kind in KINDS:
        p = probs_of_kind(n, n + 5, kind, rng)
        marg, logz, scores, status, _ = E.tree_marginals_arrays(p[None], [n], single_root)
        assert status[0] == 1
        assert np.abs(marg[0, 1:n].sum(axis=1) - 1).max() <= 1e-10
        assert (marg[0] >= 0).all() and (marg[0] <= 1).all()
        if single_root:
            assert abs(marg[0, :, 0].sum() - 1) <= 1e-10
        # d ln Z / d ln p(arc) = marg(arc): a central difference, step 1e-6, on float64 potentials through the
        # host form's own pieces (p is float32, so the step cannot be taken on the input)
        w, ok, ln_c = E._normalised_potentials(p, n, np.dtype(np.float64))
        arcs = np.argwhere(ok)
        for i, j in arcs[rng.choice(len(arcs), 5, replace=False)]:
            z = []
            for step in (1e-6, -1e-6):
                q = w.copy()
                q[i, j] *= np.exp(step)
                sign, ln_det = np.linalg.slogdet(E._laplacian(q, n, single_root))
                assert sign > 0
                z.append(ln_det)
            assert abs((z[0] - z[1]) / 2e-6 - marg[0, i, j]) <= 1e-7, (kind, i, j)


@pytest.mark.parametrize("single_root", [False, True])
def test_below_four_nodes_every_tree_is_projective(single_root):
    rng = np.random.default_rng(8)
    for case in range(40):
        n = 2 + case % 2
        p = rng.random((1, n, n + 2)).astype(np.float32)
        p[rng.random(p.shape) < 0.15] = 0
        a = E.tree_marginals_arrays(p, [n], single_root)
        b = E.projective_marginals_arrays(p, [n], single_root)
        assert a[3][0] == b[3][0] and np.array_equal(a[2], b[2])
        if a[3][0] == 1:
            assert np.abs(a[0] - b[0]).max() <= 1e-12 and abs(a[1][0] - b[1][0]) <= 1e-12


@pytest.mark.parametrize("single_root", [False, True])
def test_graphs_without_a_tree_by_structure(single_root):
    rng = np.random.default_rng(12)
    for n in (5, 6, 33):
        cases = [probs_of_scores(case(n), n + 3) for case in (closed_group, forbidden_row)]
        cases.append(np.concatenate([weighted_closed_group(n, rng), np.ones((n, 3), np.float32)], axis=1))
        for p in cases:
            p[0, :] = 0.5                                             # row 0, columns >= n: never arcs
            p[:, n:] = 0.25
            if n <= 6:
                assert brute_force(p, n, single_root)[0] is None
            out = E.tree_marginals_arrays(p[None], [n], single_root)
            assert out[3][0] == 2 and out[1][0] == -np.inf and out[4][0] == np.inf
            check_passthrough(p, out)
            # the same graph inside a feasible launch does not disturb its neighbours
            q = np.stack([random_probs(n, n + 3, "flat", rng), p])
            both = E.tree_marginals_arrays(q, [n, n], single_root)
            assert both[3].tolist() == [1, 2]
            check_passthrough(p, both, 1)


def test_trees_that_need_two_root_children():
    for n in (3, 5, 9):
        p = two_root_children(n)
        multi = E.tree_marginals_arrays(p[None], [n], False)
        single = E.tree_marginals_arrays(p[None], [n], True)
        assert multi[3][0] == 1 and single[3][0] == 2 and single[1][0] == -np.inf
        check_passthrough(p, single)
        assert multi[0][0, 1, 0] == 1 and multi[0][0, 2, 0] == 1
        if n <= 5:
            lz, m, _ = brute_force(p, n, False)
            assert abs(multi[1][0] - lz) <= 1e-12 and np.abs(multi[0][0] - m).max() <= 1e-12


def test_the_mbr_tree_of_the_integer_scores():
    rng = np.random.default_rng(78)
    checked = 0
    for case in range(48):
        n = 4 + case % 4                                              # 4..7
        single_root = bool((case // 4) & 1)
        p = rng.random((n, n)).astype(np.float32)
        p[rng.random((n, n)) < 0.2] = 0
        marg, _, scores, status, _ = E.tree_marginals_arrays(p[None], [n], single_root)
        if status[0] != 1:
            continue
        _, _, trees = brute_force(p, n, single_root)
        best = max(sum(marg[0, i, h[i]] for i in range(1, n)) for h, _ in trees)
        pred = np.full((1, n, 2), -1, np.int32)                       # no tree: the MST pass always runs
        out, _, st = E.tree_decode_arrays(scores, [n], pred, single_root)
        assert st[0] == 1
        h = out[0, :, 0]
        assert E.is_tree(h, n, single_root, scores[0])
        assert sum(marg[0, i, h[i]] for i in range(1, n)) >= best - n * 2.0 ** -20
        checked += 1
    assert checked >= 30


def test_the_launches_cover_the_issue():
    for shape in SHAPES:
        b, v, o = shape
        seen = set()
        for part in launches(shape):
            assert len(part) == b
            seen |= {x for x in part if x[1] != "infeasible"}
            assert (b == 1 and len(part) == 1) or part[1][1] == "infeasible"
        assert any(x[1] == "infeasible" for part in launches(shape) for x in part)
        counts = {x[0] for x in seen}
        assert {2, 3, v} <= counts and (v <= 4 or any(3 < x < v for x in counts))
        assert {(v, kind) for kind in KINDS} <= seen
        if v == L:
            assert {L - 1, L} <= counts
        if v == L + 1:
            assert {L - 1, L, L + 1} <= counts
            assert any({L + 1, 5} <= {x[0] for x in part} for part in launches(shape))


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=launch_ids)
def test_table_keeps_the_cap_and_float32_host_form_the_bar(shape, k):
    """Every status-1 graph of the GPU table has bar <= 2^-6, and the host
    form in float32 stays inside the bars the kernel is held to."""
    b, v, o = shape
    p, n, kinds, allowed, host = reference(shape, k)
    for single_root in (False, True):
        h_marg, h_logz, h_scores, h_status, cond = host[single_root]
        got = E.tree_marginals_arrays(p, n, single_root, np.float32)
        assert got[0].dtype == np.float32 and np.array_equal(got[3], h_status)
        for g, what in enumerate(kinds):
            m = int(n[g])
            if what == "infeasible":
                assert h_status[g] == 2
            elif what != "sparse" or m > 8:                           # (a small sparse graph may have no tree)
                assert h_status[g] == 1, (what, m)
            if h_status[g] != 1:
                continue
            bar = lapl_bar(m, cond[g])
            err = np.abs(got[0][g].astype(np.float64) - h_marg[g]).max()
            err_z = abs(float(got[1][g]) - h_logz[g])
            print("n %d %s single_root %d: cond %.3g bar %.3g, float32 host form: marg err %.3g (ratio %.3g), "
                  "logz err %.3g" % (m, what, single_root, cond[g], bar, err, err / bar, err_z))
            assert bar <= CAP, (what, m, cond[g], bar)
            assert err <= bar, (what, m, err, bar)
            assert err_z <= bar / 4 + abs(h_logz[g]) * 2.0 ** -23, (what, m, err_z)


# ------------------------------------------------------------- the CPU model
def check_tree_mbr_parse(m, raw):
    """The issue's model checks that hold on any device; returns the MBR trees
    and their confidences.  (The arg-max joins the comparison of the summed
    confidences where it is a tree: heads that form a cycle are outside the
    set the MBR tree is the best of, and may collect more.)"""
    plain = m.parse(raw)
    mst, mst_conf = m.parse(raw, tree=True, confidence="nonprojective")
    mbr, conf = m.parse(raw, tree="mbr", confidence="nonprojective")
    again, plain_conf = m.parse(raw, confidence="nonprojective")
    proj, proj_conf = m.parse(raw, tree="projective", confidence="nonprojective")
    assert again == plain and mst == m.parse(raw, tree=True) and mbr == m.parse(raw, tree="mbr")
    assert proj == m.parse(raw, tree="projective")
    for d, a, t, c, s, sc, ac, pc in zip(raw, plain, mbr, conf, mst, mst_conf, plain_conf, proj_conf):
        n = len(d["node_features"])
        assert len(t) == n - 1 == len(c) == len(sc) == len(ac) == len(pc) == len(s)
        assert [x[1] for x in t] == [x[1] for x in a]
        assert E.is_tree([-1] + [x[0] for x in t], n, True)
        assert E.is_tree([-1] + [x[0] for x in s], n, True)
        assert all(0.0 <= x <= 1.0 for x in c + sc + ac + pc)
        assert sum(c) >= sum(sc) - n * 2.0 ** -20                     # MBR: the most expected-correct heads
        if E.is_tree([-1] + [x[0] for x in a], n, True):
            assert sum(c) >= sum(ac) - n * 2.0 ** -20
    for kw in (dict(tree="mbr", confidence=True), dict(tree="mbr", confidence="projective"),
               dict(tree=True, confidence=True), dict(tree=True, confidence="projective"),
               dict(confidence="matrix-tree"), dict(tree="mst"), dict(tree="MBR")):
        with pytest.raises(ValueError):
            m.parse(raw, **kw)
    with pytest.raises(ValueError, match="nonprojective"):
        m.parse(raw, tree="mbr", confidence=True)
    return mbr, conf


def test_model_mbr_and_confidence_on_a_cpu_device():
    m = _synthetic_model()
    raw = _synthetic_raw()
    check_tree_mbr_parse(m, raw)
    data = m.process_raw_graphs(raw, False)
    o = m.params["output_size"]
    graphs, las, uas = 0, 0.0, 0.0
    seen = np.zeros(3, int)
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p = m.predict_batch(dict(feed), tree="mbr", confidence="nonprojective")
        assert set(p) == {"heads", "labels", "n_nodes", "sentences_id", "tree_status", "head_confidence",
                          "log_partition"}
        assert "head_confidence" not in m.predict_batch(dict(feed), tree="mbr")
        probs = m.ops["computed_values"].numpy().reshape(b, v, o)
        marg, logz, scores, status, _ = E.tree_marginals_arrays(probs, p["n_nodes"], True)
        assert (status == 1).all() and (p["tree_status"] != 2).all()
        seen += [int((p["tree_status"] == k).sum()) for k in (0, 1, 2)]
        pred = np.stack([p["heads"], p["labels"]], axis=2)
        assert p["head_confidence"].dtype == np.float32 and p["head_confidence"].shape == (b, v)
        assert np.array_equal(p["head_confidence"], E.arc_confidence_arrays(marg.astype(np.float32), p["n_nodes"], pred))
        assert np.array_equal(p["log_partition"], logz.astype(np.float32))
        q = m.predict_batch(dict(feed), tree=True, confidence="nonprojective")
        assert np.array_equal(q["heads"], m.predict_batch(dict(feed), tree=True)["heads"])
        assert np.array_equal(q["log_partition"], p["log_partition"])
        for g in range(b):
            n = int(p["n_nodes"][g])
            arg = np.full((1, v, 2), -1, np.int32)
            host, _, st = E.tree_decode_arrays(scores[g][None], [n], arg, True)
            assert st[0] == 1
            assert E.tree_total(scores[g], p["heads"][g], n) == E.tree_total(scores[g], host[0, :, 0], n)
        with pytest.raises(ValueError):
            m.predict_batch(dict(feed), tree="mbr", confidence=True)
        # evaluate_batch: host scores of the returned heads
        got = m.evaluate_batch(dict(feed), on_device=True, tree="mbr")
        r = m._decode_forward(dict(feed), True, "mbr", True)
        assert np.array_equal(r["pred"][:, :, 0], p["heads"])
        per_graph = [E.graph_scores_from_lists(r["pred"][g], r["gold"][g]) for g in range(b)]
        assert got == tuple(sum(x[c] for x in per_graph) / b for c in range(3))
        graphs += b
        las += got[0] * b
        uas += got[1] * b
    assert seen[1] > 0 and seen[2] == 0, seen
    ref = m.score_epoch(data)
    got = m.score_epoch(data, tree="mbr")
    assert m.decode_stats["repaired_graphs"] == seen[1] and m.decode_stats["infeasible_graphs"] == 0
    assert got[0] == ref[0] and got[3] == ref[3] and got[5] == ref[5]
    assert got[1:3] == (las / graphs, uas / graphs)
    assert m.score_epoch(data)[:4] == ref[:4]


def test_host_decoder_and_output_heads_take_the_same_arguments():
    """decode_chain calls its two backends alike: tree_marginals of the host
    adapter and of the device binding agree on the names, order, kinds and
    defaults of the parameters the chain passes (the check of test_decode.py,
    with projective_marginals beside it: the two are interchangeable)."""
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    params = ("probs_head", "n_nodes", "single_root", "with_scores")
    for name in ("tree_marginals", "projective_marginals"):
        dev = inspect.signature(getattr(OutputHeads, name)).parameters
        host = inspect.signature(getattr(HostDecoder, name)).parameters
        want = ["self"] + list(params)
        assert list(dev)[:len(want)] == want and list(host)[:len(want)] == want, name
        for p in params:
            assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), (name, p)
        for sig in (dev, host):                                           # (a workspace): never required
            assert all(sig[p].default is not inspect.Parameter.empty for p in list(sig)[len(want):]), name
    assert (list(inspect.signature(OutputHeads.tree_marginals).parameters)
            == list(inspect.signature(OutputHeads.projective_marginals).parameters))
    rng = np.random.default_rng(2)
    p = rng.random((2, 5, 7)).astype(np.float32)
    out = HostDecoder().tree_marginals(p, [5, 4])
    assert out[0].dtype == np.float32 and out[1].dtype == np.float32 and len(out) == 4
    assert HostDecoder().tree_marginals(p, [5, 4], with_scores=False)[2] is None


# ------------------------------------------------------------------- the ABI
def test_tree_marginals_rejects_bad_arguments_without_gpu(lib):
    """ggnn_tree_marginals validates on the host before any launch."""
    from ggnn_amd import _lib
    x = ctypes.c_void_p(256)                          # never dereferenced: every call below fails validation
    y = ctypes.c_void_p(512)
    need = 2 * 4 * L * (L | 1)                        # b = 2, v = L + 1: (v - 1) rows of (v - 1) | 1 floats
    ok = dict(b=2, v=30, o=150, p=x, n=x, single=1, marg=y, logz=x, scores=None, status=x, ws=None, ws_bytes=0)
    for change, word in ((dict(o=0), b"1..1024"), (dict(o=1025), b"1..1024"), (dict(o=29), b"v 30 > o 29"),
                         (dict(v=257, o=300), b"GGNN_TREE_MAXV"), (dict(b=0), b">= 1"), (dict(p=None), b"NULL"),
                         (dict(n=None), b"NULL"), (dict(marg=None), b"NULL"), (dict(logz=None), b"NULL"),
                         (dict(status=None), b"NULL"), (dict(single=2), b"0 or 1"), (dict(marg=x), b"alias"),
                         (dict(v=L + 1, o=256), b"workspace"),
                         (dict(v=L + 1, o=256, ws=x, ws_bytes=need - 1), b"workspace"),
                         (dict(v=L + 1, o=256, ws=None, ws_bytes=need), b"workspace")):
        a = dict(ok, **change)
        d = _lib.dims(a["b"], a["v"], 64, 1, 1)
        rc = lib.ggnn_tree_marginals(ctypes.byref(d), a["p"], a["o"], a["n"], a["single"], a["marg"], a["logz"],
                                     a["scores"], a["status"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
        assert b"tree_marginals" in lib.ggnn_last_error()
    assert lib.ggnn_tree_marginals(None, x, 150, x, 1, y, x, None, x, None, 0, None) == -1
    assert lib.ggnn_tree_marginals_workspace_bytes(2, L + 1) == need
    assert lib.ggnn_tree_marginals_workspace_bytes(256, L) == 0
    assert lib.ggnn_tree_marginals_workspace_bytes(0, 256) == 0
    assert lib.ggnn_tree_marginals_workspace_bytes(3, 256) == 3 * 4 * 255 * 255
    assert {"ggnn_tree_marginals", "ggnn_tree_marginals_workspace_bytes"} <= set(_lib.EXPORTED)
    # the matrix ((n - 1) rows of (n - 1) | 1 floats) and what the kernel keeps beside it (5,656 B: three float
    # and one row-sum array, three int16 arrays of 256, 24 B of scalars) fit the 160 KiB of a CU at L, not at L + 1
    assert L == E.LAPL_LDS_MAXN and 4 * (L - 1) * ((L - 1) | 1) + 5656 <= 160 * 1024 < 4 * L * (L | 1) + 5656
    assert L < _lib.TREE_MAXV
