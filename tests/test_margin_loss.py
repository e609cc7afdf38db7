"""The max-margin training loss on the host (evaluation.margin_loss_arrays):
against brute force over every tree of small graphs (the loss and, by central
differences, its gradient with respect to the head logits), the three kinds of
graph (not used, inactive, active), cost 0 against the plain decoders, the
model's parameters, and the two conditions that the GPU tests' inputs meet."""
import numpy as np
import pytest

import margin_loss_cases as MC
import tree_loss_cases as TL
from ggnn_amd import evaluation as E
from test_tree_loss import FAMILIES, all_trees

LN2 = float(np.log(2.0))


def resolution(n, v):
    """The most the host form's l can fall short of the true maximum: every
    score and C are rounded to half a unit of 2^-k bits, two trees are compared."""
    return 1.5 * (n - 1) * LN2 * 2.0 ** -E.tree_score_shift(v)


def brute_margin(z, trees, gold, n, cost):
    """(l, the maximising trees' rows, the gap to the best other value) of one
    graph in float64 on the logits z [v, o]: l = max over ``trees`` of sum_d
    z[d][T_d] - z[d][y_d] + cost [T_d != y_d] (the rows' logsumexp cancels)."""
    w = np.arange(1, n)
    y = np.asarray(gold)[1:]
    tot = (z[w[None, :], trees[:, 1:]] - z[w, y][None, :] + cost * (trees[:, 1:] != y[None, :])).sum(axis=1)
    best = tot.max()
    rest = tot[tot < best]
    return float(best), np.flatnonzero(tot == best), float(best - rest.max()) if rest.size else np.inf


# ------------------------------------------------------------------ brute force
@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_loss_equals_brute_force_within_the_scores_resolution(n, family, single_root):
    v, o = n + 1, n + 2
    trees = all_trees(n, family, single_root)
    gold = [0] + list(range(0, n - 1))
    y = TL.heads_to_gold(gold, v, o)[None]
    for seed in TL.SEEDS:
        p32, _ = TL.softmax_probs(1, v, o, 100 * n + seed)
        lp = np.log(p32[0].astype(np.float64))
        for cost in (1.0, 2.5):
            ref, _, _ = brute_margin(lp, trees, gold, n, cost)
            term, marg, heads, value, hamming, status, used = E.margin_loss_arrays(p32, y, [n], family, single_root,
                                                                                   1.0, cost)
            assert status.tolist() == [1] and used.tolist() == [1] and ref >= 0
            assert E.is_tree(heads[0], n, single_root) and (family == "nonprojective" or E.is_projective(heads[0], n))
            assert heads[0, 0] == -1 and (heads[0, n:] == -1).all()
            raw = MC.raw_loss(p32[0], gold, heads[0], n, cost)
            # T* is a tree of the family, so l <= the maximum, and it is short of it by the resolution at most
            assert ref - resolution(n, v) <= raw <= ref + 1e-12, (raw, ref)
            assert value[0] == np.float32(max(0.0, raw)) and hamming[0] == (heads[0, 1:n] != gold[1:]).sum()
            ce = -lp[np.arange(1, n), gold[1:]].sum()
            assert abs(term - (max(0.0, raw) - ce)) <= 1e-12 * max(1.0, abs(ce))


@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [3, 4, 5])
def test_gradient_equals_central_differences_at_a_unique_maximiser(n, family, single_root):
    """The loss is piecewise linear in the logits: where one tree leads every
    other by more than the step and the scores' resolution, marg - y is the
    gradient and central differences give it to rounding."""
    v, o, cost, step = n + 1, n + 2, 1.0, 1e-4
    trees = all_trees(n, family, single_root)
    gold = [0] + list(range(0, n - 1))
    y = TL.heads_to_gold(gold, v, o)[None]
    checked = 0
    for seed in TL.SEEDS:
        p32, z = TL.softmax_probs(1, v, o, 100 * n + seed)
        ref, arg, gap = brute_margin(z[0], trees, gold, n, cost)
        if not (len(arg) == 1 and gap > 1e-2 and ref > 1e-2):
            continue
        checked += 1
        _, marg, heads, _, _, _, used = E.margin_loss_arrays(p32, y, [n], family, single_root, 1.0, cost)
        assert used.tolist() == [1] and heads[0, 1:n].tolist() == trees[arg[0], 1:].tolist()
        grad = marg[0].astype(np.float64) - y[0]
        loss = lambda zz: max(0.0, brute_margin(zz, trees, gold, n, cost)[0])
        worst = 0.0
        for d in range(v):
            for k in range(o):
                zp, zm = z[0].copy(), z[0].copy()
                zp[d, k] += step
                zm[d, k] -= step
                worst = max(worst, abs((loss(zp) - loss(zm)) / (2 * step) - grad[d, k]))
        assert worst <= 1e-9, (n, family, single_root, seed, worst)
    assert checked >= 2, checked


def test_the_cost_augmented_tree_never_scores_below_the_gold():
    """l >= 0 in integers: total'(T*) >= total'(y) on every used graph of every batch."""
    seen = 0
    for family, shape in MC.ABI_CASES:
        for seed in MC.SEEDS:
            for cost in MC.COSTS:
                p, y, n, _ = MC.batch(family, shape, seed, cost)
                gold = MC.gold_heads(y)
                s2 = E.margin_scores(E.tree_scores(p, n, shape[1]), gold, cost, shape[1])
                for single_root in (True, False):
                    r = MC.reference(family, shape, seed, single_root, cost)
                    for g in np.flatnonzero(r["used"]):
                        m = int(n[g])
                        assert E.tree_total(s2[g], r["heads"][g], m) >= E.tree_total(s2[g], gold[g], m)
                        seen += 1
    assert seen > 500


# ------------------------------------------------------------------ the three kinds of graph
@pytest.mark.parametrize("family", [0, 1])
def test_not_used_inactive_and_active_graphs(family):
    shape, b = (6, 9, 12), 6
    p, y, n, kinds = MC.batch(family, shape, 0, 1.0)
    r = MC.reference(family, shape, 0, True, 1.0)
    assert r["used"].tolist() == MC.expected_used(family, b)
    gold = MC.gold_heads(y)
    total = 0.0
    for g, kind in enumerate(kinds):
        m = int(n[g])
        if not r["used"][g]:                       # the local loss: the probabilities stay in place
            assert r["marg"][g].tobytes() == p[g].tobytes() and (r["heads"][g] == -1).all(), kind
            assert r["value"][g] == 0 and r["hamming"][g] == 0 and r["status"][g] == 0, kind
            continue
        assert r["status"][g] == 1 and (r["heads"][g, 1:m] >= 0).all()
        assert r["heads"][g, 0] == -1 and (r["heads"][g, m:] == -1).all()
        lp_gold = float(np.log(p[g, np.arange(1, m), gold[g, 1:m]].astype(np.float64)).sum())
        if kind == "confident":                    # inactive: T* = y, no gradient
            assert r["heads"][g, 1:m].tolist() == gold[g, 1:m].tolist() and r["raw"][g] == 0 and r["value"][g] == 0
            assert r["marg"][g].tobytes() == y[g].tobytes() and r["hamming"][g] == 0
            total += lp_gold
            continue
        assert r["raw"][g] > 1e-9 and r["hamming"][g] >= 1, (kind, r["raw"][g])      # active
        onehot = np.zeros_like(p[g])
        onehot[np.arange(1, m), r["heads"][g, 1:m]] = 1
        assert r["marg"][g].tobytes() == onehot.tobytes()
        assert r["value"][g] == np.float32(r["raw"][g])
        total += r["raw"][g] + lp_gold
    assert abs(r["term"] - total / r["tn"]) <= 1e-12 * abs(r["term"])
    # the near ties: at cost 1 the rivals (half a nat behind) win, every word where any tree is allowed; at cost 0
    # the gold arcs (0.1 nats ahead) do
    g = kinds.index("near ties")
    assert r["hamming"][g] == int(n[g]) - 1 if family == 0 else r["hamming"][g] >= 1
    r0 = MC.reference(family, shape, 0, True, 0.0)
    assert r0["used"][g] == 1 and r0["hamming"][g] == 0 and r0["raw"][g] == 0
    assert r0["marg"][g].tobytes() == MC.batch(family, shape, 0, 0.0)[1][g].tobytes()


@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family", [0, 1])
def test_cost_zero_is_the_plain_decode(family, single_root):
    shape = (4, 65, 70)
    decode = E.projective_decode_arrays if family == 1 else E.tree_decode_arrays
    for seed in MC.SEEDS:
        p, y, n, _ = MC.batch(family, shape, seed, 0.0)
        r = MC.reference(family, shape, seed, single_root, 0.0)
        scores = E.tree_scores(p, n, shape[1])
        assert np.array_equal(E.margin_scores(scores, MC.gold_heads(y), 0.0, shape[1]), scores)
        pred, _, status = decode(scores, n, np.full((len(n), shape[1], 2), -1, np.int32), single_root)
        for g in np.flatnonzero(r["used"]):
            assert status[g] == 1 and pred[g, 1:n[g], 0].tolist() == r["heads"][g, 1:n[g]].tolist()
            assert r["raw"][g] >= -resolution(int(n[g]), shape[1])


# ------------------------------------------------------------------ arguments and parameters
def test_host_form_validates_its_arguments():
    p, y, n, _ = MC.batch(0, (6, 9, 12), 0, 1.0)
    for bad in (-0.5, 64.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError):
            E.margin_loss_arrays(p, y, n, 0, True, 3.0, bad)
    for bad in ("nonprojective-margin", "projective-margin", "eisner", 2, None, True):
        with pytest.raises(ValueError):
            E.margin_loss_arrays(p, y, n, bad, True, 3.0, 1.0)
    a = E.margin_loss_arrays(p, y, n, 0, True, 3.0, 64.0)
    b = E.margin_loss_arrays(p, y, n, "nonprojective", True, 3.0, 64.0)
    assert a[0] == b[0] and all(np.array_equal(u, w) for u, w in zip(a[1:], b[1:]))
    assert E.margin_cost_units(1.0, 9) == int(np.rint(2 ** 16 / LN2)) and E.margin_cost_units(0.0, 200) == 0
    # |s'| <= 150 * 2^k at the largest cost
    assert E.margin_cost_units(64.0, 200) <= 150 * 2 ** E.tree_score_shift(200)


def test_the_likelihood_families_are_as_before():
    assert E.TREE_LOSS_FAMILIES == {"nonprojective": 0, "projective": 1}
    for name in E.MARGIN_LOSS_KINDS:
        with pytest.raises(ValueError):
            E._tree_loss_family(name)
    assert E.MARGIN_LOSS_KINDS == {"nonprojective-margin": 0, "projective-margin": 1}


def test_params_are_validated_at_construction():
    kinds = (None, "nonprojective", "projective", "nonprojective-margin", "projective-margin")
    for kind in kinds:                                     # the margin is checked whatever the loss
        for bad in (-1.0, 64.5, float("nan"), "1", None, True):
            with pytest.raises(ValueError):
                TL.dev_model(device="cpu", structured_loss=kind, structured_loss_margin=bad)
    for bad in ("eisner", "margin", "projective_margin", True, 0):
        with pytest.raises(ValueError):
            TL.dev_model(device="cpu", structured_loss=bad)
    m, _ = TL.dev_model(device="cpu")
    assert m.params["structured_loss"] is None and m.params["structured_loss_margin"] == 1.0
    assert m._structured() is None and m._tree_loss_arg("n") is None
    # today's kinds: today's 2-tuple, whatever the margin says
    m, _ = TL.dev_model(device="cpu", structured_loss="projective", structured_loss_margin=2.5)
    assert m._structured() == (1, True) and m._tree_loss_arg("n") == (1, True, "n")
    m, _ = TL.dev_model(device="cpu", structured_loss="projective-margin", structured_loss_single_root=False)
    assert m._structured() == (1, False, 1.0) and m._tree_loss_arg("n") == (1, False, "n", 1.0)
    m, _ = TL.dev_model(device="cpu", structured_loss="nonprojective-margin", structured_loss_margin=2.5)
    assert m._structured() == (0, True, 2.5) and m._tree_loss_arg(None) is None
    assert dict(m.params)["structured_loss_margin"] == 2.5          # what the checkpoint pickles
    # the node counts of a feed: as for the likelihood kinds
    feed = TL.dev_feeds(m, _, count=6)[0]
    n = m._loss_n_nodes(feed)
    assert n is not None and n.dtype == np.int32 and (n >= 2).all()
    assert m._loss_n_nodes(dict(feed, node_mask=np.asarray(feed["node_mask"]) * 0.5)).tolist() == [0] * len(n)


# ------------------------------------------------------------------ the GPU tests' inputs
def test_gpu_inputs_are_away_from_rounding_boundaries():
    """Every allowed arc's log2 p * 2^k lies at least 2^-20 from a rounding
    boundary: a last-bit difference between two double log2 cannot move an
    integer score (|log2 p * 2^k| < 2^24, so one ulp of it is below 2^-28)."""
    seen = 0
    for family, shape in MC.ABI_CASES:
        v = shape[1]
        scale = float(2 ** E.tree_score_shift(v))
        for seed in MC.SEEDS:
            for cost in MC.COSTS:
                p, _, n, _ = MC.batch(family, shape, seed, cost)
                ok = E.tree_scores(p, n, v) != E.TREE_FORBIDDEN
                x = np.log2(p[ok].astype(np.float64)) * scale
                assert np.abs(x).max() < 2.0 ** 24
                off = np.abs(x - np.floor(x) - 0.5).min()
                assert off >= 2.0 ** -20, (family, shape, seed, cost, off)
                seen += int(ok.sum())
    assert seen > 10 ** 6


def test_gpu_inputs_have_no_loss_near_zero():
    """Every used graph has l = 0 exactly or |l| > 1e-9: whether it is active
    does not hang on the last bits of a double log.  On abi_batch's graphs at
    cost 1 and seed 0 every eligible graph is active with l >= 2.2."""
    for family, shape in MC.ABI_CASES:
        b = shape[0]
        for seed in MC.SEEDS:
            for cost in MC.COSTS:
                for single_root in (True, False):
                    r = MC.reference(family, shape, seed, single_root, cost)
                    assert r["used"].tolist() == MC.expected_used(family, b), (family, shape, seed, cost, single_root)
                    raw = r["raw"][r["used"] == 1]
                    assert ((raw == 0) | (np.abs(raw) > 1e-9)).all(), (family, shape, seed, cost, raw)
                    assert np.array_equal(r["value"], np.maximum(r["raw"], 0).astype(np.float32))
                    if cost == 1.0 and seed == 0:
                        assert (r["raw"][:b] >= 2.2).all(), r["raw"][:b]
