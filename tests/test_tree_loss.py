"""The tree-structured training loss on the host (evaluation.gold_tree_ok,
tree_loss_arrays): against brute force over every tree of small graphs (the
loss and, by central differences, its gradient with respect to the head
logits), one graph of every kind that is not eligible, the captured step's
input layout, and the eligibility of the real dev sentences' gold trees."""
import itertools

import numpy as np
import pytest

import tree_loss_cases as TL
from ggnn_amd import evaluation as E
from ggnn_amd.graphs import StepLayout

FAMILIES = ("nonprojective", "projective")


# ------------------------------------------------------------------ brute force
def all_trees(n, family, single_root):
    """Every head vector over nodes 0..n-1 (heads[0] = 0) that is a tree of the family."""
    out = []
    for hs in itertools.product(range(n), repeat=n - 1):
        heads = (0,) + hs
        if E.is_tree(heads, n, single_root) and (family == "nonprojective" or E.is_projective(heads, n)):
            out.append(heads)
    return np.asarray(out, np.int64)


def brute_loss(z, trees, gold, n, p=None):
    """-ln(weight(gold) / Z) of one graph in float64: the potentials are the
    softmax of the logits z [v, o] over all o columns (or ``p`` as given), the
    weight of a tree the product of its words' potentials, Z the sum over
    ``trees``."""
    if p is None:
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    lp = np.log(p)
    w = np.arange(1, n)
    tot = lp[w[None, :], trees[:, 1:]].sum(axis=1)
    mx = tot.max()
    ln_z = mx + np.log(np.exp(tot - mx).sum())
    return -lp[w, np.asarray(gold)[1:]].sum() + ln_z


@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_loss_and_gradient_equal_brute_force(n, family, single_root):
    v, o = n + 1, n + 2                                   # a padding row and two padding columns
    trees = all_trees(n, family, single_root)
    gold = [0] + list(range(0, n - 1))                    # the chain i -> i - 1
    assert any(tuple(t) == tuple(gold) for t in trees)
    y = TL.heads_to_gold(gold, v, o)[None]
    for seed in TL.SEEDS:
        p32, z = TL.softmax_probs(1, v, o, 100 * n + seed)
        term, marg, logz, status, used = E.tree_loss_arrays(p32, y, [n], family, single_root, 1.0)
        assert status[0] == 1 and used[0] == 1
        # the loss: on the potentials the host form reads (rounded to float32)
        p64 = p32[0].astype(np.float64)
        ce = -np.log(p64[np.arange(1, n), gold[1:]]).sum()
        ref = brute_loss(None, trees, gold, n, p=p64)
        assert abs(ce + term - ref) <= 1e-12 * abs(ref), (ce + term, ref)
        assert abs(term - float(logz[0])) <= 1e-15 * abs(term)
        # the gradient with respect to the logits: central differences, step 1e-4.  1e-6: the host forms round
        # their input to float32 (2^-24 per potential, at most 5 potentials per tree) and the difference quotient
        # itself is good to about 1e-8
        grad = marg[0].astype(np.float64) - y[0]
        worst = 0.0
        for d in range(v):
            for k in range(o):
                zp, zm = z[0].copy(), z[0].copy()
                zp[d, k] += 1e-4
                zm[d, k] -= 1e-4
                fd = (brute_loss(zp, trees, gold, n) - brute_loss(zm, trees, gold, n)) / 2e-4
                worst = max(worst, abs(fd - grad[d, k]))
        assert worst <= 1e-6, (n, family, single_root, seed, worst)
        # every word's marginals sum to 1: the two -p[d][k] terms of the gradient cancel
        assert np.abs(marg[0, 1:n].sum(axis=1) - 1).max() <= 1e-12


# ------------------------------------------------------------------ graphs that are not eligible
def _case(kind):
    """(p [1, v, o], y [1, v, o], n, family, single_root) of one graph that is not eligible."""
    v, o, n = 7, 9, 6
    p, _ = TL.softmax_probs(1, v, o, 5)
    heads = [0] + list(range(0, n - 1))                   # the chain: eligible as it stands
    family, single_root = "nonprojective", True
    y = None
    if kind == "gold cycle":
        heads[2], heads[3] = 3, 2
    elif kind == "two ROOT children":
        heads[4] = 0
    elif kind == "word without gold":
        y = TL.heads_to_gold(heads, v, o)
        y[3] = 0
    elif kind == "two golds in a row":
        y = TL.heads_to_gold(heads, v, o)
        y[3, 0] = 1
    elif kind == "gold column >= n":
        heads[5] = n
    elif kind == "gold on the word itself":
        heads[4] = 4
    elif kind == "gold arc of potential 0":
        p[0, 3, 2] = 0
    elif kind == "crossing gold":
        heads = [0, 0, 4, 1, 1, 4]                        # (2, 4) crosses (3, 1); a tree with one ROOT child
        family = "projective"
    elif kind == "n < 2":
        n, heads = 1, [0]
    elif kind == "no tree":
        p[0, 2, :] = 0                                    # word 2 has no allowed arc at all
    else:
        raise KeyError(kind)
    if y is None:
        y = TL.heads_to_gold(heads, v, o)
    return p, y[None], n, family, single_root


KINDS = ("gold cycle", "two ROOT children", "word without gold", "two golds in a row", "gold column >= n",
         "gold on the word itself", "gold arc of potential 0", "crossing gold", "n < 2", "no tree")


def test_the_plain_chain_is_eligible():
    """The base of every case below, before its defect is put in."""
    v, o, n = 7, 9, 6
    p, _ = TL.softmax_probs(1, v, o, 5)
    y = TL.chain_gold(n, v, o)[None]
    for family in FAMILIES:
        for single_root in (True, False):
            assert E.gold_tree_ok(y, p, [n], family, single_root).all()
            assert E.tree_loss_arrays(p, y, [n], family, single_root, 3.0)[4].tolist() == [1]


@pytest.mark.parametrize("kind", KINDS)
def test_a_graph_that_is_not_eligible_keeps_the_local_loss(kind):
    p, y, n, family, single_root = _case(kind)
    assert not E.gold_tree_ok(y, p, [n], family, single_root).any()
    term, marg, logz, status, used = E.tree_loss_arrays(p, y, [n], family, single_root, 3.0)
    assert used.tolist() == [0] and status[0] != 1
    assert marg.astype(np.float32).tobytes() == p.tobytes()
    assert term == 0.0
    if kind == "two ROOT children":                       # a tree all the same, once ROOT may have several children
        assert E.tree_loss_arrays(p, y, [n], family, False, 3.0)[4].tolist() == [1]
    if kind == "crossing gold":                           # and a crossing tree is a dependency tree
        term, marg, _, _, used = E.tree_loss_arrays(p, y, [n], "nonprojective", single_root, 3.0)
        assert used.tolist() == [1] and term < 0 and marg.astype(np.float32).tobytes() != p.tobytes()


def test_a_batch_mixes_used_and_unused_graphs():
    p, y, n, kinds = TL.abi_batch(0, (6, 9, 12), 0)
    for single_root in (True, False):
        r = TL.abi_reference(0, (6, 9, 12), 0, single_root)
        assert r["used"].tolist() == [1] * 6 + [0] * 3 and r["status"].tolist() == [1] * 6 + [0] * 3
        assert r["term"] == float(r["logz"][:6].sum()) / r["tn"] and r["term"] < 0
        assert r["marg"][6:].astype(np.float32).tobytes() == p[6:].tobytes()
        assert (r["bar"][:6] > 0).all() and (r["bar"] <= 2.0 ** -6).all()


def test_family_and_shapes_are_validated():
    p, _ = TL.softmax_probs(1, 4, 6, 0)
    y = TL.chain_gold(4, 4, 6)[None]
    for bad in (2, "eisner", None, True):
        with pytest.raises(ValueError):
            E.gold_tree_ok(y, p, [4], bad)
    with pytest.raises(ValueError):
        E.gold_tree_ok(y[:, :3], p, [4], 0)
    assert E.gold_tree_ok(y, p, [4], 0).tolist() == E.gold_tree_ok(y, p, [4], "nonprojective").tolist() == [True]


# ------------------------------------------------------------------ the captured step's inputs
def test_step_layout_places_the_node_counts_after_the_labels():
    b, v, ncols, o, oe = 3, 7, 6, 9, 4
    L = StepLayout(b, v, ncols, o, oe)
    assert L.SCALARS <= L.wi < L.edges < L.offs < L.yh < L.ye < L.n_nodes < L.nbytes
    assert L.n_nodes % 64 == 0 and L.n_nodes >= L.ye + b * v * oe * 4 and L.nbytes >= L.n_nodes + b * 4
    rng = np.random.default_rng(0)
    wi = rng.integers(0, 50, (b, v, ncols)).astype(np.int32)
    edges = rng.integers(0, 5, (11, 3)).astype(np.int32)
    offs = np.array([0, 4, 9, 11], np.int32)
    yh, ye = rng.random((b, v, o)).astype(np.float32), rng.random((b, v, oe)).astype(np.float32)
    n = np.array([7, 2, 5], np.int32)
    host = np.full(L.nbytes, 0xAB, np.uint8)
    L.fill(host, [1, 2, 3], 9, 17.5, wi, edges, offs, yh, ye, n_nodes=n)
    assert np.array_equal(host[L.n_nodes:L.n_nodes + b * 4].view(np.int32), n)
    # the nine-argument call fills everything else the same and leaves the counts at zero
    old = np.full(L.nbytes, 0xAB, np.uint8)
    L.fill(old, [1, 2, 3], 9, 17.5, wi, edges, offs, yh, ye)
    assert (old[L.n_nodes:L.n_nodes + b * 4] == 0).all()
    assert old[:L.n_nodes].tobytes() == host[:L.n_nodes].tobytes()
    assert np.array_equal(old[L.yh:L.yh + yh.nbytes].view(np.float32), yh.reshape(-1))
    assert np.array_equal(old[L.ye:L.ye + ye.nbytes].view(np.float32), ye.reshape(-1))
    assert np.array_equal(old[L.wi:L.wi + wi.nbytes].view(np.int32), wi.reshape(-1))
    assert old[32:36].view(np.float32)[0] == np.float32(17.5) and old[24:32].view(np.int64)[0] == 9


# ------------------------------------------------------------------ the model's parameters and the real data
def test_params_are_validated_at_construction():
    for bad in (dict(structured_loss="eisner"), dict(structured_loss=True), dict(structured_loss=0),
                dict(structured_loss="projective", structured_loss_single_root="yes"),
                dict(structured_loss_single_root=None)):
        with pytest.raises(ValueError):
            TL.dev_model(device="cpu", **bad)
    m, _ = TL.dev_model(device="cpu")
    assert m.params["structured_loss"] is None and m.params["structured_loss_single_root"] is True
    assert m._structured() is None and m._loss_n_nodes({"num_graphs": 2}) is None
    m, _ = TL.dev_model(device="cpu", structured_loss="projective", structured_loss_single_root=False)
    assert m._structured() == (1, False)


def test_every_real_dev_gold_tree_is_eligible():
    """The 48 dev sentences of tests/golden/batching_golden.npz: one-hot,
    single-rooted and projective, so eligible under both families and both
    root modes (on potentials that allow every arc)."""
    m, data = TL.dev_model(device="cpu", structured_loss="nonprojective")
    assert len(data) == 48
    o = m.params["output_size"]
    seen = 0
    for feed in TL.dev_feeds(m, data, count=len(data)):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        n = m._loss_n_nodes(feed)
        assert n is not None and n.dtype == np.int32 and (n >= 2).all()
        y = np.asarray(feed["target_values_head"], np.float32).reshape(b, v, o)
        p = np.full((b, v, o), 1.0 / o, np.float32)
        for family in FAMILIES:
            for single_root in (True, False):
                assert E.gold_tree_ok(y, p, n, family, single_root).all(), (family, single_root)
        seen += b
    assert seen == 48
    # a feed whose masks are not in closed form: the local loss for the batch
    feed = dict(feed, node_mask=np.asarray(feed["node_mask"]) * 0.5)
    assert m._loss_n_nodes(feed).tolist() == [0] * int(feed["num_graphs"])
