"""ggnn_tree_sample on the GPU against the host form in float64
(evaluation.tree_sample_arrays) on the same seed: status, the contract of the
samples (trees over allowed arcs, the root count, -1 / -inf where it says), the
trees themselves under the explained-difference rule of
tests/tree_sample_cases.py (a GPU sample may differ from the host's only where
the host's margin is below the graph's bar n * cond * 2^-24; at most 2 % of the
table's samples may differ at all), log_prob within
  bar / 4 + |ln Z| 2^-23 + 2^-22 * sum_d |ln p[d][head_d]|
(the first two terms: the bound on the marginal kernel's logz, the last: fp32
ln and the final rounding), bit-reproducibility, the independence of a sample
from num_samples and from whose workspace is used, one small distribution
(4096 samples of a flat 5-node graph) and the model's predict_batch(samples=) /
sample_trees, eager and with captured steps."""
import numpy as np
import pytest

from decode_cases import _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from ggnn_amd._lib import SAMPLE_LDS_MAXN as L
from tree_sample_cases import (ALL_LAUNCHES, DIFFER_SHARE, K, SEED, check_samples, differing, lapl_bar, launch_ids,
                               reference, sample_reference, unexplained)

pytestmark = pytest.mark.gpu

TALLY = {"samples": 0, "differ": 0, "log_prob": 0.0}


def _launch(torch, p, n, single_root, num_samples=K, seed=SEED, workspace=None, marginals=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    oh = OutputHeads(64)
    heads, log_prob, status = oh.tree_sample(t(p), t(n), num_samples, seed, single_root, marginals, workspace)
    torch.cuda.synchronize()
    assert heads.dtype == torch.int32 and log_prob.dtype == torch.float32 and status.dtype == torch.int32
    return heads.cpu().numpy(), log_prob.cpu().numpy(), status.cpu().numpy()


def _check_against_host(p, n, cond, h_logz, ref, got, what):
    """The explained-difference rule and the log_prob bound of one launch;
    returns (status-1 samples, differing samples)."""
    heads, log_prob, status = got
    h_heads, _, h_status, margin = ref
    assert np.array_equal(status, h_status), (what, status, h_status)
    diff = differing(h_heads, heads, status)
    bad = unexplained(diff, margin, n, cond)
    assert not bad, "%s: (graph, sample, margin, bar) differ unexplained: %s" % (what, bad)
    for g, s in np.argwhere(status == 1):
        m = int(n[g])
        terms = np.log(p[g, np.arange(1, m), heads[g, s, 1:m]].astype(np.float64))
        bound = lapl_bar(m, cond[g]) / 4 + abs(h_logz[g]) * 2.0 ** -23 + 2.0 ** -22 * np.abs(terms).sum()
        err = abs(float(log_prob[g, s]) - (terms.sum() - float(h_logz[g])))
        TALLY["log_prob"] = max(TALLY["log_prob"], err / bound)
        assert err <= bound, (what, g, s, err, bound)
    return int((status == 1).sum()), int(diff.sum())


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=launch_ids)
def test_kernel_samples_equal_host_samples(shape, k):
    torch = _torch()
    p, n, kinds, allowed, host = reference(shape, k)
    for single_root in (False, True):
        _, h_logz, _, h_status, cond = host[single_root]
        got = _launch(torch, p, n, single_root)
        assert got[0].shape == (shape[0], K, shape[1])
        check_samples(p, n, allowed, h_status, single_root, *got)
        total, differ = _check_against_host(p, n, cond, h_logz, sample_reference(shape, k, single_root), got,
                                            (shape, k, single_root))
        TALLY["samples"] += total
        TALLY["differ"] += differ
    print("so far: %d of %d samples differ (explained), largest log_prob error / bound %.3g"
          % (TALLY["differ"], TALLY["samples"], TALLY["log_prob"]))


def test_share_of_differing_samples():
    """Over the launches above (this test runs after them) at most 2 % of the
    samples differ from the float64 host form's."""
    print("%d of %d samples differ, largest log_prob error / bound %.3g"
          % (TALLY["differ"], TALLY["samples"], TALLY["log_prob"]))
    assert TALLY["differ"] <= DIFFER_SHARE * TALLY["samples"]


@pytest.mark.parametrize("shape", [(2, 65, 150), (3, L + 1, max(L + 1, 150))], ids=["lds", "both-tiers"])
def test_bytes_do_not_depend_on_launch_num_samples_or_workspace(shape):
    torch = _torch()
    p, n, _, _, _ = reference(shape, 0)
    b, v, _ = shape
    if v > L:
        assert n.max() > L and n.min() <= L                           # both tiers in one grid
    for single_root in (False, True):
        a = _launch(torch, p, n, single_root)
        c = _launch(torch, p, n, single_root)
        assert (a[2] == 1).any()
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes()
        eight = _launch(torch, p, n, single_root, 2 * K)
        for x, y in zip(a, eight):
            assert x.tobytes() == np.ascontiguousarray(y[:, :K]).tobytes()
        assert not np.array_equal(a[0], _launch(torch, p, n, single_root, seed=SEED + 1)[0])
        need = 0 if v <= L else b * K * 4 * (v - 1) * ((v - 1) | 1)
        ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=torch.device("cuda"))
        own = _launch(torch, p, n, single_root, workspace=ws)
        for x, y in zip(a, own):
            assert x.tobytes() == y.tobytes()
        if need:
            assert (ws[need:].cpu().numpy() == 0xA5).all()            # nothing past the stated bytes
            with pytest.raises(ValueError):
                _launch(torch, p, n, single_root, workspace=ws[:need - 1])


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    p = torch.full((2, 4, 6), 0.5, dtype=torch.float32, device=dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    good = oh.tree_marginals(p, n, True, with_scores=False)
    for bad in (dict(probs_head=p.double()), dict(probs_head=p.cpu()), dict(n_nodes=n.long()), dict(n_nodes=n[:1]),
                dict(probs_head=p[:, :, :3]), dict(num_samples=0), dict(num_samples=4097),
                dict(marginals=(good[0][:1],) + good[1:]), dict(marginals=(good[0], good[1], None, good[3].long()))):
        with pytest.raises(ValueError):
            oh.tree_sample(**dict(dict(probs_head=p, n_nodes=n, num_samples=2), **bad))
    heads, log_prob, status = oh.tree_sample(p, n, 2, marginals=good)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [[1, 1], [1, 1]] and (heads[:, :, 1:].cpu().numpy() >= 0).all()


def test_flat_five_node_distribution():
    """One flat 5-node graph, 4096 samples, both root modes: the multiset of
    trees is the float64 host form's up to explained samples (the host's own
    frequencies are held to the exact weight / Z by the forced form's test)."""
    torch = _torch()
    rng = np.random.default_rng(77)
    p = (0.2 + rng.random((1, 5, 8))).astype(np.float32)
    n = np.asarray([5], np.int32)
    for single_root in (False, True):
        cond = E.tree_marginals_arrays(p, n, single_root)[4]
        h_heads, _, h_status, margin = E.tree_sample_arrays(p, n, 4096, 3, single_root)
        heads, log_prob, status = _launch(torch, p, n, single_root, 4096, 3)
        assert (status == 1).all() and (h_status == 1).all()
        diff = differing(h_heads, heads, status)
        bad = unexplained(diff, margin, n, cond)
        assert not bad, bad
        trees = {tuple(h) for h in heads[0]}
        assert all(E.is_tree(h, 5, single_root) for h in trees)
        assert len(trees) > (30 if single_root else 60)                 # of 64 / 125 trees
        print("single_root %d: %d distinct trees, %d of 4096 samples differ (explained)"
              % (single_root, len(trees), int(diff.sum())))


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_model_samples_agree_with_the_host_chain(graphs):
    torch = _torch()
    from ggnn_amd.decoding import HostDecoder, decode_chain
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    trees, log_probs = m.sample_trees(raw, 3, seed=5)
    assert m.sample_trees(raw, 3, seed=5) == (trees, log_probs)
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o, oe = m.params["output_size"], m.output_size_edges
    compared = 0
    for i, feed in enumerate(m.make_minibatch_iterator(data, False)):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p0 = m.predict_batch(dict(feed))
        got = m.predict_batch(dict(feed), samples=3, sample_seed=5 + i)
        assert set(got) == set(p0) | {"sampled_heads", "sample_log_prob", "sample_status"}
        assert np.array_equal(got["heads"], p0["heads"])
        hp = m.ops["computed_values"].detach().reshape(b, v, o).cpu().numpy()
        hp_e = m.ops["computed_values_edges"].detach().reshape(b, v, oe).cpu().numpy()
        n = np.asarray(got["n_nodes"], np.int32)
        host = decode_chain(HostDecoder(), hp, hp_e, n, None, False, True, False, 3, 5 + i)
        _, h_logz, _, h_status, cond = E.tree_marginals_arrays(hp, n, True)
        ref = E.tree_sample_arrays(hp, n, 3, 5 + i, True)
        assert np.array_equal(ref[0], host["sampled_heads"]) and np.array_equal(ref[2], host["sample_status"])
        _check_against_host(hp, n, cond, h_logz, ref,
                            (got["sampled_heads"], got["sample_log_prob"], got["sample_status"]), ("batch", i))
        with_mbr = m.predict_batch(dict(feed), tree="mbr", samples=3, sample_seed=5 + i)   # the chain's own marginals
        assert with_mbr["sampled_heads"].tobytes() == got["sampled_heads"].tobytes()
        for g, k in enumerate(got["sentences_id"]):                     # sample_trees: the same draws, as lists
            m_g = int(n[g])
            assert [[h for h, _ in t] for t in trees[k]] == [list(map(int, x[1:m_g])) for x in got["sampled_heads"][g]]
            assert all([l - 1 for _, l in t] == list(map(int, got["labels"][g, 1:m_g])) for t in trees[k])
            assert log_probs[k] == [float(x) for x in got["sample_log_prob"][g]]
        compared += b
    assert compared == len(raw)
