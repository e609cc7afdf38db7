"""ggnn_projective_sample on the GPU against the host form in float64
(evaluation.projective_sample_arrays) on the same seed: status, the contract of
the samples (projective trees over allowed arcs, the root count, -1 / -inf
where it says), the trees themselves under the explained-difference rule of
tests/projective_sample_cases.py (a GPU sample may differ from the host's only
where the host's margin is below the graph's bar marg_bar(n, span_max); at most
2 % of the table's samples may differ at all), logz within marg_bar / 4,
log_prob within
  marg_bar / 4 + |ln Z| 2^-23 + 2^-22 * sum_d |ln p[d][head_d]|
(the first two terms: the bound on ln Z, the last: fp32 ln and the final
rounding), bit-reproducibility, the independence of a sample from num_samples,
from the chunk it falls into and from whose workspace is used, one small
distribution (4096 samples of a flat 5-node graph), the binding's checks and
the model's predict_batch(sample_family="projective") / sample_trees(family=),
eager and with captured steps."""
import numpy as np
import pytest

from decode_cases import _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from projective_sample_cases import (ALL_LAUNCHES, CHUNK, DIFFER_SHARE, K, SEED, P, check_samples, differing, flat_five,
                                     launch_ids, marg_bar, reference, sample_reference, unexplained)

pytestmark = pytest.mark.gpu

TALLY = {"samples": 0, "differ": 0, "log_prob": 0.0, "logz": 0.0, "margin": 0.0}


def _launch(torch, p, n, single_root, num_samples=K, seed=SEED, workspace=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    oh = OutputHeads(64)
    heads, log_prob, status, logz = oh.projective_sample(t(p), t(n), num_samples, seed, single_root, workspace)
    torch.cuda.synchronize()
    assert heads.dtype == torch.int32 and log_prob.dtype == torch.float32 and status.dtype == torch.int32
    assert logz.dtype == torch.float32
    return heads.cpu().numpy(), log_prob.cpu().numpy(), status.cpu().numpy(), logz.cpu().numpy()


def _check_against_host(p, n, span_max, h_logz, ref, got, what):
    """The explained-difference rule and the logz / log_prob bounds of one
    launch; returns (status-1 samples, differing samples)."""
    heads, log_prob, status, logz = got
    h_heads, _, h_status, margin = ref[:4]
    assert np.array_equal(status, h_status), (what, status, h_status)
    diff = differing(h_heads, heads, status)
    for g, s in np.argwhere(diff):
        TALLY["margin"] = max(TALLY["margin"], margin[g, s] / marg_bar(int(n[g]), float(span_max[g])))
    bad = unexplained(diff, margin, n, span_max)
    assert not bad, "%s: (graph, sample, margin, bar) differ unexplained: %s" % (what, bad)
    if logz is not None:
        for g in range(len(n)):
            if not np.isfinite(h_logz[g]) or min(int(n[g]), p.shape[1]) < 2:
                assert logz[g] == h_logz[g], (what, g, logz[g], h_logz[g])
                continue
            bound = marg_bar(int(n[g]), span_max[g]) / 4
            err = abs(float(logz[g]) - float(h_logz[g]))
            TALLY["logz"] = max(TALLY["logz"], err / bound)
            assert err <= bound, (what, g, err, bound)
    for g, s in np.argwhere(status == 1):
        m = int(n[g])
        terms = np.log(p[g, np.arange(1, m), heads[g, s, 1:m]].astype(np.float64))
        bound = marg_bar(m, span_max[g]) / 4 + abs(h_logz[g]) * 2.0 ** -23 + 2.0 ** -22 * np.abs(terms).sum()
        err = abs(float(log_prob[g, s]) - (terms.sum() - float(h_logz[g])))
        TALLY["log_prob"] = max(TALLY["log_prob"], err / bound)
        assert err <= bound, (what, g, s, err, bound)
    return int((status == 1).sum()), int(diff.sum())


def _tally():
    return ("%d of %d samples differ (explained; largest margin / bar %.3g), largest logz error / bound %.3g, largest "
            "log_prob error / bound %.3g" % (TALLY["differ"], TALLY["samples"], TALLY["margin"], TALLY["logz"],
                                             TALLY["log_prob"]))


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=launch_ids)
def test_kernel_samples_equal_host_samples(shape, k):
    torch = _torch()
    p, n, kinds, allowed, host = reference(shape, k)
    for single_root in (False, True):
        _, h_logz, _, h_status, span_max = host[single_root]
        got = _launch(torch, p, n, single_root)
        assert got[0].shape == (shape[0], K, shape[1])
        check_samples(p, n, allowed, h_status, single_root, *got[:3])
        total, differ = _check_against_host(p, n, span_max, h_logz, sample_reference(shape, k, single_root), got,
                                            (shape, k, single_root))
        TALLY["samples"] += total
        TALLY["differ"] += differ
    print("so far: " + _tally())


def test_share_of_differing_samples():
    """Over the launches above (this test runs after them) at most 2 % of the
    samples differ from the float64 host form's.  Measured on one MI355X: 0 of
    824; logz at most 0.58 of its bound, log_prob at most 0.10 of its own."""
    print(_tally())
    assert TALLY["differ"] <= DIFFER_SHARE * TALLY["samples"]


@pytest.mark.parametrize("shape", [(2, 65, 150), (3, P + 1, max(P + 1, 150))], ids=["lds", "both-tiers"])
def test_bytes_do_not_depend_on_launch_num_samples_or_workspace(shape):
    torch = _torch()
    p, n, _, _, _ = reference(shape, 0)
    b, v, _ = shape
    if v > P:
        assert n.max() > P and n.min() <= P                           # both tiers in one grid
    for single_root in (False, True):
        a = _launch(torch, p, n, single_root)
        c = _launch(torch, p, n, single_root)
        assert (a[2] == 1).any()
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes()
        # K = 4 is a prefix of K = 8, of K = CHUNK and of K = CHUNK + 1 (a second workgroup per graph)
        for more in (2 * K, CHUNK, CHUNK + 1):
            got = _launch(torch, p, n, single_root, more)
            for x, y in zip(a[:3], got[:3]):
                assert x.tobytes() == np.ascontiguousarray(y[:, :K]).tobytes(), more
            assert a[3].tobytes() == got[3].tobytes()
            assert (got[2] == got[2][:, :1]).all()                     # the last chunk's samples: the graph's status
        assert not np.array_equal(a[0], _launch(torch, p, n, single_root, seed=SEED + 1)[0])
        many = CHUNK + 1
        need = 0 if v <= P else b * 2 * 8 * v * (v + 1)
        ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=torch.device("cuda"))
        mine = _launch(torch, p, n, single_root, many)
        own = _launch(torch, p, n, single_root, many, workspace=ws[:need] if need else ws)
        for x, y in zip(mine, own):
            assert x.tobytes() == y.tobytes()
        if need:
            assert (ws[need:].cpu().numpy() == 0xA5).all()            # nothing past the stated bytes
            assert not (ws[:need].cpu().numpy() == 0xA5).all()        # (the tables were written there)
            with pytest.raises(ValueError):
                _launch(torch, p, n, single_root, many, workspace=ws[:need - 1])


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    p = torch.full((2, 4, 6), 0.5, dtype=torch.float32, device=dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    for bad in (dict(probs_head=p.double()), dict(probs_head=p.cpu()), dict(n_nodes=n.long()), dict(n_nodes=n[:1]),
                dict(probs_head=p[:, :, :3]), dict(num_samples=0), dict(num_samples=4097),
                dict(workspace=torch.empty(8, dtype=torch.float32, device=dev)),
                dict(workspace=torch.empty(8, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            oh.projective_sample(**dict(dict(probs_head=p, n_nodes=n, num_samples=2), **bad))
    heads, log_prob, status, logz = oh.projective_sample(p, n, 2)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [[1, 1], [1, 1]] and (heads[:, :, 1:].cpu().numpy() >= 0).all()
    assert np.isfinite(logz.cpu().numpy()).all()


def test_flat_five_node_distribution():
    """One flat 5-node graph, 4096 samples, both root modes: every sample is
    the float64 host form's, or an explained one (the host's own frequencies
    are held to the exact weight / Z by the forced form's test)."""
    torch = _torch()
    p, n = flat_five()
    for single_root in (False, True):
        span_max = E.projective_marginals_arrays(p, n, single_root)[4]
        h_heads, _, h_status, margin, _ = E.projective_sample_arrays(p, n, 4096, 3, single_root)
        heads, log_prob, status, _ = _launch(torch, p, n, single_root, 4096, 3)
        assert (status == 1).all() and (h_status == 1).all()
        diff = differing(h_heads, heads, status)
        bad = unexplained(diff, margin, n, span_max)
        assert not bad, bad
        trees = {tuple(h) for h in heads[0]}
        assert all(E.is_tree(h, 5, single_root) and E.is_projective(h, 5) for h in trees)
        print("single_root %d: %d distinct trees, %d of 4096 samples differ (explained)"
              % (single_root, len(trees), int(diff.sum())))


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_model_samples_agree_with_the_host_chain(graphs):
    torch = _torch()
    from ggnn_amd.decoding import HostDecoder, decode_chain
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    trees, log_probs = m.sample_trees(raw, 3, seed=5, family="projective")
    assert m.sample_trees(raw, 3, seed=5, family="projective") == (trees, log_probs)
    plain = m.sample_trees(raw, 3, seed=5)
    assert plain == m.sample_trees(raw, 3, seed=5, family="nonprojective")
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o, oe = m.params["output_size"], m.output_size_edges
    compared = 0
    for i, feed in enumerate(m.make_minibatch_iterator(data, False)):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        p0 = m.predict_batch(dict(feed), samples=3, sample_seed=5 + i)
        named = m.predict_batch(dict(feed), samples=3, sample_seed=5 + i, sample_family="nonprojective")
        assert set(named) == set(p0)
        for key in p0:                                                  # the default family: byte for byte
            assert np.asarray(named[key]).tobytes() == np.asarray(p0[key]).tobytes(), key
        got = m.predict_batch(dict(feed), samples=3, sample_seed=5 + i, sample_family="projective")
        assert set(got) == set(p0) and np.array_equal(got["heads"], p0["heads"])
        hp = m.ops["computed_values"].detach().reshape(b, v, o).cpu().numpy()
        hp_e = m.ops["computed_values_edges"].detach().reshape(b, v, oe).cpu().numpy()
        n = np.asarray(got["n_nodes"], np.int32)
        host = decode_chain(HostDecoder(), hp, hp_e, n, None, False, True, False, 3, 5 + i, "projective")
        _, h_logz, _, h_status, span_max = E.projective_marginals_arrays(hp, n, True)
        ref = E.projective_sample_arrays(hp, n, 3, 5 + i, True)
        assert np.array_equal(ref[0], host["sampled_heads"]) and np.array_equal(ref[2], host["sample_status"])
        _check_against_host(hp, n, span_max, h_logz, ref,
                            (got["sampled_heads"], got["sample_log_prob"], got["sample_status"], None), ("batch", i))
        for g, s in np.argwhere(got["sample_status"] == 1):
            assert E.is_projective(got["sampled_heads"][g, s], int(n[g]))
        for g, k in enumerate(got["sentences_id"]):                     # sample_trees: the same draws, as lists
            m_g = int(n[g])
            assert [[h for h, _ in t] for t in trees[k]] == [list(map(int, x[1:m_g])) for x in got["sampled_heads"][g]]
            assert log_probs[k] == [float(x) for x in got["sample_log_prob"][g]]
        compared += b
    assert compared == len(raw)
