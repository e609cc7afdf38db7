"""ggnn_tree_marginals on the GPU against the host form in float64
(evaluation.tree_marginals_arrays): status, the arcs that are not allowed,
untouched graphs, the error bar of the issue on marg, logz and the row sums,
the integer scores, the projective marginals below four nodes,
reproducibility at both storage tiers, the binding's checks, the model's
tree="mbr" / confidence="nonprojective" keywords and decode_chain on both
backends.  The table, the builders and the bar are those of
tests/test_tree_marginals.py (where the table's cap, bar <= 2^-6, is
asserted): bar = n * cond * 2^-24 for a marginal, bar / 4 + |ln Z| * 2^-23 for
ln Z, n * 2^-20 + bar for a row sum."""
import numpy as np
import pytest

from decode_cases import _batch_bytes, _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from ggnn_amd._lib import LAPL_LDS_MAXN as L
from test_projective_marginals import SCALE, marg_bar
from test_tree_decode import F
from test_tree_marginals import ALL_LAUNCHES, CAP, check_tree_mbr_parse, lapl_bar, launch_ids, reference

pytestmark = pytest.mark.gpu

WORST = {"marg": 0.0, "logz": 0.0, "rows": 0.0}


def _launch(torch, p, n, single_root, with_scores=True, workspace=None, name="tree_marginals"):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    oh = OutputHeads(64)
    marg, logz, scores, status = getattr(oh, name)(t(p), t(n), single_root, with_scores, workspace)
    torch.cuda.synchronize()
    assert marg.dtype == torch.float32 and logz.dtype == torch.float32 and status.dtype == torch.int32
    return (marg.cpu().numpy(), logz.cpu().numpy(), None if scores is None else scores.cpu().numpy(),
            status.cpu().numpy())


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=launch_ids)
def test_kernel_equals_host_marginals(shape, k):
    torch = _torch()
    b, v, o = shape
    p, n, kinds, allowed, host = reference(shape, k)
    for single_root in (False, True):
        h_marg, h_logz, h_scores, h_status, cond = host[single_root]
        marg, logz, scores, status = _launch(torch, p, n, single_root)
        assert np.array_equal(status, h_status), (status, h_status, kinds, n)
        small = None
        for g in range(b):
            m = int(n[g])
            if status[g] != 1:
                assert marg[g].tobytes() == p[g].tobytes() and (scores[g] == F).all()
                assert logz[g] == (-np.inf if status[g] == 2 else 0)
                continue
            ok = allowed[g]
            assert np.array_equal(ok, h_scores[g] != F)
            assert np.isfinite(marg[g]).all() and (marg[g][~ok] == 0).all() and (scores[g][~ok] == F).all()
            assert (scores[g][ok] != F).all() and (marg[g] >= 0).all() and (marg[g] <= 1).all()
            # the device's own outputs: the scores of its marginals, the rows of a distribution
            assert np.array_equal(scores[g][ok], np.rint(marg[g][ok] * np.float32(SCALE)).astype(np.int32))
            rows = np.abs(marg[g, 1:m].astype(np.float64).sum(axis=1) - 1).max()
            # against float64
            bar = lapl_bar(m, cond[g])
            bar_z = bar / 4 + abs(h_logz[g]) * 2.0 ** -23
            err = np.abs(marg[g].astype(np.float64) - h_marg[g]).max()
            err_z = abs(float(logz[g]) - h_logz[g])
            print("n %d %s single_root %d: cond %.3g, marg err %.3g (bar %.3g, ratio %.3g), logz err %.3g (bound "
                  "%.3g, ratio %.3g), row sums off by %.3g (bound %.3g)"
                  % (m, kinds[g], single_root, cond[g], err, bar, err / bar, err_z, bar_z, err_z / bar_z, rows,
                     m * 2.0 ** -20 + bar))
            WORST["marg"] = max(WORST["marg"], err / bar)
            WORST["logz"] = max(WORST["logz"], err_z / bar_z)
            WORST["rows"] = max(WORST["rows"], rows / (m * 2.0 ** -20 + bar))
            assert bar <= CAP
            assert rows <= m * 2.0 ** -20 + bar, (kinds[g], m, rows)
            assert err <= bar, (kinds[g], m, err, bar)
            assert err_z <= bar_z, (kinds[g], m, err_z, bar_z)
            # below four nodes no two arcs can cross: the projective kernel's output of the same launch
            if m <= 3:
                if small is None:
                    small = _launch(torch, p, n, single_root, name="projective_marginals")
                    span_max = E.projective_marginals_arrays(p, n, single_root)[4]
                assert small[3][g] == 1
                both = bar + marg_bar(m, span_max[g])
                assert np.abs(marg[g].astype(np.float64) - small[0][g]).max() <= both
                assert abs(float(logz[g]) - float(small[1][g])) <= bar_z + marg_bar(m, span_max[g]) / 4
    print("largest error / bar so far: marg %.3g, logz %.3g, row sums %.3g" % (WORST["marg"], WORST["logz"],
                                                                                WORST["rows"]))


@pytest.mark.parametrize("shape", [(2, 65, 150), (3, L + 1, max(L + 1, 150))], ids=["lds", "both-tiers"])
def test_two_launches_give_identical_bytes(shape):
    torch = _torch()
    p, n, _, _, _ = reference(shape, 0)
    if shape[1] > L:
        assert n.max() > L and n.min() <= L                           # both tiers in one grid
    for single_root in (False, True):
        a = _launch(torch, p, n, single_root)
        b = _launch(torch, p, n, single_root)
        assert (a[3] == 1).any()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        c = _launch(torch, p, n, single_root, with_scores=False)      # scores are optional: the same marginals
        assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    p = torch.full((2, 4, 6), 0.5, dtype=torch.float32, device=dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    for bad in (dict(probs_head=p.double()), dict(probs_head=p.cpu()), dict(n_nodes=n.long()), dict(n_nodes=n[:1]),
                dict(probs_head=p[:, :, :3]), dict(probs_head=p[0]), dict(probs_head=p.transpose(1, 2)),
                dict(probs_head=torch.zeros(2, 8, 6, dtype=torch.float32, device=dev))):
        with pytest.raises(ValueError):
            oh.tree_marginals(**dict(dict(probs_head=p, n_nodes=n), **bad))
    # a workspace too small for graphs above LAPL_LDS_MAXN nodes
    v = L + 1
    p = torch.full((2, v, v), 0.5, dtype=torch.float32, device=dev)
    need = 2 * 4 * (v - 1) * ((v - 1) | 1)
    with pytest.raises(ValueError):
        oh.tree_marginals(p, n, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        oh.tree_marginals(p, n, workspace=torch.empty(need, dtype=torch.int32, device=dev))
    out = oh.tree_marginals(p, n, workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert out[3].cpu().tolist() == [1, 1]
    assert torch.allclose(out[0][:, 1:4, :4].sum(dim=2), torch.ones(2, 3, device=dev), atol=1e-5)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_model_mbr_and_confidence(graphs):
    torch = _torch()
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    check_tree_mbr_parse(m, raw)
    data = m.process_raw_graphs(raw, False)
    o = m.params["output_size"]
    seen = np.zeros(3, int)
    tot = [0, 0.0, 0.0, 0.0]
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        mst = m.predict_batch(dict(feed), tree=True, confidence="nonprojective")
        p = m.predict_batch(dict(feed), tree="mbr", confidence="nonprojective")
        assert np.array_equal(p["labels"], mst["labels"])
        # the device's own marginals and scores of the batch the model holds
        probs = m.ops["computed_values"].detach().reshape(b, v, o).contiguous()
        n_dev = torch.from_numpy(np.asarray(p["n_nodes"], np.int32)).to(probs.device)
        marg, logz, scores, status = m._decode_heads().tree_marginals(probs, n_dev, True)
        marg, scores = marg.cpu().numpy(), scores.cpu().numpy()
        assert (status.cpu().numpy() == 1).all() and (p["tree_status"] != 2).all()
        seen += [int((p["tree_status"] == k).sum()) for k in (0, 1, 2)]
        for q in (mst, p):                                            # confidences: the marginals at the returned heads
            pred = np.stack([q["heads"], q["labels"]], axis=2)
            assert q["head_confidence"].tobytes() == E.arc_confidence_arrays(marg, q["n_nodes"], pred).tobytes()
            assert q["log_partition"].tobytes() == logz.cpu().numpy().tobytes()
        for g in range(b):
            n = int(p["n_nodes"][g])
            arg = np.full((1, v, 2), -1, np.int32)
            host, _, st = E.tree_decode_arrays(scores[g][None], [n], arg, True)
            assert st[0] == 1 and E.is_tree(p["heads"][g], n, True, scores[g])
            assert E.tree_total(scores[g], p["heads"][g], n) == E.tree_total(scores[g], host[0, :, 0], n)
        # evaluate_batch: host scores of the returned heads
        gold = m._decode_forward(dict(feed), True)["gold"].cpu().numpy()
        pred = np.stack([p["heads"], p["labels"]], axis=2)
        host = [0.0, 0.0, 0.0]
        for g in range(b):
            x = E.graph_scores_from_lists(pred[g], gold[g])
            for c in range(3):
                host[c] += x[c]
        host = tuple(x / b for x in host)
        assert m.evaluate_batch(dict(feed), on_device=True, tree="mbr") == host
        tot[0] += b
        for c in range(3):
            tot[1 + c] += host[c] * b
    assert seen[0] + seen[1] == tot[0] and seen[1] > 0, seen
    plain = m.score_epoch(data)
    m.score_epoch(data, tree=True)
    torch.cuda.synchronize()
    tree_bytes = m.decode_stats["d2h_bytes"]
    got = m.score_epoch(data, tree="mbr")
    torch.cuda.synchronize()
    st = m.decode_stats
    assert st["d2h_bytes"] == tree_bytes == _batch_bytes(m, data, 6)  # the loss, [b, 5] counts and [b] status
    assert st["repaired_graphs"] == seen[1] and st["infeasible_graphs"] == 0 and st["fallback_graphs"] == 0, st
    assert got[1:4] == (tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0]), (got, tot)
    assert got[0] == plain[0] and got[3] == plain[3] and got[5] == plain[5]
    assert m.score_epoch(data)[:4] == plain[:4]


def test_decode_chain_agrees_on_both_backends():
    """One forward, decode_chain through the device binding and through the
    host adapter on the fetched probabilities."""
    torch = _torch()
    from ggnn_amd.decoding import HostDecoder, decode_chain
    m = _synthetic_model(False)
    data = m.process_raw_graphs(_synthetic_raw(), False)
    o, oe = m.params["output_size"], m.output_size_edges
    compared = 0
    for feed in m.make_minibatch_iterator(data, False):
        m._eval_forward(dict(feed))
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        n = m._feed_n_nodes(m.placeholders)
        probs = m.ops["computed_values"].detach().reshape(b, v, o).contiguous()
        probs_e = m.ops["computed_values_edges"].detach().reshape(b, v, oe).contiguous()
        n_dev = torch.from_numpy(n).to(probs.device)
        dev = decode_chain(m._decode_heads(), probs, probs_e, n_dev, None, "mbr", True, "nonprojective")
        torch.cuda.synchronize()
        hp = probs.cpu().numpy()
        host = decode_chain(HostDecoder(), hp, probs_e.cpu().numpy(), n, None, "mbr", True, "nonprojective")
        h_marg, h_logz, _, h_status, cond = E.tree_marginals_arrays(hp, n, True)
        assert (h_status == 1).all()
        for key in ("pred", "counts", "tree_status"):
            assert dev[key].dtype == torch.int32 and np.array_equal(dev[key].cpu().numpy(), host[key]), key
        conf, logz = dev["head_confidence"].cpu().numpy().astype(np.float64), dev["log_partition"].cpu().numpy()
        for g in range(b):
            bar = lapl_bar(int(n[g]), cond[g])
            assert np.abs(conf[g] - host["head_confidence"][g]).max() <= bar + 2.0 ** -24   # (host: rounded to fp32)
            assert abs(float(logz[g]) - h_logz[g]) <= bar / 4 + abs(h_logz[g]) * 2.0 ** -23
        compared += b
    assert compared > 0
