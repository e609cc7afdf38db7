"""ggnn_projective_marginals / ggnn_arc_confidence on the GPU against the host
form in float64 (evaluation.projective_marginals_arrays): status, the arcs
that are not allowed, untouched graphs, the error bar of the issue on marg and
logz, the integer scores, row sums, reproducibility at both storage tiers, the
binding's checks, and the model's tree="projective-mbr" / confidence keywords.

Error bar (fp32 tables in log space): every table entry is one log-sum-exp of
at most n terms, (log2 n + 4) 2^-24 in the log plus the rounding of stored
values of magnitude <= span_max; an entry depends on a chain of at most n
lengths going in and n coming out; a marginal combines an inside value, an
outside value and logz: 4 n (log2 n + 4 + span_max) 2^-24, a quarter of it for
logz.  span_max is the host form's (potentials as given; the kernel's tables
hold smaller values, it subtracts every row's largest ln p first).  It covers
logz as well as the tables: with single_root logz is no table entry, and at n
= 2 there is no table at all, while logz = ln p of the one arc is stored in
fp32 like any other value (|logz| in 16..32 has half an ulp of 9.5e-7, above
n (log2 n + 4) 2^-24 = 6e-7)."""
import numpy as np
import pytest

from decode_cases import _batch_bytes, _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from ggnn_amd._lib import MARG_LDS_MAXN as M
from test_projective_decode import only_crossing_tree
from test_projective_marginals import SCALE, check_mbr_parse, marg_bar, probs_of_scores, random_probs
from test_tree_decode import F, closed_group, forbidden_row

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 150),                       # the smallest bucket
          (3, 8, 8),                         # v = o
          (2, 64, 64),                       # exact wave width
          (2, 65, 150),                      # one past it
          (3, M, max(M, 150)),               # the largest graphs with tables in LDS
          (3, M + 1, max(M + 1, 150)),       # both storage tiers in one grid
          (1, 198, 198),                     # the largest reference bucket
          (1, 256, 256)]                     # GGNN_TREE_MAXV
KINDS = ("flat", "sparse", "peaked", "tiny")


def _node_counts(v):
    """2, an interior value and v; around MARG_LDS_MAXN also M - 1, M and one
    short graph."""
    out = [v, 5] if v == M + 1 else [v]      # (first: n = M + 1 and n = 5 share a launch)
    out += [2, max(2, min(v - 1, v // 2 + 1))]
    if v in (M, M + 1):
        out += [x for x in (M - 1, M) if x < v]
    return list(dict.fromkeys(out))


def _launches(shape):
    """The launches of a shape as lists of b (n, kind): every node count with
    every kind of input; graph 1 of every launch (b = 1: launches of their
    own) has no projective tree."""
    b, v, o = shape
    counts = _node_counts(v)
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


def _infeasible(n, o, k):
    if n == 2:
        return np.zeros((2, o), np.float32)
    if n < 5:
        return probs_of_scores(closed_group(n), o)
    return probs_of_scores((only_crossing_tree, closed_group, forbidden_row)[k % 3](n), o)


_REFERENCE = {}


def _reference(shape, k):
    """One launch's input and both host results in float64 (single_root False /
    True), computed once and left unchanged.  Graph 0 carries a NaN in a row <
    n; rows and columns >= n hold values that must never be read as arcs."""
    key = (shape, k)
    if key not in _REFERENCE:
        b, v, o = shape
        part = _launches(shape)[k]
        rng = np.random.default_rng(7000 + 100 * v + k)
        n = np.asarray([x[0] for x in part], np.int32)
        kinds = [x[1] for x in part]
        p = rng.random((b, v, o)).astype(np.float32)              # (padding: plain positive numbers)
        for g in range(b):
            m = int(n[g])
            p[g, :m, :] = _infeasible(m, o, k) if kinds[g] == "infeasible" else random_probs(m, o, kinds[g], rng)
        m = int(n[0])
        if m >= 3:
            p[0, 2, 1] = np.nan                                       # an arc that is simply not allowed
        else:
            p[0, 0, 1] = np.nan                                       # row 0 < n: never an arc
        host = {sr: E.projective_marginals_arrays(p, n, sr) for sr in (False, True)}
        allowed = E.tree_scores(p, n, v) != F
        for a in (p, n, allowed) + host[False] + host[True]:
            a.setflags(write=False)
        _REFERENCE[key] = (p, n, kinds, allowed, host)
    return _REFERENCE[key]


def _launch(torch, p, n, single_root, with_scores=True, workspace=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    oh = OutputHeads(64)
    marg, logz, scores, status = oh.projective_marginals(t(p), t(n), single_root, with_scores, workspace)
    torch.cuda.synchronize()
    assert marg.dtype == torch.float32 and logz.dtype == torch.float32 and status.dtype == torch.int32
    return (marg.cpu().numpy(), logz.cpu().numpy(), None if scores is None else scores.cpu().numpy(),
            status.cpu().numpy())


ALL_LAUNCHES = [(shape, k) for shape in SHAPES for k in range(len(_launches(shape)))]
WORST = {"marg": 0.0, "logz": 0.0}


def test_the_launches_cover_the_issue():
    for shape in SHAPES:
        b, v, o = shape
        seen = set()
        for part in _launches(shape):
            assert len(part) == b
            seen |= {x for x in part if x[1] != "infeasible"}
            assert (b == 1 and len(part) == 1) or part[1][1] == "infeasible"
        assert any(x[1] == "infeasible" for part in _launches(shape) for x in part)
        counts = {x[0] for x in seen}
        assert {2, v} <= counts and any(2 < x < v for x in counts)
        assert {(v, kind) for kind in KINDS} <= seen
        if v == M:
            assert {M - 1, M} <= counts
        if v == M + 1:
            assert {M - 1, M, M + 1} <= counts
            assert any({M + 1, 5} <= {x[0] for x in part} for part in _launches(shape))


@pytest.mark.parametrize("shape,k", ALL_LAUNCHES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_kernel_equals_host_marginals(shape, k):
    torch = _torch()
    b, v, o = shape
    p, n, kinds, allowed, host = _reference(shape, k)
    for single_root in (False, True):
        h_marg, h_logz, h_scores, h_status, span_max = host[single_root]
        for g, what in enumerate(kinds):                              # the cases are what they claim to be
            if what != "sparse" or n[g] > 8:                          # (a small sparse graph may have no tree)
                assert h_status[g] == (2 if what == "infeasible" else 1), (what, n[g])
        marg, logz, scores, status = _launch(torch, p, n, single_root)
        assert np.array_equal(status, h_status), (status, h_status, kinds, n)
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
            bar = marg_bar(m, span_max[g])
            err = np.abs(marg[g].astype(np.float64) - h_marg[g]).max()
            err_z = abs(float(logz[g]) - h_logz[g])
            print("n %d %s single_root %d: marg err %.3g (bar %.3g, ratio %.3g), logz err %.3g (ratio %.3g), "
                  "row sums off by %.3g (bound %.3g)" % (m, kinds[g], single_root, err, bar, err / bar, err_z,
                                                         err_z / (bar / 4), rows, m * 2.0 ** -20))
            WORST["marg"] = max(WORST["marg"], err / bar)
            WORST["logz"] = max(WORST["logz"], err_z / (bar / 4))
            assert rows <= m * 2.0 ** -20, (kinds[g], m, rows)
            assert err <= bar, (kinds[g], m, err, bar)
            assert err_z <= bar / 4, (kinds[g], m, err_z, bar / 4)
    print("largest error / bar so far: marg %.3g, logz %.3g" % (WORST["marg"], WORST["logz"]))


@pytest.mark.parametrize("shape", [(2, 65, 150), (3, M + 1, max(M + 1, 150))], ids=["lds", "both-tiers"])
def test_two_launches_give_identical_bytes(shape):
    torch = _torch()
    p, n, _, _, _ = _reference(shape, 0)
    a = _launch(torch, p, n, True)
    b = _launch(torch, p, n, True)
    assert (a[3] == 1).any()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = _launch(torch, p, n, True, with_scores=False)                 # scores are optional: the same marginals
    assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()


@pytest.mark.parametrize("shape", [(4, 4, 150), (2, 65, 150), (3, M + 1, max(M + 1, 150))], ids=str)
def test_arc_confidence_is_a_gather(shape):
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    b, v, o = shape
    p, n, _, _, _ = _reference(shape, 0)
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    n_dev = torch.from_numpy(np.array(n)).to(dev)
    marg, _, _, _ = oh.projective_marginals(torch.from_numpy(np.array(p)).to(dev), n_dev, True, False)
    rng = np.random.default_rng(v)
    pred = rng.integers(-1, o, (b, v, 2)).astype(np.int32)            # any column, -1 included
    pred[:, 1::2, 0] = marg.cpu().numpy()[:, 1::2].argmax(axis=2)
    conf = oh.arc_confidence(marg, n_dev, torch.from_numpy(pred).to(dev))
    torch.cuda.synchronize()
    host = E.arc_confidence_arrays(marg.cpu().numpy(), n, pred)
    assert conf.dtype == torch.float32 and conf.cpu().numpy().tobytes() == host.tobytes()
    assert (host[:, 0] == 0).all() and (host != 0).any()


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    p = torch.full((2, 4, 6), 0.5, dtype=torch.float32, device=dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    pred = torch.zeros(2, 4, 2, dtype=torch.int32, device=dev)
    for bad in (dict(probs_head=p.double()), dict(probs_head=p.cpu()), dict(n_nodes=n.long()), dict(n_nodes=n[:1]),
                dict(probs_head=p[:, :, :3]), dict(probs_head=p[0]), dict(probs_head=p.transpose(1, 2)),
                dict(probs_head=torch.zeros(2, 8, 6, dtype=torch.float32, device=dev))):
        with pytest.raises(ValueError):
            oh.projective_marginals(**dict(dict(probs_head=p, n_nodes=n), **bad))
    marg = oh.projective_marginals(p, n)[0]
    for bad in (dict(marg=marg.double()), dict(marg=marg.cpu()), dict(n_nodes=n.long()), dict(pred=pred[:, :3]),
                dict(pred=pred.long()), dict(pred=pred.cpu())):
        with pytest.raises(ValueError):
            oh.arc_confidence(**dict(dict(marg=marg, n_nodes=n, pred=pred), **bad))
    # a workspace too small for graphs above MARG_LDS_MAXN nodes
    v = M + 1
    p = torch.full((2, v, v), 0.5, dtype=torch.float32, device=dev)
    need = 2 * 14 * v * (v + 1)
    with pytest.raises(ValueError):
        oh.projective_marginals(p, n, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        oh.projective_marginals(p, n, workspace=torch.empty(need, dtype=torch.int32, device=dev))
    out = oh.projective_marginals(p, n, workspace=torch.empty(need, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert out[3].cpu().tolist() == [1, 1]
    assert torch.allclose(out[0][:, 1:4, :4].sum(dim=2), torch.ones(2, 3, device=dev), atol=1e-5)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_model_mbr_and_confidence(graphs):
    torch = _torch()
    m = _synthetic_model(graphs)
    raw = _synthetic_raw()
    check_mbr_parse(m, raw)
    data = m.process_raw_graphs(raw, False)
    o = m.params["output_size"]
    seen = np.zeros(3, int)
    tot = [0, 0.0, 0.0, 0.0]
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        plain = m.predict_batch(dict(feed), confidence=True)
        p = m.predict_batch(dict(feed), tree="projective-mbr", confidence=True)
        assert np.array_equal(p["labels"], plain["labels"])
        # the device's own marginals and scores of the batch the model holds
        probs = m.ops["computed_values"].detach().reshape(b, v, o).contiguous()
        n_dev = torch.from_numpy(np.asarray(p["n_nodes"], np.int32)).to(probs.device)
        marg, logz, scores, status = m._decode_heads().projective_marginals(probs, n_dev, True)
        marg, scores = marg.cpu().numpy(), scores.cpu().numpy()
        assert (status.cpu().numpy() == 1).all() and (p["tree_status"] != 2).all()
        seen += [int((p["tree_status"] == k).sum()) for k in (0, 1, 2)]
        for q in (plain, p):                                          # confidences: the marginals at the returned heads
            pred = np.stack([q["heads"], q["labels"]], axis=2)
            assert q["head_confidence"].tobytes() == E.arc_confidence_arrays(marg, q["n_nodes"], pred).tobytes()
            assert q["log_partition"].tobytes() == logz.cpu().numpy().tobytes()
        for g in range(b):
            n = int(p["n_nodes"][g])
            arg = np.full((1, v, 2), -1, np.int32)
            host, _, st = E.projective_decode_arrays(scores[g][None], [n], arg, True)
            assert st[0] == 1
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
        assert m.evaluate_batch(dict(feed), on_device=True, tree="projective-mbr") == host
        tot[0] += b
        for c in range(3):
            tot[1 + c] += host[c] * b
    assert seen[0] + seen[1] == tot[0] and seen[1] > 0, seen
    plain = m.score_epoch(data)
    m.score_epoch(data, tree="projective")
    torch.cuda.synchronize()
    proj_bytes = m.decode_stats["d2h_bytes"]
    got = m.score_epoch(data, tree="projective-mbr")
    torch.cuda.synchronize()
    st = m.decode_stats
    assert st["d2h_bytes"] == proj_bytes == _batch_bytes(m, data, 6)   # the loss, [b, 5] counts and [b] status
    assert st["repaired_graphs"] == seen[1] and st["infeasible_graphs"] == 0 and st["fallback_graphs"] == 0, st
    assert got[1:4] == (tot[1] / tot[0], tot[2] / tot[0], tot[3] / tot[0]), (got, tot)
    assert got[0] == plain[0] and got[3] == plain[3] and got[5] == plain[5]
    assert m.score_epoch(data)[:4] == plain[:4]
