"""ggnn_heads_decode on the GPU: the kernel against its host form
(evaluation.decode_arrays) and the reference's lists (adj_mat_to_target), and
the model's predict_batch / parse / evaluate_batch(on_device=True) /
score_epoch against the host scorer.  Exact integer and bit equality only."""
import numpy as np
import pytest

from decode_cases import _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4, 150, 12),      # the smallest bucket
          (2, 64, 64, 1),       # exact wave width, a single label column
          (2, 130, 150, 65),    # partial third / second lane chunk
          (2, 6, 1024, 46),     # the widest head
          (2, 38, 150, 46)]


def _n_vectors(b, v):
    """Three launches per shape: together every graph count of 2, an interior
    value and v occurs; the third launch carries the NaN / +inf graphs (its
    graph 1 has n < v <= o, so a masked column exists)."""
    mid = max(2, min(v - 1, v // 2 + 1))
    return [([2, mid, v][:b], False), ([v, mid, 2][:b], False), ([v, mid, v][:b], True)]


def _case(b, v, o, oe, n, nonfinite, seed):
    rng = np.random.default_rng(seed)
    heads = np.zeros((b, v, o), np.float32)
    labs = np.zeros((b, v, oe), np.float32)
    ph = (rng.integers(0, 9, heads.shape) / 8).astype(np.float32)      # 9 levels: ties in most rows
    pe = (rng.integers(0, 9, labs.shape) / 8).astype(np.float32)
    # (padding rows hold values too: the mask, not the data, must drop them)
    expect = []                                      # (graph, node, predicted head) of the planted rows
    for g in range(b):
        k = n[g]
        for node in range(1, k):
            heads[g, node, rng.integers(0, k)] = 1
            labs[g, node, rng.integers(0, oe)] = 1
        # row 1: a tie between an earlier and a later column; a larger value in
        # the first masked column must lose
        ph[g, 1, :] = 0.25
        ph[g, 1, 0] = ph[g, 1, k - 1] = 0.75
        if k < o:
            ph[g, 1, k] = 0.875
        pe[g, 1, :] = 0.125
        pe[g, 1, 0] = pe[g, 1, oe - 1] = 0.5
        expect.append((g, 1, 0))
        if k >= 3:                                   # an all-zero row inside n
            ph[g, 2, :k] = 0
            expect.append((g, 2, -1))
        if k >= 4:                                   # a gold row without a 1
            heads[g, 3, :] = 0
    if nonfinite:
        ph[0, 1, 0] = np.nan
        ph[1, 1, n[1]] = np.inf
        expect = [x for x in expect if x[:2] not in ((0, 1), (1, 1))]
    return heads, labs, ph, pe, expect


_REFERENCE = {}


def _reference(shape, k):
    """One launch's inputs and host results, computed once and left unchanged."""
    if (shape, k) not in _REFERENCE:
        b, v, o, oe = shape
        n, nonfinite = _n_vectors(b, v)[k]
        heads, labs, ph, pe, expect = _case(b, v, o, oe, n, nonfinite, seed=1000 * k + v)
        host = E.decode_arrays(ph, pe, np.asarray(n, np.int32), heads, labs)
        for a in (heads, labs, ph, pe) + host:
            a.setflags(write=False)
        _REFERENCE[(shape, k)] = (n, nonfinite, heads, labs, ph, pe, expect, host)
    return _REFERENCE[(shape, k)]


def _launch(torch, ph, pe, n, heads=None, labs=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    labels = None if heads is None else [t(heads), t(labs)]
    out = OutputHeads(64).decode([t(ph), t(pe)], t(np.asarray(n, np.int32)), labels)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(x) for x in s))
def test_kernel_equals_host_decode_and_reference_lists(shape, k):
    torch = _torch()
    b, v, o, oe = shape
    n, nonfinite, heads, labs, ph, pe, expect, (h_pred, h_gold, h_counts) = _reference(shape, k)
    pred, gold, counts = _launch(torch, ph, pe, n, heads, labs)
    assert pred.dtype == gold.dtype == counts.dtype == torch.int32
    pred, gold, counts = pred.cpu().numpy(), gold.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(pred, h_pred), np.argwhere(pred != h_pred)[:5]
    assert np.array_equal(gold, h_gold), np.argwhere(gold != h_gold)[:5]
    assert np.array_equal(counts, h_counts), (counts, h_counts)
    # the reference's lists per graph, from the closed-form masks
    m, m_e = E.closed_form_masks(n, v, o, oe)
    flat = lambda a: np.ascontiguousarray(a, np.float32).reshape(b, -1)
    with np.errstate(invalid="ignore"):
        _, res, tgt = E.results_reshaped_btb(flat(heads), flat(ph), flat(m), v, o, oe)
        _, res_e, tgt_e = E.results_reshaped_btb(flat(labs), flat(pe), flat(m_e), v, o, oe, is_edge=True)
    for g in range(b):
        assert (pred[g, 0] == -1).all() and (pred[g, n[g]:] == -1).all() and (gold[g, 0] == -1).all()
        rg_h, rg_e = E.lists_from_decoded(pred[g])
        tg_h, tg_e = E.lists_from_decoded(gold[g])
        assert rg_h == E.adj_mat_to_target(res[g], is_probability=True)
        assert rg_e == E.adj_mat_to_target(res_e[g], is_probability=True)
        assert tg_h == E.adj_mat_to_target(tgt[g]) and tg_e == E.adj_mat_to_target(tgt_e[g])
        if n[g] >= 4:
            assert gold[g, 3, 0] == -1 and gold[g, 3, 1] >= 0       # the gold row without a 1
    for g, node, head in expect:
        assert pred[g, node, 0] == head, (g, node, pred[g, node], head)
    for g in range(b):
        if not (nonfinite and g < 2):
            assert pred[g, 1, 1] == 0                                # the label tie: the earlier column
        if n[g] >= 3 or (nonfinite and g < 2):
            assert counts[g, 4] == 0                                 # a zero row / NaN / masked +inf
    if k == 0 and b >= 2:
        assert counts[0, 4] == 1 and counts[0, 0] == 1               # n = 2: one node, regular
    # without gold: the same predictions, no gold tensor, counts 0 but `regular`
    pred2, gold2, counts2 = _launch(torch, ph, pe, n)
    assert gold2 is None and np.array_equal(pred2.cpu().numpy(), pred)
    h2 = E.decode_arrays(ph, pe, np.asarray(n, np.int32))
    assert np.array_equal(counts2.cpu().numpy(), h2[2]) and (h2[2][:, :4] == 0).all()


def test_two_launches_give_identical_bytes():
    torch = _torch()
    shape = SHAPES[2]
    n, _, heads, labs, ph, pe, _, _ = _reference(shape, 2)
    a = _launch(torch, ph, pe, n, heads, labs)
    b = _launch(torch, ph, pe, n, heads, labs)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ------------------------------------------------------------------ the model
def _host_lists_of_staged_batch(m, feed):
    """[[head, label], ...] per graph from the probabilities the model holds
    for the batch it just ran, through the reference's functions."""
    b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
    o, oe = m.params["output_size"], m.output_size_edges
    cv = m.ops["computed_values"].cpu().numpy()
    cv_e = m.ops["computed_values_edges"].cpu().numpy()
    mask = np.asarray(feed["node_mask"], np.float32).reshape(b, v * o)
    mask_e = np.asarray(feed["node_mask_edges"], np.float32).reshape(b, v * oe)
    _, res, _ = E.results_reshaped_btb(np.zeros_like(cv), cv, mask, v, o, oe)
    _, res_e, _ = E.results_reshaped_btb(np.zeros_like(cv_e), cv_e, mask_e, v, o, oe, is_edge=True)
    return [E.merge_head_and_edge_graph(E.adj_mat_to_target(res[g], is_probability=True),
                                        E.adj_mat_to_target(res_e[g], is_probability=True)) for g in range(b)]


def test_predict_batch_and_parse_equal_the_host_lists():
    _torch()
    m = _synthetic_model(True)
    raw = _synthetic_raw()
    data = m.process_raw_graphs(raw, False)
    assert len(data[0]) >= 3
    ref = {}
    for feed in m.make_minibatch_iterator(data, False):
        p = m.predict_batch(feed)
        lists = _host_lists_of_staged_batch(m, feed)
        b = int(feed["num_graphs"])
        assert p["heads"].shape == (b, int(feed["num_vertices"])) and p["heads"].dtype == np.int32
        for g, s in enumerate(feed["sentences_id"]):
            k = int(p["n_nodes"][g])
            got = [[int(h), int(lab) + 1] for h, lab in zip(p["heads"][g, 1:k], p["labels"][g, 1:k])]
            assert got == lists[g] and len(got) == k - 1
            assert (p["heads"][g, k:] == -1).all() and (p["labels"][g, k:] == -1).all()
            ref[s] = lists[g]
    parsed = m.parse([{k: x for k, x in d.items() if k != "targets"} for d in raw])
    assert parsed == [ref[d["id"]] for d in raw]


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_evaluate_batch_on_device_equals_host(graphs):
    _torch()
    m = _synthetic_model(graphs)
    data = m.process_raw_graphs(_synthetic_raw(), False)
    by_shape = {}
    for feed in m.make_minibatch_iterator(data, False):
        by_shape.setdefault((feed["num_graphs"], feed["num_vertices"]), feed)
    feeds = list(by_shape.values())[:3]
    assert len(feeds) == 3
    for feed in feeds:
        host = m.evaluate_batch(dict(feed))
        # three runs of a shape: eager, capture + replay, replay
        for _ in range(3):
            assert m.evaluate_batch(dict(feed), on_device=True) == host
    st = m.graph_stats
    if graphs:
        assert st["replayed"] >= 6 and st["captured"] >= 3, st
    else:
        assert st["replayed"] == 0 and st["captured"] == 0, st


def test_score_epoch_equals_run_epoch_on_real_dev_sentences():
    """The first 40 sentences of the dev set at batch 20: score_epoch returns
    run_epoch's loss and scores with no graph on the host fallback (every
    real node of these sentences has a gold head and label and a non-zero
    probability row: tests/test_decode.py checks the gold side on the CPU)."""
    torch = _torch()
    from ggnn_amd.batching import TRAIN_WITH_DEV, wsj_model_sizes
    from ggnn_amd.model import DenseGGNNChemModel
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20,
                                   "compact_adjacency": True}, seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False, restrict=40)
    ref = m.run_epoch("valid", data, False)
    # the reference path alone: every graph regular under the host scorer's flags
    o, oe = m.params["output_size"], m.output_size_edges
    for labels, cv, v, labels_e, cv_e in zip(ref[7], ref[8], ref[9], ref[13], ref[14]):
        b = cv.shape[0]
        n = np.asarray(labels_e).reshape(b, v, oe).sum(axis=(1, 2)).astype(np.int32) + 1
        _, _, counts = E.decode_arrays(cv.reshape(b, v, o), cv_e.reshape(b, v, oe), n,
                                       np.asarray(labels, np.float32).reshape(b, v, o),
                                       np.asarray(labels_e, np.float32).reshape(b, v, oe))
        assert (counts[:, 4] == 1).all() and (counts[:, 0] > 0).all()
    got = m.score_epoch(data)
    torch.cuda.synchronize()
    assert got[:4] == (ref[0], ref[5], ref[6], ref[16]), (got, ref[0], ref[5], ref[6], ref[16])
    assert got[5] == ref[4]
    st = m.decode_stats
    assert st["graphs"] == 40 and st["fallback_graphs"] == 0, st
    # fetched: the loss and [b, 5] counts per batch
    assert st["d2h_bytes"] == sum(4 + 4 * 5 * cv.shape[0] for cv in ref[8])


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
def test_decode_chain_on_the_device_equals_the_host_adapter(graphs):
    """The one chain (decoding.decode_chain) with the device binding as its
    backend, as _decode_forward runs it, against the same chain with the host
    adapter on the probabilities fetched from the same forward: pred, gold,
    counts and tree_status element for element, for every tree mode whose
    kernels are bit-exact against their host forms."""
    _torch()
    from ggnn_amd.decoding import HostDecoder, decode_chain
    m = _synthetic_model(graphs)
    data = m.process_raw_graphs(_synthetic_raw(), False)
    o, oe = m.params["output_size"], m.output_size_edges
    repaired = {False: 0, True: 0, "projective": 0}
    for feed in m.make_minibatch_iterator(data, False):
        for tree in repaired:
            r = m._decode_forward(dict(feed), True, tree)
            b, v, ph = r["b"], r["v"], r["ph"]
            fetch = lambda key, w: m.ops[key].detach().reshape(b, v, w).cpu().numpy()
            labels = [np.asarray(ph[key], np.float32).reshape(b, v, w)
                      for key, w in (("target_values_head", o), ("target_values_edges", oe))]
            host = decode_chain(HostDecoder(), fetch("computed_values", o), fetch("computed_values_edges", oe),
                                r["n_nodes"], labels, tree)
            assert (r["tree_status"] is None) == (host["tree_status"] is None) == (tree is False)
            for key in ("pred", "gold", "counts") + (("tree_status",) if tree else ()):
                got = r[key].cpu().numpy()
                assert got.dtype == host[key].dtype == np.int32 and np.array_equal(got, host[key]), (tree, key)
            if tree:
                repaired[tree] += int((host["tree_status"] == 1).sum())
    assert repaired[True] > 0 and repaired["projective"] > 0, repaired        # the passes had work to do
