"""Decoding of the heads (evaluation.decode_arrays / scores_from_counts, the
host form of ggnn_heads_decode) and the model's predict / parse interface on
a CPU device.  Every comparison is exact: integer lists and float bits.

The library's forward needs a HIP device, so the CPU-device model tests swap
build_loss for a seeded numpy stand-in that writes the two heads'
probabilities where build_loss writes them; everything after the forward --
masks, decoding, lists, scores, batching order -- is the code under test."""
import numpy as np
import pytest
import torch

from ggnn_amd import evaluation as E
from ggnn_amd.batching import synthetic_treebank
from ggnn_amd.model import DenseGGNNChemModel


def _random_batch(rng, trial):
    """A batch of the kinds tests/test_evaluation.py scores, with the edge
    cases planted: ties, an all-zero probability row, a gold row with no 1, a
    gold row with two 1s, a NaN row (by trial number)."""
    b, v, e = int(rng.integers(1, 6)), int(rng.integers(2, 12)), int(rng.integers(1, 5))
    o = max(12, v)
    heads = np.zeros((b, v, o), np.float32)
    labs = np.zeros((b, v, e), np.float32)
    n = np.zeros(b, np.int32)
    for g in range(b):
        n[g] = int(rng.integers(2, v + 1))
        for node in range(1, n[g]):
            heads[g, node, rng.integers(0, n[g])] = 1
            labs[g, node, rng.integers(0, e)] = 1
    lv = [2, 5, 255][trial % 3]                      # few levels: ties everywhere
    ph = (rng.integers(0, lv + 1, heads.shape) / lv).astype(np.float32)
    pe = (rng.integers(0, lv + 1, labs.shape) / lv).astype(np.float32)
    g = int(rng.integers(0, b))
    node = int(rng.integers(1, n[g]))
    kind = trial % 7
    if kind == 1:                                    # a planted tie: an earlier and a later column
        ph[g, node, :] = 0.25
        ph[g, node, 0] = ph[g, node, n[g] - 1] = 1.0
        pe[g, node, :] = 0.5
    elif kind == 2:                                  # an all-zero probability row inside n
        ph[g, node, :] = 0
    elif kind == 3:
        pe[g, node, :] = 0
    elif kind == 4:                                  # a gold row with no 1
        heads[g, node, :] = 0
    elif kind == 5:                                  # a gold row with two 1s: the first counts
        heads[g, node, :] = 0
        heads[g, node, 0] = heads[g, node, n[g] - 1] = 1
    elif kind == 6:                                  # a NaN row
        ph[g, node, int(rng.integers(0, o))] = np.nan
    return b, v, o, e, n, heads, labs, ph, pe


def _outcome(fn):
    try:
        return fn()
    except (ZeroDivisionError, IndexError) as ex:    # the reference's list path raises for such batches
        return type(ex)


def test_decode_arrays_and_scores_match_the_host_scorer():
    rng = np.random.default_rng(11)
    seen_irregular = seen_regular = 0
    for trial in range(420):
        b, v, o, e, n, heads, labs, ph, pe = _random_batch(rng, trial)
        m, m_e = E.closed_form_masks(n, v, o, e)
        flat = lambda a: np.ascontiguousarray(a, np.float32).reshape(b, -1)
        args = (flat(heads), flat(ph), v, flat(m), flat(labs), flat(pe), flat(m_e), o, e)
        pred, gold, counts = E.decode_arrays(ph, pe, n, heads, labs)
        assert pred.dtype == gold.dtype == counts.dtype == np.int32
        assert pred.shape == gold.shape == (b, v, 2) and counts.shape == (b, 5)
        with np.errstate(invalid="ignore"):
            # (the same pred from a feed's own masks, as predict_batch takes it without closed-form masks)
            assert (E.pred_from_masks(flat(ph), flat(pe), m, m_e) == pred).all(), trial
            _, res, tgt = E.results_reshaped_btb(args[0], args[1], args[3], v, o, e)
            _, res_e, tgt_e = E.results_reshaped_btb(args[4], args[5], args[6], v, o, e, is_edge=True)
        for g in range(b):
            assert (pred[g, 0] == -1).all() and (pred[g, n[g]:] == -1).all(), trial
            rg_h, rg_e = E.lists_from_decoded(pred[g])
            tg_h, tg_e = E.lists_from_decoded(gold[g])
            assert rg_h == E.adj_mat_to_target(res[g], is_probability=True), trial
            assert rg_e == E.adj_mat_to_target(res_e[g], is_probability=True), trial
            assert tg_h == E.adj_mat_to_target(tgt[g]) and tg_e == E.adj_mat_to_target(tgt_e[g]), trial
        # without gold: the same predictions, no counts but `regular`
        pred2, gold2, counts2 = E.decode_arrays(ph, pe, n)
        assert gold2 is None and (pred2 == pred).all() and (counts2[:, :4] == 0).all()
        assert (counts2[:, 4] >= counts[:, 4]).all()
        with np.errstate(invalid="ignore"):
            ref = _outcome(lambda: E.batch_las_uas(*args))
            by_probs = _outcome(lambda: E.scores_from_counts(counts, lambda i: E.graph_scores(
                args[0][i], args[1][i], args[3][i], args[4][i], args[5][i], args[6][i], v, o, e)))
        by_lists = _outcome(lambda: E.scores_from_counts(counts, lambda i: E.graph_scores_from_lists(pred[i], gold[i])))
        assert by_probs == ref and by_lists == ref, (trial, ref, by_probs, by_lists)
        seen_irregular += int((counts[:, 4] == 0).sum())
        seen_regular += int((counts[:, 4] == 1).sum())
        if trial % 7 == 6:
            assert (counts[:, 4] == 0).any(), trial      # the NaN graph is never regular
    assert seen_irregular > 100 and seen_regular > 100


def test_decode_arrays_masked_column_loses_and_inf_is_irregular():
    b, v, o, e = 2, 4, 6, 3
    ph = np.full((b, v, o), 0.125, np.float32)
    pe = np.full((b, v, e), 0.25, np.float32)
    ph[:, 1, 1] = 0.5
    ph[:, 1, 3] = 0.75            # column 3 >= n = 3: masked, must lose to column 1
    ph[:, 2, 2] = ph[:, 2, 0] = 0.5
    pe[:, :, 2] = 0.5
    ph[1, 2, 5] = np.inf          # a masked +inf: inf * 0 = NaN on the host path
    n = np.array([3, 3], np.int32)
    pred, gold, counts = E.decode_arrays(ph, pe, n)
    assert gold is None
    assert pred[0].tolist() == [[-1, -1], [1, 2], [0, 2], [-1, -1]]
    assert pred[1].tolist() == [[-1, -1], [1, 2], [-1, 2], [-1, -1]]
    assert counts[:, 4].tolist() == [1, 0]


def test_heads_decode_rejects_bad_arguments_without_gpu(lib):
    """ggnn_heads_decode validates on the host before any launch."""
    import ctypes
    from ggnn_amd import _lib
    d = _lib.dims(2, 30, 64, 1, 1)
    P = ctypes.c_void_p
    x = P(256)                                        # never dereferenced: every call below fails validation
    ok = dict(o=150, oe=12, ph=x, pl=x, gh=None, gl=None, n=x, pred=x, gold=None, counts=x)
    for change, word in ((dict(o=0), b"1..1024"), (dict(o=1025), b"1..1024"), (dict(oe=0), b"1..1024"),
                         (dict(oe=1025), b"1..1024"), (dict(o=29), b"v 30 > o 29"), (dict(ph=None), b"NULL"),
                         (dict(pl=None), b"NULL"), (dict(n=None), b"NULL"), (dict(pred=None), b"NULL"),
                         (dict(counts=None), b"NULL"), (dict(gh=x), b"together"), (dict(gl=x), b"together")):
        a = dict(ok, **change)
        rc = lib.ggnn_heads_decode(ctypes.byref(d), a["ph"], a["o"], a["pl"], a["oe"], a["gh"], a["gl"], a["n"],
                                   a["pred"], a["gold"], a["counts"], None)
        assert rc == -1 and word in lib.ggnn_last_error(), (change, lib.ggnn_last_error())
    assert lib.ggnn_heads_decode(None, x, 150, x, 12, None, None, x, x, None, x, None) == -1
    assert "ggnn_heads_decode" in _lib.EXPORTED and _lib.DECODE_COUNTS == 5


def _abi_entries(lib):
    """{entry: call(**changes)} for the decode entry points of the C ABI at b = 2,
    v = 20, o = 150 with dummy pointers (no call here gets past validation):
    x everywhere, y where a pointer must differ from the input."""
    import ctypes
    from ggnn_amd import _lib
    x, y = ctypes.c_void_p(256), ctypes.c_void_p(512)
    tail = ("ws", "ws_bytes", "stream")
    a_pass = ("x", "o", "n", "single", "pred", "gold", "counts", "status") + tail
    marginals = ("x", "o", "n", "single", "marg", "logz", "scores", "status") + tail
    loss = ("x", "o", "gold_head", "n", "family", "single", "tn", "marg", "logz", "status", "used", "loss") + tail
    order = {"heads_decode": ("x", "o", "pl", "oe", "gh", "gl", "n", "pred", "gold", "counts", "stream"),
             "tree_decode": a_pass, "projective_decode": a_pass,
             "projective_marginals": marginals, "tree_marginals": marginals,
             "arc_confidence": ("x", "o", "n", "pred", "conf", "stream"),
             "tree_loss": loss, "tree_loss_dev": loss,
             "tree_sample": ("x", "o", "n", "single", "marg", "logz", "m_status", "num", "seed", "heads", "log_prob",
                             "status") + tail,
             "projective_sample": ("x", "o", "n", "single", "num", "seed", "heads", "log_prob", "status",
                                   "logz") + tail,
             "projective_kbest": ("x", "o", "n", "single", "K", "heads", "totals", "count", "status") + tail}
    ok = dict(dims=True, b=2, v=20, o=150, oe=12, single=1, family=0, num=3, K=3, seed=0, ws=None, ws_bytes=0,
              stream=None, gh=None, gl=None, gold=None, counts=None, marg=y)

    def entry(name):
        def call(**changes):
            a = dict(ok, **changes)
            if name.startswith("tree_loss"):        # the loss entries always take a workspace
                a = dict(dict(ok, ws=x, ws_bytes=1 << 40, tn=x if name.endswith("_dev") else 1.0), **changes)
            elif name == "heads_decode":
                a = dict(dict(ok, counts=x), **changes)
            d = _lib.dims(a["b"], a["v"], 64, 1, 1)
            args = [a.get(k, x) for k in order[name]]
            rc = getattr(lib, "ggnn_" + name)(ctypes.byref(d) if a["dims"] else None, *args)
            return rc, lib.ggnn_last_error()
        return call
    return {name: entry(name) for name in order}, x


def test_abi_reports_the_first_fault_in_the_documented_order(lib):
    """Two faults in one call: every decode entry point reports the one that
    comes first in dims, b / v, o, v > o, GGNN_TREE_MAXV, single_root, NULL, the
    entry's own checks (in its own order), workspace -- with these exact texts."""
    calls, x = _abi_entries(lib)
    together = lambda name: "%s: gold and counts must be given together (one is NULL)" % name
    alias = lambda name: "%s: marg must not alias probs_head" % name
    count = lambda name, what, top, got: "%s: %s must lie in 1..%d (got %d)" % (name, what, top, got)
    grid = lambda name, what: "%s: %s exceeds the grid" % (name, what)
    # entry -> (a required pointer, [(faults of its own checks in order, the text)], v of a short workspace)
    tree_passes = {
        "tree_decode": ("pred", [(dict(gold=x), together("tree_decode"))], None),
        "projective_decode": ("status", [(dict(counts=x), together("projective_decode"))], 129),
        "projective_marginals": ("logz", [(dict(marg=x), alias("projective_marginals"))], 108),
        "tree_marginals": ("n", [(dict(marg=x), alias("tree_marginals"))], 200),
        "tree_loss": ("used", [(dict(family=2), "tree_loss: family must be 0 (all trees) or 1 (projective)"),
                               (dict(tn=0.0), "tree_loss: target_num must be > 0"),
                               (dict(marg=x), alias("tree_loss"))], 20),
        "tree_loss_dev": ("ws", [(dict(family=-1), "tree_loss: family must be 0 (all trees) or 1 (projective)"),
                                 (dict(marg=x), alias("tree_loss"))], 20),
        "tree_sample": ("m_status", [(dict(num=0), count("tree_sample", "num_samples", 4096, 0)),
                                     (dict(marg=None), "tree_sample: single_root needs marg (NULL pointer)"),
                                     (dict(b=1 << 20, num=4096), grid("tree_sample", "b * num_samples"))], 200),
        "projective_sample": ("log_prob", [(dict(num=4097), count("projective_sample", "num_samples", 4096, 4097)),
                                           (dict(b=1 << 23, num=4096), grid("projective_sample", "b * chunks"))],
                              129),
        "projective_kbest": ("totals", [(dict(K=17), count("projective_kbest", "K", 16, 17))],
                             lib.ggnn_projective_kbest_lds_maxn(3) + 1)}
    cases = []
    for name, (ptr, own, v_short) in tree_passes.items():
        said = "tree_loss" if name == "tree_loss_dev" else name
        first, last = own[0], own[-1]
        cases += [(name, dict(dims=False, b=0), "%s: dims is NULL" % said),
                  (name, dict(b=0, o=0), "%s: b, v must be >= 1" % said),
                  (name, dict(v=0, o=1025), "%s: b, v must be >= 1" % said),
                  (name, dict(o=0), "%s: o must lie in 1..1024 (got 0)" % said),
                  (name, dict(v=257, o=256), "%s: v 257 > o 256" % said),
                  (name, {"o": 19, ptr: None}, "%s: v 20 > o 19" % said),
                  (name, dict(v=257, o=300, single=2), "%s: v 257 > GGNN_TREE_MAXV 256" % said),
                  (name, {"single": 2, ptr: None}, "%s: single_root must be 0 or 1" % said),
                  (name, dict(first[0], single=-1), "%s: single_root must be 0 or 1" % said),
                  (name, {ptr: None, **first[0]}, "%s: NULL pointer" % said)]
        cases += [(name, dict(later[0], **earlier[0]), earlier[1]) for earlier, later in zip(own, own[1:])]
        if v_short:                                  # the last own check beside a workspace that is too short
            cases.append((name, dict(last[0], v=v_short, o=256, ws=None if v_short > 20 else x, ws_bytes=0), last[1]))
    cases += [("tree_loss_dev", dict(tn=None, dims=False), "tree_loss_dev: NULL target_num"),
              ("tree_sample", dict(num=0, marg=None, b=1 << 20), count("tree_sample", "num_samples", 4096, 0)),
              ("projective_sample", dict(num=0, v=129, o=256), count("projective_sample", "num_samples", 4096, 0)),
              ("arc_confidence", dict(dims=False, v=0), "arc_confidence: dims is NULL"),
              ("arc_confidence", dict(b=0, o=0), "arc_confidence: b, v must be >= 1"),
              ("arc_confidence", dict(o=1025, v=0), "arc_confidence: b, v must be >= 1"),
              ("arc_confidence", dict(o=0), "arc_confidence: o must lie in 1..1024 (got 0)"),
              ("arc_confidence", dict(o=19, conf=None), "arc_confidence: v 20 > o 19"),
              ("arc_confidence", dict(v=257, o=300, pred=None), "arc_confidence: NULL pointer"),
              ("heads_decode", dict(dims=False, o=0), "heads_decode: dims is NULL"),
              ("heads_decode", dict(b=0, oe=0), "heads_decode: b, v must be >= 1"),
              ("heads_decode", dict(o=0), "heads_decode: o and oe must lie in 1..1024 (got 0, 12)"),
              ("heads_decode", dict(oe=1025, o=19), "heads_decode: o and oe must lie in 1..1024 (got 19, 1025)"),
              ("heads_decode", dict(o=19, pl=None), "heads_decode: v 20 > o 19"),
              ("heads_decode", dict(v=257, o=300, counts=None, gh=x), "heads_decode: NULL pointer"),
              ("heads_decode", dict(gl=x),
               "heads_decode: gold_head and gold_label must be given together (one is NULL)")]
    # a short workspace alone: the last report, with the size the entry's own query gives
    for name, size, v in (("projective_decode", lib.ggnn_projective_decode_workspace_bytes(2, 129), 129),
                          ("projective_marginals", lib.ggnn_projective_marginals_workspace_bytes(2, 108), 108),
                          ("tree_marginals", lib.ggnn_tree_marginals_workspace_bytes(2, 200), 200),
                          ("tree_sample", lib.ggnn_tree_sample_workspace_bytes(2, 200, 3), 200),
                          ("projective_sample", lib.ggnn_projective_sample_workspace_bytes(2, 129, 3), 129)):
        assert size > 0
        cases.append((name, dict(v=v, o=256), "%s: workspace of 0 bytes, %d needed" % (name, size)))
        cases.append((name, dict(v=v, o=256, ws=x, ws_bytes=size - 1),
                      "%s: workspace of %d bytes, %d needed" % (name, size - 1, size)))
    cases.append(("tree_loss", dict(ws_bytes=255), "tree_loss: workspace of 255 bytes, 256 needed"))
    assert len(cases) > 120 and {name for name, _, _ in cases} == set(calls)
    for name, changes, text in cases:
        rc, said = calls[name](**changes)
        assert rc == -1 and said == text.encode(), (name, changes, said)


def test_real_dev_gold_lists_are_regular():
    """The first 40 dev sentences (tests/test_gpu_decode.py scores them on the
    device): every real node has a gold head and label, so with non-zero
    probability rows no graph needs the host fallback."""
    from ggnn_amd.batching import TRAIN_WITH_DEV, wsj_model_sizes
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20}, device="cpu", seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False, restrict=40)
    o, oe = m.params["output_size"], m.output_size_edges
    graphs = 0
    for feed in m.make_minibatch_iterator(data, False):
        b, v = feed["num_graphs"], feed["num_vertices"]
        n = m._feed_n_nodes(feed)
        assert n is not None
        y = np.asarray(feed["target_values_head"], np.float32).reshape(b, v, o)
        y_e = np.asarray(feed["target_values_edges"], np.float32).reshape(b, v, oe)
        _, gold, counts = E.decode_arrays(np.full((b, v, o), 0.5, np.float32), np.full((b, v, oe), 0.5, np.float32),
                                          n, y, y_e)
        assert (counts[:, 4] == 1).all() and (counts[:, 0] == n - 1).all()
        # the host scorer's own flags agree: the vectorised path, no list fallback
        kt, _ = E._first_max(y[:, 1:, :], False)
        kte, _ = E._first_max(y_e[:, 1:, :], False)
        real = np.arange(1, v)[None, :] < n[:, None]
        assert (kt == real).all() and (kte == real).all()
        graphs += b
    assert graphs == 40


# ------------------------------------------------------------- the CPU model
def _cpu_model(seed, batch_size=2):
    return DenseGGNNChemModel(params={"hidden_size": 64, "num_timesteps": 2, "batch_size": batch_size},
                              num_edge_types=3, device="cpu", seed=seed, precision="fp32", vocab_size=50,
                              embedding_sizes=dict(loc=16, pos=8, word=24, edge=16))


def _stub_forward(m, decimals):
    """build_loss's outputs from a numpy stand-in seeded by the staged batch's
    word_inputs (so a batch gets the same probabilities whoever stages it)."""
    def build_loss(task_id=0):
        ph = m.placeholders
        b, v = int(ph["num_graphs"]), int(ph["num_vertices"])
        o, oe = m.params["output_size"], m.output_size_edges
        wi = np.asarray(ph["word_inputs"]).astype(np.int64)
        rng = np.random.default_rng(int((wi * np.arange(1, wi.size + 1).reshape(wi.shape)).sum()) % (2 ** 31))
        cv = np.round(rng.random((b, v * o)) * 0.98 + 0.01, decimals).astype(np.float32)
        cv_e = np.round(rng.random((b, v * oe)) * 0.98 + 0.01, decimals).astype(np.float32)
        m.ops["computed_values"] = torch.from_numpy(cv)
        m.ops["computed_values_edges"] = torch.from_numpy(cv_e)
        m.ops["loss"] = torch.tensor(float(cv.sum() + cv_e.sum()) / (b * v))
        return m.ops["loss"]
    m.build_loss = build_loss
    return m


def _raw(n_sentences=14, seed=3):
    raw = synthetic_treebank(n_sentences, num_edge_types=3, output_size_edges=12, pos_size=46, vocab_size=50,
                             max_nodes=30, seed=seed)
    empty = dict(raw[0], graph=[], targets=[], node_features=[0], node_features_target=[0], words_index=[0], id="e")
    return raw[:5] + [empty] + raw[5:]


def _host_lists(m, data):
    """{sentence id: [[head, label], ...]} from run_epoch's returned
    probabilities through adj_mat_to_target + merge_head_and_edge_graph."""
    out = m.run_epoch("valid", data, False)
    cvs, nvs, masks, ids, cvs_e, masks_e = out[8], out[9], out[10], out[11], out[14], out[15]
    o, oe = m.params["output_size"], m.output_size_edges
    lists = {}
    for cv, v, mask, sid, cv_e, mask_e in zip(cvs, nvs, masks, ids, cvs_e, masks_e):
        _, res, _ = E.results_reshaped_btb(np.zeros_like(cv), cv, mask, v, o, oe)
        _, res_e, _ = E.results_reshaped_btb(np.zeros_like(cv_e), cv_e, mask_e, v, o, oe, is_edge=True)
        for g, s in enumerate(sid):
            lists[s] = E.merge_head_and_edge_graph(E.adj_mat_to_target(res[g], is_probability=True),
                                                   E.adj_mat_to_target(res_e[g], is_probability=True))
    return lists


def test_parse_equals_the_host_lists_in_input_order():
    m = _stub_forward(_cpu_model(0), decimals=1)      # one decimal: ties in every row
    raw = _raw()
    data = m.process_raw_graphs(raw, False)
    assert len(data[0]) >= 3                          # the input spans at least 3 buckets
    ref = _host_lists(m, data)
    no_targets = [{k: x for k, x in d.items() if k != "targets"} for d in raw]
    got = m.parse(no_targets)
    assert all("targets" not in d for d in no_targets)           # the input dicts are not touched
    assert len(got) == len(raw)
    for d, entry in zip(raw, got):
        if len(d["graph"]) == 0:
            assert entry == []
        else:
            assert entry == ref[d["id"]], d["id"]
            assert len(entry) == len(d["node_features"]) - 1
            assert all(0 <= h < len(d["node_features"]) and 1 <= lab <= m.output_size_edges for h, lab in entry)
    # bucket order differs from input order here, so input order is not an accident
    bucket_order = [el["id"] for bucket in data[0].values() for el in bucket]
    assert bucket_order != [d["id"] for d in raw if len(d["graph"])]


def test_predict_batch_arrays():
    m = _stub_forward(_cpu_model(0), decimals=1)
    data = m.process_raw_graphs(_raw(), False)
    ref = _host_lists(m, data)
    for feed in m.make_minibatch_iterator(data, False):
        p = m.predict_batch(feed)
        b, v = feed["num_graphs"], feed["num_vertices"]
        assert p["heads"].shape == p["labels"].shape == (b, v) and p["heads"].dtype == np.int32
        n = np.asarray(feed["node_mask_edges"]).reshape(b, -1).sum(axis=1) / m.output_size_edges
        assert p["n_nodes"].tolist() == n.tolist() and list(p["sentences_id"]) == list(feed["sentences_id"])
        for g, s in enumerate(feed["sentences_id"]):
            k = int(n[g])
            assert (p["heads"][g, k:] == -1).all() and p["heads"][g, 0] == -1 and p["labels"][g, 0] == -1
            assert [[int(h), int(lab) + 1] for h, lab in zip(p["heads"][g, 1:k], p["labels"][g, 1:k])] == ref[s]


def test_parse_fed_back_as_targets_scores_one():
    m = _stub_forward(_cpu_model(1), decimals=6)
    raw = [d for d in _raw() if len(d["graph"])]
    parsed = m.parse(raw)
    again = [dict(d, targets=t) for d, t in zip(raw, parsed)]
    data = m.process_raw_graphs(again, False)
    feeds = list(m.make_minibatch_iterator(data, False))
    assert len(feeds) >= 3
    for feed in feeds:
        assert m.evaluate_batch(feed) == (1.0, 1.0, 1.0)
        assert m.evaluate_batch(feed, on_device=True) == (1.0, 1.0, 1.0)


def test_evaluate_batch_on_device_equals_the_host_scorer():
    m = _stub_forward(_cpu_model(2), decimals=1)
    data = m.process_raw_graphs(_raw(20, seed=5), False)
    seen = set()
    for feed in m.make_minibatch_iterator(data, False):
        host = m.evaluate_batch(feed)
        assert m.evaluate_batch(feed, on_device=True) == host
        seen.add(host)
    assert len(seen) > 3
    # a feed whose masks are not get_mask's closed form takes the host scorer
    feed = dict(feed)
    mask = np.array(feed["node_mask"], dtype=np.float64)
    mask.reshape(feed["num_graphs"], feed["num_vertices"], -1)[0, 1, 0] = 0.0
    feed["node_mask"] = mask
    assert m._feed_n_nodes(feed) is None
    assert m.evaluate_batch(feed, on_device=True) == m.evaluate_batch(feed)
    # ... and predict_batch decodes on the host with the feed's own masks
    p = m.predict_batch(feed)
    b, v, o, oe = feed["num_graphs"], feed["num_vertices"], m.params["output_size"], m.output_size_edges
    cv, cv_e = m.ops["computed_values"].numpy(), m.ops["computed_values_edges"].numpy()
    _, res, _ = E.results_reshaped_btb(np.zeros_like(cv), cv, mask.reshape(b, -1), v, o, oe)
    _, res_e, _ = E.results_reshaped_btb(np.zeros_like(cv_e), cv_e, np.reshape(feed["node_mask_edges"], (b, -1)),
                                         v, o, oe, is_edge=True)
    for g in range(b):
        assert E.lists_from_decoded(np.stack([p["heads"][g], p["labels"][g]], axis=1)) == (
            E.adj_mat_to_target(res[g], is_probability=True), E.adj_mat_to_target(res_e[g], is_probability=True))


def test_score_epoch_equals_run_epoch_on_a_cpu_device():
    m = _stub_forward(_cpu_model(3), decimals=1)
    data = m.process_raw_graphs(_raw(20, seed=7), False)
    ref = m.run_epoch("valid", data, False)
    got = m.score_epoch(data)
    assert got[:4] == (ref[0], ref[5], ref[6], ref[16]) and got[5] == ref[4]
    assert m.decode_stats["graphs"] == 20
    # the shared epoch loop's progress line changes no value
    loud = m.run_epoch("valid", data, False, verbose=True)
    assert (loud[0], loud[4], loud[5], loud[6], loud[16]) == (ref[0], ref[4], ref[5], ref[6], ref[16])


def test_predict_batch_without_closed_form_masks_attempts_nothing():
    """A feed whose masks the decode cannot rebuild: heads / labels come from
    the feed's own masks and every structured key holds its "not attempted"
    value, in the shapes and dtypes of a decoded batch."""
    m = _stub_forward(_cpu_model(4), decimals=2)
    feed = dict(next(iter(m.make_minibatch_iterator(m.process_raw_graphs(_raw(), False), False))))
    b, v, o, oe = feed["num_graphs"], feed["num_vertices"], m.params["output_size"], m.output_size_edges
    assert b == 2
    mask = np.array(feed["node_mask"], dtype=np.float64)
    mask.reshape(-1)[0] = 0.5                         # not get_mask's closed form: no node counts
    feed["node_mask"] = mask
    assert m._feed_n_nodes(feed) is None
    p = m.predict_batch(feed, tree="projective", confidence=True, samples=3, kbest=2)
    assert list(p) == ["heads", "labels", "n_nodes", "sentences_id", "tree_status", "head_confidence",
                       "log_partition", "sampled_heads", "sample_log_prob", "sample_status", "kbest_heads",
                       "kbest_count", "kbest_status", "kbest_log_prob"]
    pred = E.pred_from_masks(m.ops["computed_values"].numpy(), m.ops["computed_values_edges"].numpy(),
                             mask.astype(np.float32).reshape(b, v, o),
                             np.asarray(feed["node_mask_edges"], np.float32).reshape(b, v, oe))
    n = np.asarray(feed["node_mask_edges"]).reshape(b, -1).sum(axis=1) / oe
    want = {"heads": (pred[:, :, 0], np.int32), "labels": (pred[:, :, 1], np.int32), "n_nodes": (n, np.int32),
            "tree_status": (np.full(b, 2), np.int32),
            "head_confidence": (np.zeros((b, v)), np.float32), "log_partition": (np.full(b, np.nan), np.float32),
            "sampled_heads": (np.full((b, 3, v), -1), np.int32),
            "sample_log_prob": (np.full((b, 3), -np.inf), np.float32), "sample_status": (np.full((b, 3), 2), np.int32),
            "kbest_heads": (np.full((b, 2, v), -1), np.int32), "kbest_count": (np.zeros(b), np.int32),
            "kbest_status": (np.full(b, 2), np.int32), "kbest_log_prob": (np.full((b, 2), -np.inf), np.float32)}
    for key, (value, dtype) in want.items():
        assert isinstance(p[key], np.ndarray) and p[key].dtype == dtype and p[key].shape == value.shape, key
        assert np.array_equal(p[key], value, equal_nan=True), key
    assert list(p["sentences_id"]) == list(feed["sentences_id"])
    assert (p["heads"][:, 1:] >= 0).any()
    for kw, text in ((dict(samples=E.SAMPLE_MAX + 1), "samples must lie in 0..4096 (got 4097)"),
                     (dict(samples=-1), "samples must lie in 0..4096 (got -1)"),
                     (dict(kbest=E.KBEST_MAX + 1), "kbest must lie in 0..16 (got 17)"),
                     (dict(kbest=-1), "kbest must lie in 0..16 (got -1)")):
        with pytest.raises(ValueError) as err:
            m.predict_batch(feed, **kw)
        assert str(err.value) == text


def test_raw_sentence_drivers_equal_predict_batch_per_batch():
    """parse, parse_kbest and sample_trees are predict_batch over the batches
    of the raw sentences: the lists land at the input positions, and batch i
    of sample_trees draws with seed (seed + i) mod 2^64."""
    m = _stub_forward(_cpu_model(5), decimals=2)
    raw = _raw()
    feeds = list(m.make_minibatch_iterator(m.process_raw_graphs([dict(d, id=i) for i, d in enumerate(raw)], False),
                                           False))
    assert len(feeds) >= 5
    assert [s for f in feeds for s in f["sentences_id"]] != sorted(s for f in feeds for s in f["sentences_id"])

    def expected(rows, **kw):
        """[per input sentence: what rows(p, g, n) lists] over predict_batch(feed, **kw(i)) of batch i."""
        out = [[] for _ in raw]
        for i, feed in enumerate(feeds):
            p = m.predict_batch(feed, **{k: x(i) if callable(x) else x for k, x in kw.items()})
            for g, s in enumerate(p["sentences_id"]):
                out[s] = rows(p, g, int(p["n_nodes"][g]))
        return out

    pairs = lambda heads, p, g, n: [[int(h), int(lab) + 1] for h, lab in zip(heads[1:n], p["labels"][g, 1:n])]
    assert m.parse(raw) == expected(lambda p, g, n: pairs(p["heads"][g], p, g, n))
    trees, conf = m.parse(raw, tree="projective", confidence=True)
    assert trees == expected(lambda p, g, n: pairs(p["heads"][g], p, g, n), tree="projective")
    assert conf == expected(lambda p, g, n: [float(c) for c in p["head_confidence"][g, 1:n]], tree="projective",
                            confidence=True)
    ranks = lambda p, g: range(int(p["kbest_count"][g]))
    trees, log_probs = m.parse_kbest(raw, 2)
    assert trees == expected(lambda p, g, n: [pairs(p["kbest_heads"][g, r], p, g, n) for r in ranks(p, g)], kbest=2)
    assert log_probs == expected(lambda p, g, n: [float(p["kbest_log_prob"][g, r]) for r in ranks(p, g)], kbest=2)
    assert max(map(len, trees)) == 2 and trees[5] == [] == log_probs[5]          # (the empty sentence)
    drawn = lambda p, g: np.nonzero(p["sample_status"][g] == 1)[0]
    for family in ("nonprojective", "projective"):
        for seed in (5, 2 ** 64 - 2):                # (the second: batches 2.. wrap round to seeds 0..)
            kw = dict(samples=2, sample_family=family, sample_seed=lambda i: (seed + i) % 2 ** 64)
            trees, log_probs = m.sample_trees(raw, 2, seed=seed, family=family)
            assert trees == expected(lambda p, g, n: [pairs(p["sampled_heads"][g, s], p, g, n) for s in drawn(p, g)],
                                     **kw), (family, seed)
            assert log_probs == expected(lambda p, g, n: [float(p["sample_log_prob"][g, s]) for s in drawn(p, g)],
                                         **kw), (family, seed)
            assert sum(map(len, trees)) == 2 * (len(raw) - 1)
    assert m.sample_trees(raw, 2, seed=5)[0] != m.sample_trees(raw, 2, seed=6)[0]


def test_host_decoder_and_output_heads_take_the_same_arguments():
    """decode_chain calls its two backends alike: the five methods of the host
    adapter and of the device binding agree on the names, order, kinds and
    defaults of the parameters the chain passes."""
    import inspect
    from ggnn_amd.decoding import HostDecoder
    from ggnn_amd.heads import OutputHeads
    a_pass = ("scores", "n_nodes", "pred", "gold", "counts", "single_root")
    used = {"decode": ("probs", "n_nodes", "labels"), "tree_decode": a_pass, "projective_decode": a_pass,
            "projective_marginals": ("probs_head", "n_nodes", "single_root", "with_scores"),
            "arc_confidence": ("marg", "n_nodes", "pred")}
    for name, params in used.items():
        dev = inspect.signature(getattr(OutputHeads, name)).parameters
        host = inspect.signature(getattr(HostDecoder, name)).parameters
        want = ["self"] + list(params)
        assert list(dev)[:len(want)] == want and list(host)[:len(want)] == want, name
        for p in params:
            assert (dev[p].kind, dev[p].default) == (host[p].kind, host[p].default), (name, p)
        for sig in (dev, host):                                           # (a workspace): never required
            assert all(sig[p].default is not inspect.Parameter.empty for p in list(sig)[len(want):]), name
