"""Host LAS/UAS evaluation of the btb task.

The reference scores each evaluated batch on the host from the heads'
probabilities (``humanize_batch_results_btb``, chem_tensorflow_dense.py:1160-1215):

* ``get_results_reshaped`` (btb branch, :1054-1079) masks the head / label
  probabilities and reshapes them to [b, 1, v, o] and [b, e, v, 1];
* ``adj_mat_to_target`` (:106-131) turns a target 0/1 tensor, or a probability
  tensor (``is_probability=True``: the arg-max), into a list of
  ``[source, edge_type]`` per receiving node 1..v-1;
* ``merge_head_and_edge_graph`` (:1279-1280) joins the head list with the label
  list; ``get_las_uas`` (:1304-1319) counts exact matches (LAS) and matching
  heads (UAS, or labels with ``is_edge``).

Pure numpy; no part of the GPU path.  Pinned by the reference's own test vectors
(``tests_chem.py:9-27, 50-88``) in ``tests/test_evaluation.py``.
"""
from __future__ import annotations

import numpy as np


def adj_mat_to_target(adj_mat, is_probability=False, true_target=None):
    """[e, v, o] -> [[source, edge_type], ...] for receiving nodes 1..v-1
    (chem_tensorflow_dense.py:106-131).  A node whose slice is all zero, or
    (0/1 input) holds no exact 1, is skipped.  The first maximum in (edge type,
    source) row-major order wins, as ``np.where(...)[..][0]`` does there.
    ``true_target`` is accepted for signature parity (only used by a disabled
    diagnostic in the reference).  Vectorised over the nodes (the per-node loop
    took half of run_epoch's host time at batch 20)."""
    a = np.asarray(adj_mat)
    num_e, num_v, num_o = a.shape
    if num_v < 2:
        return []
    # row n-1 = node n's [e, o] slice flattened in (edge type, source) order
    t = np.transpose(a[:, 1:, :], (1, 0, 2)).reshape(num_v - 1, num_e * num_o)
    mx = t.max(axis=1)
    eq = t == (mx[:, None] if is_probability else 1)
    keep = (mx != 0) & eq.any(axis=1)  # (a NaN maximum matches nothing: skipped)
    first = eq.argmax(axis=1)
    e, src = np.divmod(first[keep], num_o)
    return [[int(x), int(y) + 1] for x, y in zip(src, e)]


def get_las_uas(target_graph, result_graph, is_edge=False):
    """Labelled / unlabelled attachment score of one sentence
    (chem_tensorflow_dense.py:1304-1319).  Edges are [head, label]; UAS compares
    the head (index 0), or the label (index 1) when ``is_edge``.  Divides by the
    number of predicted edges, as the reference does."""
    idx = 1 if is_edge else 0
    las = uas = 0
    for i, r in enumerate(result_graph):
        t = target_graph[i]
        if t == r:
            las += 1
            uas += 1
        elif t[idx] == r[idx]:
            uas += 1
    n = len(result_graph)
    return las / n, uas / n


def merge_head_and_edge_graph(result_graph_l, result_graph_e):
    """[[head, _]] + [[_, label]] -> [[head, label]] (chem_tensorflow_dense.py:1279-1280)."""
    return [[x[0], y[1]] for x, y in zip(result_graph_l, result_graph_e)]


def results_reshaped_btb(targets, computed_values, mask, num_vertices, output_size, output_size_edges,
                         is_edge=False):
    """btb branch of ``get_results_reshaped`` (chem_tensorflow_dense.py:1054-1079):
    returns (mask, results, targets) as [b, 1, v, o] (heads) or [b, e, v, 1]
    (labels, ``is_edge``)."""
    v, e, o = int(num_vertices), int(output_size_edges), int(output_size)
    cv, m, t = np.asarray(computed_values), np.asarray(mask), np.asarray(targets)
    if is_edge:
        res = np.transpose(np.reshape(cv * m, [-1, v, e, 1]), [0, 2, 1, 3])
        tgt = np.transpose(np.reshape(t, [-1, v, e, 1]), [0, 2, 1, 3])
        msk = np.transpose(np.reshape(m, [-1, v, e, 1]), [0, 2, 1, 3])
        return msk, res, tgt
    return np.reshape(m, [-1, 1, v, o]), np.reshape(cv * m, [-1, 1, v, o]), np.reshape(t, [-1, 1, v, o])


def _first_max(t, is_probability):
    """adj_mat_to_target's choice for a batch: t [b, n, K] (node rows 1..v-1,
    (edge type, source) flattened).  Returns (keep [b, n] bool, first [b, n])."""
    mx = t.max(axis=2)
    eq = t == (mx[..., None] if is_probability else 1)
    return (mx != 0) & eq.any(axis=2), eq.argmax(axis=2)


def batch_las_uas(labels, computed_values, num_vertices, mask, labels_e, computed_values_e, mask_edges,
                  output_size, output_size_edges):
    """Mean (LAS, UAS, label accuracy) over a batch, as
    ``humanize_batch_results_btb`` computes them (chem_tensorflow_dense.py:1160-1215,
    without its file output): heads from the arg-max of the head
    probabilities, labels from the arg-max of the label probabilities.

    Vectorised over the batch: every graph whose four node lists (target and
    result heads and labels) keep the same nodes -- the normal case, every
    real node has a target and a non-zero probability row -- is scored from
    per-node comparisons; any other graph goes through the reference's
    list-based path (get_las_uas compares the lists by POSITION).  The
    per-graph scores are added in graph order, as the reference does, so the
    result is bit-identical (tests/test_evaluation.py: fixtures of the
    reference's own functions)."""
    _, res, tgt = results_reshaped_btb(labels, computed_values, mask, num_vertices, output_size,
                                       output_size_edges)
    _, res_e, tgt_e = results_reshaped_btb(labels_e, computed_values_e, mask_edges, num_vertices, output_size,
                                           output_size_edges, is_edge=True)
    b, v, o = tgt.shape[0], tgt.shape[2], tgt.shape[3]
    if v < 2:
        return _batch_las_uas_lists(res, tgt, res_e, tgt_e)
    # node rows 1..v-1, (edge type, source) flattened: heads [b, v-1, o] (one edge
    # type), labels [b, v-1, e] (source 0)
    kt, ft = _first_max(tgt[:, 0, 1:, :], False)
    kr, fr = _first_max(res[:, 0, 1:, :], True)
    kte, fte = _first_max(np.transpose(tgt_e[:, :, 1:, 0], (0, 2, 1)), False)
    kre, fre = _first_max(np.transpose(res_e[:, :, 1:, 0], (0, 2, 1)), True)
    same = (kt == kr).all(axis=1) & (kt == kte).all(axis=1) & (kt == kre).all(axis=1)
    n = kt.sum(axis=1)
    head_ok = (ft == fr) & kt
    lab_ok = (fte == fre) & kt
    las_n = (head_ok & lab_ok).sum(axis=1)
    uas_n = head_ok.sum(axis=1)
    lab_n = lab_ok.sum(axis=1)
    acc_las = acc_uas = acc_uas_e = 0.0
    for i in range(b):
        if same[i] and n[i] > 0:
            ni = int(n[i])
            las, uas, uas_e = int(las_n[i]) / ni, int(uas_n[i]) / ni, int(lab_n[i]) / ni
        else:
            las, uas, uas_e = _graph_las_uas(res[i], tgt[i], res_e[i], tgt_e[i])
        acc_las += las
        acc_uas += uas
        acc_uas_e += uas_e
    return acc_las / b, acc_uas / b, acc_uas_e / b


def closed_form_masks(n_nodes, num_vertices, output_size, output_size_edges):
    """The btb masks of ``get_mask`` for a batch: (node_mask [b, v, o] with 1
    where i < n and j < n, node_mask_edges [b, v, e] with 1 where i < n), bool."""
    n = np.asarray(n_nodes).reshape(-1, 1)
    r = np.arange(int(num_vertices))[None, :] < n
    c = np.arange(int(output_size))[None, :] < n
    return r[:, :, None] & c[:, None, :], np.broadcast_to(r[:, :, None], r.shape + (int(output_size_edges),))


def _pred_of_masked(res, res_e):
    """pred [b, v, 2] int32 from masked probabilities [b, v, o] / [b, v, e]:
    each node row 1..v-1's first maximum, -1 for node 0 and an all-zero row."""
    pred = np.full(res.shape[:2] + (2,), -1, np.int32)
    keep, first = _first_max(res[:, 1:, :], True)
    pred[:, 1:, 0] = np.where(keep, first, -1)
    keep, first = _first_max(res_e[:, 1:, :], True)
    pred[:, 1:, 1] = np.where(keep, first, -1)
    return pred


def pred_from_masks(probs, probs_e, mask, mask_e):
    """decode_arrays' pred for a feed whose masks are not of get_mask's closed
    form: probs [b, v, o] / probs_e [b, v, e] (or flattened per graph) times
    the feed's own node_mask / node_mask_edges of the same sizes."""
    m, m_e = np.asarray(mask, np.float32), np.asarray(mask_e, np.float32)
    return _pred_of_masked(np.asarray(probs, np.float32).reshape(m.shape) * m,
                           np.asarray(probs_e, np.float32).reshape(m_e.shape) * m_e)


def _node_counts(n_nodes, b, v, o):
    """n_nodes as int64 [b], clipped to 0..min(v, o) as the kernels clip it."""
    n = np.clip(np.asarray(n_nodes).astype(np.int64).reshape(-1), 0, min(v, o))
    if n.shape[0] != b:
        raise ValueError("n_nodes: %d values for %d graphs" % (n.shape[0], b))
    return n


def _count_in_range(name, x, top, low=1):
    """int(x) for a count (K, num_samples; low 0: predict_batch's samples /
    kbest, 0 = off) that must lie in low..top."""
    x = int(x)
    if not low <= x <= top:
        raise ValueError("%s must lie in %d..%d (got %d)" % (name, low, top, x))
    return x


def _head_input(x, n_nodes, name, dtype, what):
    """How the host forms of the tree passes open: x as a [b, v, o] array
    (``name`` in the messages; int32 scores must come as int32, probabilities
    are converted to float32), the shape rule the kernels share (``what``
    opens its message) and _node_counts.  Returns (array, b, v, o, nn)."""
    a = np.asarray(x) if dtype == np.int32 else np.asarray(x, dtype)
    if a.ndim != 3 or a.dtype != dtype:
        raise ValueError("%s must be %s[b, v, o]" % (name, "int32 " if dtype == np.int32 else ""))
    b, v, o = a.shape
    if v > o or v > TREE_MAXV or o > 1024:
        raise ValueError("%s v <= o, v <= %d, o <= 1024 (got v %d, o %d)" % (what, TREE_MAXV, v, o))
    return a, b, v, o, _node_counts(n_nodes, b, v, o)


def decode_arrays(probs, probs_e, n_nodes, labels=None, labels_e=None):
    """The host form of ``ggnn_heads_decode`` (include/ggnn.h), written with
    the scorer's own ``_first_max``: probs [b, v, o] and probs_e [b, v, e] are
    masked in ``get_mask``'s closed form for n_nodes [b] (as
    results_reshaped_btb masks them), every node row 1..v-1 takes its first
    maximum (adj_mat_to_target), labels / labels_e (0/1, same shapes) their
    first exact 1.  Returns (pred [b, v, 2], gold [b, v, 2] or None, counts
    [b, 5]) as int32: zero-based (head, label) columns, -1 = the node is
    skipped; counts = (n_kept, las, uas, lab, regular) per graph, where
    regular says that every list skips the same nodes and the rows i < n hold
    no NaN / inf -- then the first four are batch_las_uas's per-graph counts."""
    p, pe = np.asarray(probs, np.float32), np.asarray(probs_e, np.float32)
    if p.ndim != 3 or pe.ndim != 3 or p.shape[:2] != pe.shape[:2]:
        raise ValueError("probs [b, v, o] and probs_e [b, v, e] expected, got %s and %s" % (p.shape, pe.shape))
    b, v, o = p.shape
    e = pe.shape[2]
    n = _node_counts(n_nodes, b, v, o)
    m, m_e = closed_form_masks(n, v, o, e)
    with np.errstate(invalid="ignore"):     # (inf * 0: a NaN, as on the reference's path)
        res, res_e = p * m.astype(np.float32), pe * m_e.astype(np.float32)
    pred = _pred_of_masked(res, res_e)
    real = m_e[:, 1:, 0]
    bad = ((~np.isfinite(p[:, 1:, :])).any(axis=2) | (~np.isfinite(pe[:, 1:, :])).any(axis=2)) & real
    kept = pred[:, 1:, 0] >= 0
    regular = ((pred[:, 1:, 1] >= 0) == kept).all(axis=1) & ~bad.any(axis=1)
    counts = np.zeros((b, 5), np.int32)
    gold = None
    if (labels is None) != (labels_e is None):
        raise ValueError("labels and labels_e are given together")
    if labels is not None:
        y, ye = np.asarray(labels, np.float32), np.asarray(labels_e, np.float32)
        if y.shape != p.shape or ye.shape != pe.shape:
            raise ValueError("labels must have the probabilities' shapes")
        gold = np.full((b, v, 2), -1, np.int32)
        keep, first = _first_max(y[:, 1:, :], False)
        gold[:, 1:, 0] = np.where(keep, first, -1)
        keep, first = _first_max(ye[:, 1:, :], False)
        gold[:, 1:, 1] = np.where(keep, first, -1)
        has = gold[:, 1:, 0] >= 0
        regular &= (has == kept).all(axis=1) & ((gold[:, 1:, 1] >= 0) == kept).all(axis=1)
        hit_h = has & (pred[:, 1:, 0] == gold[:, 1:, 0])
        hit_l = has & (pred[:, 1:, 1] == gold[:, 1:, 1])
        counts[:, 0] = has.sum(axis=1)
        counts[:, 1] = (hit_h & hit_l).sum(axis=1)
        counts[:, 2] = hit_h.sum(axis=1)
        counts[:, 3] = hit_l.sum(axis=1)
    counts[:, 4] = regular
    return pred, gold, counts


def scores_from_counts(counts, fallback):
    """batch_las_uas's (LAS, UAS, label accuracy) from the decode counts
    [b, 5]: the per-graph quotients in Python ints / floats, added in graph
    order.  A graph with regular == 0 or n_kept == 0 is scored by
    ``fallback(i)`` -> (las, uas, label accuracy): the reference's list path
    (graph_scores on its probabilities, or graph_scores_from_lists), which is
    what batch_las_uas does with such a graph -- bit-identical."""
    c = np.asarray(counts)
    b = c.shape[0]
    acc_las = acc_uas = acc_uas_e = 0.0
    for i in range(b):
        kept, las_n, uas_n, lab_n, regular = (int(x) for x in c[i])
        if regular and kept > 0:
            las, uas, uas_e = las_n / kept, uas_n / kept, lab_n / kept
        else:
            las, uas, uas_e = fallback(i)
        acc_las += las
        acc_uas += uas
        acc_uas_e += uas_e
    return acc_las / b, acc_uas / b, acc_uas_e / b


def graph_scores(labels, computed_values, mask, labels_e, computed_values_e, mask_e, num_vertices, output_size,
                 output_size_edges):
    """One graph ([v*o] / [v*e] rows of a batch's arrays) through the
    reference's lists: what batch_las_uas does with an irregular graph."""
    one = lambda a: np.asarray(a)[None]
    _, res, tgt = results_reshaped_btb(one(labels), one(computed_values), one(mask), num_vertices, output_size,
                                       output_size_edges)
    _, res_e, tgt_e = results_reshaped_btb(one(labels_e), one(computed_values_e), one(mask_e), num_vertices,
                                           output_size, output_size_edges, is_edge=True)
    return _graph_las_uas(res[0], tgt[0], res_e[0], tgt_e[0])


def lists_from_decoded(decoded):
    """decoded [v, 2] (one graph of decode's pred or gold) -> (head list,
    label list) as adj_mat_to_target gives them: [[head, 1], ...] and
    [[0, label], ...] (label one-based) over the nodes that are not skipped."""
    d = np.asarray(decoded)
    return [[int(x), 1] for x in d[1:, 0] if x >= 0], [[0, int(x) + 1] for x in d[1:, 1] if x >= 0]


def graph_scores_from_lists(pred, gold):
    """_graph_las_uas from one graph's decoded pred / gold [v, 2] instead of
    its probabilities (the decode's first maxima are adj_mat_to_target's)."""
    rg_h, rg_e = lists_from_decoded(pred)
    tg_h, tg_e = lists_from_decoded(gold)
    target_graph = merge_head_and_edge_graph(tg_h, tg_e)
    result_graph = merge_head_and_edge_graph(rg_h, rg_e)
    las, uas = get_las_uas(target_graph, result_graph)
    _, uas_e = get_las_uas(tg_e, rg_e, is_edge=True)
    return las, uas, uas_e


def _graph_las_uas(res, tgt, res_e, tgt_e):
    """One graph through the reference's lists (chem_tensorflow_dense.py:1179-1199)."""
    tg_h = adj_mat_to_target(tgt)
    tg_e = adj_mat_to_target(tgt_e)
    target_graph = merge_head_and_edge_graph(tg_h, tg_e)
    rg_h = adj_mat_to_target(res, is_probability=True, true_target=tg_h)
    rg_e = adj_mat_to_target(res_e, is_probability=True)
    result_graph = merge_head_and_edge_graph(rg_h, rg_e)
    las, uas = get_las_uas(target_graph, result_graph)
    _, uas_e = get_las_uas(tg_e, rg_e, is_edge=True)
    return las, uas, uas_e


def _batch_las_uas_lists(res, tgt, res_e, tgt_e):
    """batch_las_uas through the reference's per-graph lists only."""
    b = tgt.shape[0]
    acc_las = acc_uas = acc_uas_e = 0.0
    for i in range(b):
        tg_h = adj_mat_to_target(tgt[i])
        tg_e = adj_mat_to_target(tgt_e[i])
        target_graph = merge_head_and_edge_graph(tg_h, tg_e)
        rg_h = adj_mat_to_target(res[i], is_probability=True, true_target=tg_h)
        rg_e = adj_mat_to_target(res_e[i], is_probability=True)
        result_graph = merge_head_and_edge_graph(rg_h, rg_e)
        las, uas = get_las_uas(target_graph, result_graph)
        _, uas_e = get_las_uas(tg_e, rg_e, is_edge=True)
        acc_las += las
        acc_uas += uas
        acc_uas_e += uas_e
    return acc_las / b, acc_uas / b, acc_uas_e / b


# ------------------------------------------------- tree-constrained decoding
# Host forms of ``ggnn_tree_decode`` (include/ggnn.h): the maximum spanning
# arborescence of the head scores (Chu-Liu/Edmonds), exact integer arithmetic.
TREE_FORBIDDEN = -2 ** 31      # GGNN_TREE_FORBIDDEN
TREE_MAXV = 256                # GGNN_TREE_MAXV
TREE_LOG2_FLOOR = 150          # |log2| of the smallest positive float32 is 149
# a ROOT arc costs this much more under single_root: more than any difference
# of two trees' totals (2 * 255 * 2^31 < 2^40), far inside int64
_ROOT_PENALTY = 2 ** 42


def tree_score_shift(v):
    """k of tree_scores: the largest k <= 16 with 150 * 2^k * v * (v + 1) <=
    2^30 (the exactness contract of ggnn_tree_decode; 7 at v = 198, 12 at 40)."""
    k = 16
    while k > 0 and TREE_LOG2_FLOOR * int(v) * (int(v) + 1) * 2 ** k > 2 ** 30:
        k -= 1
    return k


def tree_scores(probs_head, n_nodes, v):
    """Integer arc scores of a batch for the tree decode: probs_head [b, v, o]
    -> int32 [b, v, o] with rint(log2(p) * 2^k), clamped below at -150 * 2^k,
    and TREE_FORBIDDEN where p <= 0 or p is NaN / +-inf, the row or column is
    >= n, the row is 0 or the arc is a self-loop.  The sum of the scores of a
    tree is the log of the product of its head probabilities at 2^-k bits."""
    p = np.asarray(probs_head, np.float32)
    if p.ndim != 3 or p.shape[1] != int(v):
        raise ValueError("probs_head [b, %d, o] expected, got %s" % (int(v), p.shape))
    b, _, o = p.shape
    n = np.asarray(n_nodes).astype(np.int64).reshape(-1, 1, 1)
    k = tree_score_shift(v)
    i = np.arange(int(v)).reshape(1, -1, 1)
    j = np.arange(o).reshape(1, 1, -1)
    ok = np.isfinite(p) & (p > 0) & (i < n) & (j < n) & (i != 0) & (i != j)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint(np.log2(np.where(ok, p, 1).astype(np.float64)) * float(2 ** k))
    q = np.maximum(q, -TREE_LOG2_FLOOR * 2 ** k)
    return np.where(ok, q, TREE_FORBIDDEN).astype(np.int32)


def _arc_allowed(scores, n, i, j):
    return 1 <= i < n and 0 <= j < n and j != i and int(scores[i][j]) != TREE_FORBIDDEN


def is_tree(heads, n, single_root, scores=None):
    """heads[i] for the words i in 1..n-1 (heads[0] is ignored): every head
    lies in 0..n-1, is not the word itself (and is an allowed arc of
    ``scores`` when given), following the heads from any word reaches node 0,
    and with single_root exactly one word has head 0."""
    n = int(n)
    h = [int(x) for x in heads[:n]]
    for i in range(1, n):
        if not (0 <= h[i] < n) or h[i] == i:
            return False
        if scores is not None and int(scores[i][h[i]]) == TREE_FORBIDDEN:
            return False
    for i in range(1, n):
        x = i
        for _ in range(n):
            if x == 0:
                break
            x = h[x]
        if x != 0:
            return False
    return not single_root or n < 2 or sum(1 for i in range(1, n) if h[i] == 0) == 1


def tree_total(scores, heads, n):
    """The sum of scores[i][heads[i]] over the words 1..n-1 (a Python int)."""
    return sum(int(scores[i][int(heads[i])]) for i in range(1, int(n)))


def _max_arborescence(s, n, single_root):
    """Chu-Liu/Edmonds on one graph, in the kernel's formulation: a supernode
    label and an accumulated offset per word give the adjusted score of an arc
    from the original scores; every round contracts all cycles of the
    supernodes' best incoming arcs; the contraction forest is expanded at the
    end.  Returns (heads or None when no tree exists, nesting levels)."""
    none = -2 ** 62
    s = np.asarray(s)[:n, :n].astype(np.int64)
    key = s.copy()
    if single_root:
        key[:, 0] -= _ROOT_PENALTY
    key[s == TREE_FORBIDDEN] = none
    key[0, :] = none
    key[np.arange(n), np.arange(n)] = none
    label = np.arange(n)            # word -> live node of the contraction forest
    off = np.zeros(n, np.int64)
    tpar = [-1] * (2 * n)           # forest parent; ids < n: the words themselves
    depth = [0] * (2 * n)
    in_u, in_i, best = [0] * (2 * n), [0] * (2 * n), [0] * (2 * n)
    nid, first_new = n, 1
    levels = 0
    done = False
    for _ in range(n):
        for x in range(first_new, nid):          # the nodes new in this round
            members = np.flatnonzero(label == x)
            vals = np.where((label != x)[None, :] & (key[members] != none), key[members] - off[members, None], none)
            k = int(vals.argmax())               # first word, then first column
            w, j = divmod(k, n)
            if vals[w, j] == none:
                return None, levels
            best[x], in_u[x], in_i[x] = int(vals[w, j]), j, int(members[w])
        live = sorted(set(int(x) for x in label[1:]))
        par = {x: int(label[in_u[x]]) for x in live}
        par[0] = 0
        on_cycle = {}
        state = {0: 2}                           # 1 = on the current walk, 2 = settled
        for x in live:
            walk, y = [], x
            while y not in state:
                state[y] = 1
                walk.append(y)
                y = par[y]
            if state[y] == 1:
                cyc = walk[walk.index(y):]
                for z in cyc:
                    on_cycle[z] = min(cyc)
            for z in walk:
                state[z] = 2
        if not on_cycle:
            done = True
            break
        first_new = nid
        new_of = {}
        for lead in sorted(set(on_cycle.values())):
            new_of[lead] = nid
            nid += 1
        for x, lead in on_cycle.items():
            tpar[x] = new_of[lead]
            depth[new_of[lead]] = max(depth[new_of[lead]], depth[x] + 1)
            levels = max(levels, depth[new_of[lead]])
        for i in range(1, n):
            x = int(label[i])
            if x in on_cycle:
                off[i] += best[x]
                label[i] = new_of[on_cycle[x]]
    if not done:
        return None, levels
    heads = [-1] * n
    entered = [False] * (2 * n)
    for x in range(nid - 1, 0, -1):
        if entered[x]:
            continue
        heads[in_i[x]] = in_u[x]
        y = in_i[x]
        while y != x:
            entered[y] = True
            y = tpar[y]
    if single_root and sum(1 for i in range(1, n) if heads[i] == 0) != 1:
        return None, levels
    return heads, levels


def _repair_arrays(what, fine, solve, scores, n_nodes, pred, gold, counts):
    """What tree_decode_arrays and projective_decode_arrays share: the
    argument checks, the copies, the per-graph loop, the status and the
    recount.  ``fine(scores[g], n, heads)``: the graph's heads are left alone
    (status 0); else ``solve(scores[g], n)`` gives its new heads (status 1) or
    None (status 2)."""
    s, b, v, o, nn = _head_input(scores, n_nodes, "scores", np.int32, what + " decode needs")
    pred = np.array(pred, np.int32)
    if pred.shape != (b, v, 2):
        raise ValueError("pred must be [%d, %d, 2]" % (b, v))
    if (gold is None) != (counts is None):
        raise ValueError("gold and counts are given together")
    if counts is not None:
        counts = np.array(counts, np.int32)
        gold = np.asarray(gold)
    status = np.zeros(b, np.int32)
    for g in range(b):
        n = int(nn[g])
        if n < 2 or fine(s[g], n, pred[g, :, 0]):
            continue
        heads = solve(s[g], n)
        if heads is None:
            status[g] = 2
            continue
        status[g] = 1
        pred[g, 1:n, 0] = heads[1:]
        if counts is not None:
            has = gold[g, 1:, 0] >= 0
            hit_h = has & (pred[g, 1:, 0] == gold[g, 1:, 0])
            counts[g, 1] = int((hit_h & (pred[g, 1:, 1] == gold[g, 1:, 1])).sum())
            counts[g, 2] = int(hit_h.sum())
    return pred, counts, status


def tree_decode_arrays(scores, n_nodes, pred, single_root=True, gold=None, counts=None, levels=None):
    """The host form of ``ggnn_tree_decode`` (include/ggnn.h).  scores int32
    [b, v, o], n_nodes [b], pred int32 [b, v, 2] (decode_arrays'), gold
    [b, v, 2] and counts [b, 5] together or both None.  Returns (pred, counts,
    status): copies with every graph whose heads pred[g, 1:n, 0] are not a tree
    over the allowed arcs (status 1) given a tree of maximum total score and
    its las / uas counts recounted; status 0 = already a tree, 2 = no tree
    exists; those graphs are returned as passed in.  ``levels``: a list that
    receives per graph the nesting depth of the contractions it needed."""
    depths = []                  # of the graphs that were solved, in graph order

    def solve(sg, n):
        heads, lv = _max_arborescence(sg, n, single_root)
        depths.append(lv)
        return heads

    out = _repair_arrays("tree", lambda sg, n, heads: is_tree(heads, n, single_root, sg), solve, scores, n_nodes,
                         pred, gold, counts)
    if levels is not None:
        solved = iter(depths)
        levels[:] = [next(solved) if st else 0 for st in out[2]]
    return out


# -------------------------------------------------------- projective decoding
# Host form of ``ggnn_projective_decode`` (include/ggnn.h, csrc/k_proj.h):
# Eisner's span dynamic programme, vectorised over the spans of one length.
PROJ_LDS_MAXN = 128            # GGNN_PROJ_LDS_MAXN
_PROJ_NEG = -2 ** 30           # a span without a derivation; no total reaches it (the range rule)


def is_projective(heads, n):
    """heads[i] for the words 1..n-1 (heads[0] is ignored; node 0 is the
    leftmost position): no two arcs (i, heads[i]), (j, heads[j]) have
    endpoints a < c < b < d, ROOT arcs included."""
    n = int(n)
    if n < 3:
        return True
    h = np.asarray([int(x) for x in heads[1:n]], np.int64)
    w = np.arange(1, n)
    lo, hi = np.minimum(w, h), np.maximum(w, h)
    return not bool(((lo[:, None] < lo[None, :]) & (lo[None, :] < hi[:, None]) & (hi[:, None] < hi[None, :])).any())


def _proj_add(a, b):
    return np.where((a == _PROJ_NEG) | (b == _PROJ_NEG), _PROJ_NEG, a + b)


def _range_ok(scores_g, n):
    """The range rule of the integer span programmes: S * (n - 1) < 2^30 for
    the largest absolute allowed score S of the graph's n nodes (no total
    then reaches _PROJ_NEG)."""
    a = scores_g[1:n, :n].astype(np.int64)
    live = a != TREE_FORBIDDEN
    live[np.arange(n - 1), np.arange(1, n)] = False
    return int(np.abs(a[live]).max(initial=0)) * (n - 1) < 2 ** 30


def _eisner(s, n, single_root):
    """The best projective tree of one graph in the kernel's formulation (the
    tables by diagonals T[d, s] = span s..s+d, the smallest split point or
    ROOT child among equals).  Returns heads (list, [0] is -1) or None."""
    lo = 1 if single_root else 0
    m = n - lo
    full = np.asarray(s)[:n, :n].astype(np.int64)
    w = full[lo:, lo:].copy()                  # w[i, j]: position i takes head at position j
    w[full[lo:, lo:] == TREE_FORBIDDEN] = _PROJ_NEG
    w[np.arange(m), np.arange(m)] = _PROJ_NEG
    if not single_root:
        w[0, :] = _PROJ_NEG                    # node 0 is never a dependent
    TR = np.full((m, m), _PROJ_NEG, np.int64)  # complete, headed at the left end
    TL = TR.copy()                             # complete, headed at the right end
    UR, UL = TR.copy(), TR.copy()              # incomplete, arc s -> t / t -> s
    TR[0, :] = TL[0, :] = 0
    for L in range(1, m):
        st = np.arange(m - L)
        k = np.arange(L)[:, None]
        base = _proj_add(TR[k, st], TL[L - 1 - k, st + k + 1]).max(axis=0)
        UR[L, st] = _proj_add(base, w[st + L, st])
        UL[L, st] = _proj_add(base, w[st, st + L])
        TR[L, st] = _proj_add(UR[k + 1, st], TR[L - 1 - k, st + k + 1]).max(axis=0)
        TL[L, st] = _proj_add(TL[k, st], UL[L - k, st + k]).max(axis=0)
    heads = [-1] * n
    stack = []

    def push(kind, a, b):
        if a != b or kind >= 2:
            stack.append((kind, a, b))

    if single_root:
        p = np.arange(m)
        root = full[1:, 0].copy()
        root[root == TREE_FORBIDDEN] = _PROJ_NEG
        tot = _proj_add(_proj_add(TL[p, 0], TR[m - 1 - p, p]), root)
        if tot.max() == _PROJ_NEG:
            return None
        r = int(np.argmax(tot))                # the first maximum
        heads[lo + r] = 0
        push(1, 0, r)
        push(0, r, m - 1)
    else:
        if TR[m - 1, 0] == _PROJ_NEG:
            return None
        push(0, 0, m - 1)
    while stack:
        kind, a, b = stack.pop()
        L = b - a
        k = np.arange(L)
        if kind == 0:
            c, target = _proj_add(UR[k + 1, a], TR[L - 1 - k, a + k + 1]), TR[L, a]
        elif kind == 1:
            c, target = _proj_add(TL[k, a], UL[L - k, a + k]), TL[L, a]
        else:
            c = _proj_add(TR[k, a], TL[L - 1 - k, a + k + 1])
            if kind == 2:
                heads[lo + b] = lo + a
                target = UR[L, a] - w[b, a]
            else:
                heads[lo + a] = lo + b
                target = UL[L, a] - w[a, b]
        f = int(np.flatnonzero((c != _PROJ_NEG) & (c == target))[0])
        if kind == 0:
            push(2, a, a + f + 1)
            push(0, a + f + 1, b)
        elif kind == 1:
            push(1, a, a + f)
            push(3, a + f, b)
        else:
            push(0, a, a + f)
            push(1, a + f + 1, b)
    return heads


def projective_decode_arrays(scores, n_nodes, pred, single_root=True, gold=None, counts=None):
    """The host form of ``ggnn_projective_decode`` (include/ggnn.h): the
    arguments of tree_decode_arrays.  Returns (pred, counts, status): copies
    with every graph whose heads pred[g, 1:n, 0] are not a projective tree over
    the allowed arcs (status 1) given a projective tree of maximum total score
    (Eisner; the smallest split point or ROOT child among equals) and its las /
    uas recounted; status 0 = already a projective tree (or n < 2), 2 = S *
    (n - 1) >= 2^30 for the largest absolute allowed score S, or no projective
    tree exists; those graphs are returned as passed in."""
    return _repair_arrays("projective",
                          lambda sg, n, heads: is_tree(heads, n, single_root, sg) and is_projective(heads, n),
                          lambda sg, n: _eisner(sg, n, single_root) if _range_ok(sg, n) else None,
                          scores, n_nodes, pred, gold, counts)


def random_projective_heads(n, rng):
    """A random projective single-rooted tree over nodes 0..n-1 (heads[0] =
    -1), drawn by random shift / left-arc / right-arc transitions of a stack
    parser: ROOT stays at the bottom of the stack and takes its one child last."""
    n = int(n)
    heads = [-1] * n
    stack, nxt = [0], 1
    while nxt < n or len(stack) > 2:
        if len(stack) > 2 and (nxt >= n or rng.random() < 0.5):
            if rng.random() < 0.5:
                heads[stack[-1]] = stack[-2]     # right-arc
                stack.pop()
            else:
                heads[stack[-2]] = stack[-1]     # left-arc
                del stack[-2]
        else:
            stack.append(nxt)
            nxt += 1
    if len(stack) == 2:
        heads[stack[1]] = 0
    return heads


# ------------------------------------------------- k-best projective trees
# Host form of ``ggnn_projective_kbest`` (include/ggnn.h, csrc/k_proj_kbest.h):
# _eisner's tables with a sorted list of up to K entries per item.  IR and IL of
# a span share the base list BS (they differ by the arc's score alone).  A
# candidate of an item is (split, rank in the first child, rank in the second
# child); a list is the first K candidates in the total order: larger total
# first, then the smaller split, the smaller first rank, the smaller second
# rank.  Candidate (r, i, j) has (i + 1)(j + 1) - 1 candidates of its split
# ahead of it, so only the pairs with (i + 1)(j + 1) <= K are formed.  Every
# entry keeps its (split, i, j) packed as split << 8 | i << 4 | j; the trees are
# read back from those.
KBEST_MAX = 16                 # GGNN_KBEST_MAX


def _kbest_take(tot, K):
    """tot int64 [C, spans]: the candidates' totals in the order (split, i, j)
    along axis 0 (_PROJ_NEG = no such candidate), C >= K.  Returns (values [K,
    spans], candidate indices [K, spans]) of the first K in the total order (a
    stable sort by descending total keeps the order of equals)."""
    order = np.argsort(-tot, axis=0, kind="stable")[:K]
    return np.take_along_axis(tot, order, axis=0), order


def _kbest_tables(s, n, single_root, K):
    """The lists of one graph: (CR, CL, BS values [K, m, m] by (rank, d, s),
    their back-pointers, the final list's values [K] and back-pointers [K])."""
    lo = 1 if single_root else 0
    m = n - lo
    full = np.asarray(s)[:n, :n].astype(np.int64)
    w = full[lo:, lo:].copy()                  # w[i, j]: position i takes head at position j
    w[full[lo:, lo:] == TREE_FORBIDDEN] = _PROJ_NEG
    w[np.arange(m), np.arange(m)] = _PROJ_NEG
    if not single_root:
        w[0, :] = _PROJ_NEG                    # node 0 is never a dependent
    pairs = np.asarray([(i, j) for i in range(K) for j in range(K // (i + 1))], np.int64)
    pi, pj = pairs[:, 0][None, :, None], pairs[:, 1][None, :, None]
    code = (pairs[:, 0] << 4) | pairs[:, 1]
    CR = np.full((K, m, m), _PROJ_NEG, np.int64)
    CL, BS = CR.copy(), CR.copy()
    CRB, CLB, BSB = (np.zeros((K, m, m), np.int64) for _ in range(3))
    CR[0, 0, :] = CL[0, 0, :] = 0

    def take(tot, L):
        val, idx = _kbest_take(tot.reshape(-1, m - L), K)
        return val, np.where(val == _PROJ_NEG, 0, ((idx // len(code)) << 8) | code[idx % len(code)])

    for L in range(1, m):
        st = np.arange(m - L)[None, None, :]
        k = np.arange(L)[:, None, None]
        sl = np.arange(m - L)
        BS[:, L, sl], BSB[:, L, sl] = take(_proj_add(CR[pi, k, st], CL[pj, L - 1 - k, st + k + 1]), L)
        ar = w[st + k + 1, st]                 # word s+k+1 takes head s
        al = w[st + k, st + L]                 # word s+k takes head t
        CR[:, L, sl], CRB[:, L, sl] = take(_proj_add(_proj_add(BS[pi, k + 1, st], ar), CR[pj, L - 1 - k, st + k + 1]), L)
        CL[:, L, sl], CLB[:, L, sl] = take(_proj_add(_proj_add(CL[pi, k, st], al), BS[pj, L - k, st + k]), L)
    if single_root:
        p = np.arange(m)[:, None, None]
        root = full[1:, 0].copy()
        root[root == TREE_FORBIDDEN] = _PROJ_NEG
        tot = _proj_add(_proj_add(CL[pi, p, 0], root[p]), CR[pj, m - 1 - p, p])
        val, idx = _kbest_take(tot.reshape(-1, 1), K)
        fv, fb = val[:, 0], (((idx // len(code)) << 8) | code[idx % len(code)])[:, 0]
    else:
        fv, fb = CR[:, m - 1, 0].copy(), np.zeros(K, np.int64)
    return (CR, CL, BS), (CRB, CLB, BSB), fv, fb


def _kbest_walk(backs, fb, rank, n, single_root):
    """The heads (list, [0] is -1) of the final list's entry ``rank``."""
    lo = 1 if single_root else 0
    m = n - lo
    heads = [-1] * n
    stack = []

    def push(kind, r, a, b):                   # kinds: 0 CR, 1 CL, 2 BS under a -> b, 3 BS under b -> a
        if a < b:
            stack.append((kind, r, a, b))

    if single_root:
        bp = int(fb[rank])
        p = bp >> 8
        heads[lo + p] = 0
        push(1, (bp >> 4) & 15, 0, p)
        push(0, bp & 15, p, m - 1)
    else:
        push(0, rank, 0, m - 1)
    while stack:
        kind, r, a, b = stack.pop()
        bp = int(backs[min(kind, 2)][r, b - a, a])
        k, i, j = bp >> 8, (bp >> 4) & 15, bp & 15
        if kind == 0:
            push(2, i, a, a + k + 1)
            push(0, j, a + k + 1, b)
        elif kind == 1:
            push(1, i, a, a + k)
            push(3, j, a + k, b)
        else:
            if kind == 2:
                heads[lo + b] = lo + a
            else:
                heads[lo + a] = lo + b
            push(0, i, a, a + k)
            push(1, j, a + k + 1, b)
    return heads


def projective_kbest_arrays(scores, n_nodes, K, single_root=True):
    """The host form of ``ggnn_projective_kbest`` (include/ggnn.h): the K best
    projective trees of every graph in order.  scores int32 [b, v, o]
    (``tree_scores``), n_nodes [b], 1 <= K <= KBEST_MAX.  Returns (heads int32
    [b, K, v]: the head of word i in the tree of rank k, -1 on node 0, rows >=
    n and ranks >= count; totals int32 [b, K]: the tree's sum of scores,
    TREE_FORBIDDEN on ranks >= count; count int32 [b]; status int32 [b]: 0 = n
    < 2, 1 = count >= 1, 2 = S * (n - 1) >= 2^30 for the largest absolute
    allowed score S, or no projective tree exists).  Rank 0 is _eisner's tree,
    ties included; the list for K is a prefix of the list for a larger K."""
    s, b, v, o, nn = _head_input(scores, n_nodes, "scores", np.int32, "projective k-best needs")
    K = _count_in_range("K", K, KBEST_MAX)
    heads = np.full((b, K, v), -1, np.int32)
    totals = np.full((b, K), TREE_FORBIDDEN, np.int32)
    count, status = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        status[g] = 2
        if not _range_ok(s[g], n):
            continue
        _, backs, fv, fb = _kbest_tables(s[g], n, bool(single_root), K)
        c = int((fv != _PROJ_NEG).sum())
        if c == 0:
            continue
        status[g], count[g] = 1, c
        totals[g, :c] = fv[:c]
        for r in range(c):
            heads[g, r, :n] = _kbest_walk(backs, fb, r, n, bool(single_root))
    return heads, totals, count, status


# ------------------------------------- k-best trees over all dependency trees
# Host form of ``ggnn_tree_kbest`` (include/ggnn.h, csrc/k_tree_kbest.h):
# Lawler's partitioning over _max_arborescence.  A subproblem = a partial head
# assignment fix[w] (-1 = free) and a list of excluded arcs (word, head); its
# best tree is the maximum arborescence of the masked scores.  The tree h that
# becomes rank r leaves one child per free word w, in increasing w: the free
# words below w fixed to h, (w, h[w]) excluded on top of the inherited
# exclusions.  The pool holds every solved child; the next rank is its first
# entry by (larger total, smaller parent rank, smaller word).
def _masked_scores(s, n, fix, excluded):
    """int32 [n, n]: s with the row of every fixed word forbidden except at
    its head and every excluded arc forbidden."""
    m = np.array(np.asarray(s)[:n, :n], np.int32)
    for w in range(1, n):
        if fix[w] >= 0:
            keep = m[w, fix[w]]
            m[w, :] = TREE_FORBIDDEN
            m[w, fix[w]] = keep
    for w, h in excluded:
        m[w, h] = TREE_FORBIDDEN
    return m


def _tree_kbest_graph(s, n, single_root, K):
    """[(total, heads)] of one graph: up to K trees, best first."""
    heads, _ = _max_arborescence(s, n, single_root)
    if heads is None:
        return []
    ranks, pool = [], {}                        # pool: (parent rank, word) -> (total, heads, fix, excluded)
    cand = (tree_total(s, heads, n), heads, [-1] * n, [])
    while True:
        total, h, fix, excluded = cand
        r = len(ranks)
        ranks.append((total, h))
        if r + 1 == K:
            break
        fix = list(fix)
        for w in range(1, n):
            if fix[w] >= 0:
                continue
            ex = excluded + [(w, h[w])]
            child, _ = _max_arborescence(_masked_scores(s, n, fix, ex), n, single_root)
            if child is not None:
                pool[(r, w)] = (tree_total(s, child, n), child, list(fix), ex)
            fix[w] = h[w]
        if not pool:
            break
        first = min(pool, key=lambda pw: (-pool[pw][0], pw[0], pw[1]))
        cand = pool.pop(first)
    return ranks


def tree_kbest_arrays(scores, n_nodes, K, single_root=True):
    """The host form of ``ggnn_tree_kbest`` (include/ggnn.h): the K best trees
    over ALL dependency trees (arcs may cross) of every graph in order.
    scores int32 [b, v, o] (``tree_scores``), n_nodes [b], 1 <= K <=
    KBEST_MAX.  Returns (heads int32 [b, K, v]: the head of word i in the tree
    of rank k, -1 on node 0, rows >= n and ranks >= count; totals int32
    [b, K]: the tree's sum of scores, TREE_FORBIDDEN on ranks >= count; count
    int32 [b]; status int32 [b]: 0 = n < 2, 1 = count >= 1, 2 = S * (n - 1) >=
    2^30 for the largest absolute allowed score S, or no tree exists).  Rank 0
    is _max_arborescence's tree, ties included; the list for K is a prefix of
    the list for a larger K."""
    s, b, v, o, nn = _head_input(scores, n_nodes, "scores", np.int32, "tree k-best needs")
    K = _count_in_range("K", K, KBEST_MAX)
    heads = np.full((b, K, v), -1, np.int32)
    totals = np.full((b, K), TREE_FORBIDDEN, np.int32)
    count, status = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        status[g] = 2
        if not _range_ok(s[g], n):
            continue
        ranks = _tree_kbest_graph(s[g], n, bool(single_root), K)
        if not ranks:
            continue
        status[g], count[g] = 1, len(ranks)
        for r, (total, h) in enumerate(ranks):
            totals[g, r] = total
            heads[g, r, 1:n] = h[1:]
    return heads, totals, count, status


# ------------------------------------------------- projective arc marginals
# Host form of ``ggnn_projective_marginals`` (include/ggnn.h, csrc/k_marg.h):
# the sum-product twin of _eisner (inside pass, explicit outside pass), in log
# space, vectorised over the spans of one length.
MARG_LDS_MAXN = 107            # GGNN_MARG_LDS_MAXN
MARG_SCORE_SCALE = 2 ** 20     # scores = rint(marg * 2^20)


def _lse(x, axis=0):
    """log-sum-exp along an axis: the maximum first, then the sum of exp(x -
    max); -inf where every term is -inf (no -inf is ever subtracted)."""
    mx = x.max(axis=axis)
    safe = np.where(mx == -np.inf, 0, mx).astype(x.dtype)
    with np.errstate(divide="ignore"):
        out = safe + np.log(np.exp(x - np.expand_dims(safe, axis)).sum(axis=axis, dtype=x.dtype))
    return np.where(mx == -np.inf, -np.inf, out).astype(x.dtype)


def _arc_log_potentials(p, n, dtype):
    """ln p where the arc "word i takes head j" is allowed (tree_scores' rule:
    finite, > 0, 1 <= i < n, j < n, j != i), -inf elsewhere; [n, n]."""
    q = np.asarray(p)[:n, :n].astype(dtype)
    ok = np.isfinite(q) & (q > 0)
    ok[0, :] = False
    ok[np.arange(n), np.arange(n)] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, np.log(np.where(ok, q, 1)), -np.inf).astype(dtype), ok


def _inside(psi, n, single_root):
    """One graph's inside pass: psi [n, n] log potentials (-inf = not
    allowed).  Returns (the tables [CR, CL, IR, IL] with T[d, s] the span
    s..s+d over the positions 0..m-1 = the nodes lo..n-1, logz, w, root): w the
    positions' own potentials, root [m] those of ROOT's arcs (None without
    single_root); logz = -inf when no projective tree exists."""
    dt = psi.dtype
    lo = 1 if single_root else 0
    m = n - lo
    w = psi[lo:, lo:]                                   # w[i, j]: position i takes the head at position j
    root = psi[1:, 0] if single_root else None
    neg = lambda: np.full((m, m), -np.inf, dt)
    CR, CL, IR, IL = neg(), neg(), neg(), neg()         # T[d, s]: the span s..s+d, as _eisner's tables
    CR[0, :] = CL[0, :] = 0
    for L in range(1, m):
        st = np.arange(m - L)
        k = np.arange(L)[:, None]
        base = _lse(CR[k, st] + CL[L - 1 - k, st + k + 1])
        IR[L, st] = base + w[st + L, st]
        IL[L, st] = base + w[st, st + L]
        CR[L, st] = _lse(IR[k + 1, st] + CR[L - 1 - k, st + k + 1])
        CL[L, st] = _lse(CL[k, st] + IL[L - k, st + k])
    p = np.arange(m)
    if single_root:
        logz = _lse(CL[p, 0] + CR[m - 1 - p, p] + root)
    else:
        logz = CR[m - 1, 0]
    return [CR, CL, IR, IL], logz, w, root


def _inside_outside(psi, n, single_root):
    """One graph: psi [n, n] log potentials (-inf = not allowed).  Returns
    (logz, marg [n, n] in psi's dtype, the largest absolute finite table
    value, ln Z included); logz = -inf when no projective tree exists."""
    dt = psi.dtype
    lo = 1 if single_root else 0
    m = n - lo
    tables, logz, w, root = _inside(psi, n, single_root)
    CR, CL, IR, IL = tables
    neg = lambda: np.full((m, m), -np.inf, dt)
    p = np.arange(m)
    marg = np.zeros((n, n), dt)
    if not np.isfinite(logz):
        return dt.type(-np.inf), marg, 0.0
    # the outside pass, from the longest length down: complete spans first
    # (they gather from longer spans only), then the incomplete spans
    oCR, oCL, oB = neg(), neg(), neg()                  # oB: outside of `base`, the lse of both arcs' outsides
    tables += [oCR, oCL, oB]
    for L in range(m - 1, 0, -1):
        S = m - L
        st = np.arange(S)
        t = st + L
        j = np.arange(S)[:, None]                       # j + 1 spans to the left / j + 1 to the right
        left = j < st                                   # st - 1 - j >= 0
        a = np.where(left, st - 1 - j, 0)
        right = t + 1 + j <= m - 1
        c = np.where(right, t + 1, 0)
        d = np.where(right, L + 1 + j, 0)
        e = np.where(left, L + 1 + j, 0)
        with np.errstate(invalid="ignore"):
            # CR[s][t]: the right part of CR[a][t] = IR[a][s] + CR[s][t], the left part of base[s][t']
            x = [np.where(left, oCR[e, a] + IR[j + 1, a], -np.inf), np.where(right, oB[d, st] + CL[j, c], -np.inf)]
            # CL[s][t]: the left part of CL[s][t'] = CL[s][t] + IL[t][t'], the right part of base[a][t]
            y = [np.where(right, oCL[d, st] + IL[np.where(right, j + 1, 0), np.where(right, t, 0)], -np.inf),
                 np.where(left, oB[e, a] + CR[j, a], -np.inf)]
        ir = np.full(S, -np.inf, dt)
        il = np.full(S, -np.inf, dt)
        if single_root:
            ir[S - 1] = CL[S - 1, 0] + root[S - 1]      # t = m - 1: ROOT's child is position s
            il[0] = CR[m - 1 - L, L] + root[L]          # s = 0: ROOT's child is position t
        elif L == m - 1:
            ir[0] = 0
        oCR[L, st] = _lse(np.concatenate(x + [ir[None]]).astype(dt))
        oCL[L, st] = _lse(np.concatenate(y + [il[None]]).astype(dt))
        # IR[s][t]: the left part of CR[s][t'], t' >= t;  IL[s][t]: the right part of CL[a][t], a <= s
        j = np.arange(S)[:, None]
        right = t + j <= m - 1
        left = j <= st
        a = np.where(left, st - j, 0)
        oIR = _lse(np.where(right, oCR[np.where(right, L + j, 0), st] + CR[j, np.where(right, t, 0)], -np.inf).astype(dt))
        oIL = _lse(np.where(left, oCL[np.where(left, L + j, 0), a] + CL[j, a], -np.inf).astype(dt))
        wr, wl = w[t, st], w[st, t]
        oB[L, st] = _lse(np.stack([oIR + wr, oIL + wl]))
        with np.errstate(invalid="ignore"):
            marg[lo + t, lo + st] = np.exp(np.where(np.isfinite(IR[L, st] + oIR), IR[L, st] + oIR - logz, -np.inf))
            marg[lo + st, lo + t] = np.exp(np.where(np.isfinite(IL[L, st] + oIL), IL[L, st] + oIL - logz, -np.inf))
    if single_root:
        x = CL[p, 0] + CR[m - 1 - p, p] + root
        marg[1 + p, 0] = np.exp(np.where(np.isfinite(x), x - logz, -np.inf))
    # (ln Z counts as the last cell of the inside pass: without single_root it is CR[0][m-1] itself)
    span_max = max([float(np.abs(T[np.isfinite(T)]).max(initial=0.0)) for T in tables] + [abs(float(logz))])
    return logz, np.minimum(marg, 1).astype(dt), span_max


def _marginals_out(marg, scores, g, n, ok, mg):
    """Graph g's written marginals, for both marginals forms: mg [n, n] on the
    allowed arcs ``ok`` and 0 elsewhere into marg[g]; rint(marg * 2^20) of the
    float32 marginals on the allowed arcs into scores[g] (TREE_FORBIDDEN
    elsewhere, as it was filled)."""
    marg[g] = 0
    marg[g, :n, :n] = np.where(ok, mg, 0)
    scores[g, :n, :n] = np.where(ok, np.rint(marg[g, :n, :n].astype(np.float32) * np.float32(MARG_SCORE_SCALE)),
                                 TREE_FORBIDDEN).astype(np.int32)


def projective_marginals_arrays(probs_head, n_nodes, single_root=True, dtype=np.float64):
    """The host form of ``ggnn_projective_marginals`` (include/ggnn.h):
    probs_head float32 [b, v, o], n_nodes [b].  The potential of "word i takes
    head j" is probs_head[g, i, j] where tree_scores allows the arc; a
    projective tree (ROOT leftmost, no crossing arcs, single_root: one ROOT
    child) weighs the product of its words' potentials.  Returns (marg
    [b, v, o], logz [b], scores int32 [b, v, o], status int32 [b], span_max
    [b]): marg[g, i, j] the share of the weight of the trees with that arc (0
    for an arc that is not allowed), logz the natural log of the total weight,
    scores = rint(marg * 2^20) on the allowed arcs and TREE_FORBIDDEN
    elsewhere; status 1 = written, 0 = n < 2, 2 = no projective tree exists:
    for status != 1 marg[g] is a copy of probs_head[g] and scores[g] is
    TREE_FORBIDDEN everywhere (logz 0 / -inf).  span_max[g]: the largest
    absolute finite value of the inside and outside tables and of logz
    (float; what an fp32 kernel's stored values are rounded at).  The tables
    are kept in ``dtype``."""
    p, b, v, o, nn = _head_input(probs_head, n_nodes, "probs_head", np.float32, "projective marginals need")
    dt = np.dtype(dtype)
    marg = p.astype(dt)
    logz = np.zeros(b, dt)
    scores = np.full((b, v, o), TREE_FORBIDDEN, np.int32)
    status = np.zeros(b, np.int32)
    span_max = np.zeros(b, np.float64)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        psi, ok = _arc_log_potentials(p[g], n, dt)
        lz, mg, span_max[g] = _inside_outside(psi, n, bool(single_root))
        logz[g] = lz
        if not np.isfinite(lz):
            status[g] = 2
            continue
        status[g] = 1
        _marginals_out(marg, scores, g, n, ok, mg)
    return marg, logz, scores, status, span_max


def arc_confidence_arrays(marg, n_nodes, pred):
    """The host form of ``ggnn_arc_confidence``: conf[g, i] = marg[g, i,
    pred[g, i, 0]] as float32, 0 where the predicted head is -1 or the row is
    0 or >= n."""
    mg = np.asarray(marg)
    pred = np.asarray(pred)
    b, v, o = mg.shape
    if pred.shape != (b, v, 2):
        raise ValueError("pred must be [%d, %d, 2]" % (b, v))
    n = np.clip(np.asarray(n_nodes).astype(np.int64).reshape(-1), 0, min(v, o))
    h = pred[:, :, 0].astype(np.int64)
    i = np.arange(v)[None, :]
    ok = (h >= 0) & (h < o) & (i >= 1) & (i < n[:, None])
    got = np.take_along_axis(mg, np.where(ok, h, 0)[:, :, None], axis=2)[:, :, 0]
    return np.where(ok, got, 0).astype(np.float32)


# ------------------------------------------------ non-projective arc marginals
# Host form of ``ggnn_tree_marginals`` (include/ggnn.h, csrc/k_lapl.h): the
# distribution over ALL dependency trees by the matrix-tree theorem (Koo et al.
# 2007; Smith & Smith 2007; McDonald & Satta 2007), np.linalg in place of the
# kernel's Gauss-Jordan elimination.
LAPL_LDS_MAXN = 199            # GGNN_LAPL_LDS_MAXN


def _normalised_potentials(p, n, dt):
    """One graph: (w [n, n] in dt, ok [n, n], ln_c float64).  w: the allowed
    potentials (tree_scores' rule) with every word's row divided by its own sum
    c[i], 0 elsewhere; a row is scaled by the power of two of its largest entry
    before it is summed (exact, so a row of fp32 subnormals loses nothing);
    ln_c = sum ln c[i].  A word without an allowed arc keeps a zero row."""
    q = np.asarray(p)[:n, :n].astype(np.float32)
    ok = np.isfinite(q) & (q > 0)
    ok[0, :] = False
    ok[np.arange(n), np.arange(n)] = False
    x = np.where(ok, q, np.float32(0))
    _, e = np.frexp(x.max(axis=1))
    scaled = np.ldexp(x, -e[:, None]).astype(dt)
    c = scaled.sum(axis=1, dtype=dt)
    live = c > 0
    w = scaled / np.where(live, c, 1).astype(dt)[:, None]
    ln_c = float(np.sum(np.log(c[live].astype(np.float64)) + e[live] * np.log(2.0)))
    return w.astype(dt), ok, ln_c


def _has_tree(ok, n, single_root):
    """Whether a dependency tree exists over the allowed arcs ok[i, j] ("word i
    may take head j"), decided on the arcs alone: without single_root every
    word is reachable from node 0 walking head -> dependent; with it some word
    with an allowed ROOT arc reaches every other word among the words."""
    reach = _reach(ok, n)
    if not single_root:
        return bool(reach[0, 1:].all())
    return bool((ok[1:, 0] & reach[1:, 1:].all(axis=1)).any())


def _reach(ok, n):
    """reach[j, i]: node i is j or below j walking head -> dependent over the
    allowed arcs ok[i, j]."""
    reach = ok.T | np.eye(n, dtype=bool)
    hops = 1
    while hops < n:                                     # boolean squaring: paths of up to 2^t arcs
        reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        hops *= 2
    return reach


def _laplacian(w, n, single_root):
    """A [(n-1), (n-1)] over the words of the normalised potentials w:
    A[h][d] = -w(d, h), A[d][d] = r(d) + sum_h w(d, h); single_root (Koo et
    al.): A[d][d] = sum_h w(d, h) and the first word's row holds r(.)."""
    W, r = w[1:, 1:], w[1:, 0]
    A = -W.T.copy()
    inner = W.sum(axis=1, dtype=w.dtype)
    A[np.arange(n - 1), np.arange(n - 1)] = inner if single_root else inner + r
    if single_root:
        A[0, :] = r
    return A


def tree_marginals_arrays(probs_head, n_nodes, single_root=True, dtype=np.float64):
    """The host form of ``ggnn_tree_marginals`` (include/ggnn.h): probs_head
    float32 [b, v, o], n_nodes [b].  The potentials are those of
    projective_marginals_arrays; a dependency tree (single_root: one ROOT
    child) weighs the product of its words' potentials and need not be
    projective.  Returns (marg [b, v, o], logz [b], scores int32 [b, v, o],
    status int32 [b], cond [b]) under projective_marginals_arrays' contract
    (status 2: no tree exists, decided by reachability over the allowed arcs;
    also a determinant that is not positive or a ln Z that is not finite).
    cond[g]: the 1-norm condition number of the graph's normalised matrix in
    float64 (1 for n < 3, inf for status 2): an elimination in fp32 is off by
    about n * cond * 2^-24.  Matrix, inverse and determinant in ``dtype``."""
    p, b, v, o, nn = _head_input(probs_head, n_nodes, "probs_head", np.float32, "tree marginals need")
    dt = np.dtype(dtype)
    single_root = bool(single_root)
    marg = p.astype(dt)
    logz = np.zeros(b, dt)
    scores = np.full((b, v, o), TREE_FORBIDDEN, np.int32)
    status = np.zeros(b, np.int32)
    cond = np.ones(b, np.float64)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        w, ok, ln_c = _normalised_potentials(p[g], n, dt)
        status[g], logz[g], cond[g] = 2, -np.inf, np.inf
        if not _has_tree(ok, n, single_root):
            continue
        A = _laplacian(w, n, single_root)
        try:
            sign, ln_det = np.linalg.slogdet(A)
            B = np.linalg.inv(A)
        except np.linalg.LinAlgError:
            continue
        lz = dt.type(float(ln_det) + ln_c)
        if not (sign > 0 and np.isfinite(lz) and np.isfinite(B).all()):
            continue
        W, r, diag = w[1:, 1:], w[1:, 0], np.diag(B)
        mg = np.zeros((n, n), dt)
        if single_root:
            first = np.arange(n - 1) == 0
            mg[1:, 1:] = np.where(first[:, None], 0, W * diag[:, None]) - np.where(first[None, :], 0, W * B)
            mg[1:, 0] = r * B[:, 0]
        else:
            mg[1:, 1:] = W * (diag[:, None] - B)
            mg[1:, 0] = r * diag
        status[g], logz[g] = 1, lz
        if n >= 3:
            cond[g] = float(np.linalg.cond(_laplacian(_normalised_potentials(p[g], n, np.dtype(np.float64))[0], n,
                                                      single_root), 1))
        else:
            cond[g] = 1.0
        _marginals_out(marg, scores, g, n, ok, np.clip(mg, 0, 1))
    return marg, logz, scores, status, cond


# ------------------------------------------------ tree-structured training loss
# Host form of ``ggnn_tree_loss`` (include/ggnn.h, csrc/k_tree_loss.h): the
# negative log-likelihood of the gold tree under the distribution over trees
# that the head probabilities define (Koo et al. 2007).  Per graph, with p the
# softmax of the head logits z and y the gold heads,
#   L = -sum_d ln p[d][gold_d] + ln Z,    dL/dz[d][k] = marg[d][k] - y[d][k]
# (every word's marginals sum to 1 over its allowed arcs, so the -p[d][k] of the
# first term and the +p[d][k] that ln Z's chain rule leaves cancel).  The first
# term is the heads' cross-entropy; these functions give the second.
TREE_LOSS_FAMILIES = {"nonprojective": 0, "projective": 1}


def _tree_loss_family(family):
    f = TREE_LOSS_FAMILIES.get(family, family)
    if isinstance(f, (bool, str)) or f not in (0, 1):
        raise ValueError("family must be 0 / 'nonprojective' or 1 / 'projective', got %r" % (family,))
    return int(f)


def gold_tree_ok(gold_head, probs_head, n_nodes, family, single_root=True):
    """bool [b]: whether a graph's gold heads have a probability under the
    distribution of ``family`` (the eligibility rule of ggnn_tree_loss).
    gold_head, probs_head: float32 [b, v, o]; n_nodes [b], clipped as the
    kernels clip it.  True when n >= 2 and: every row 1..n-1 of gold_head holds
    exactly one 1.0 and zeros otherwise; that column is an allowed arc (< n,
    not the word itself, its potential finite and > 0); row 0 and the rows >= n
    are all zero; the heads reach node 0 from every word; with single_root
    exactly one word takes column 0; with the projective family no two arcs
    cross (ROOT leftmost)."""
    family = _tree_loss_family(family)
    y = np.asarray(gold_head, np.float32)
    p = np.asarray(probs_head, np.float32)
    if y.ndim != 3 or y.shape != p.shape:
        raise ValueError("gold_head and probs_head must be [b, v, o] alike")
    b, v, o = y.shape
    if v > o or v > TREE_MAXV or o > 1024:
        raise ValueError("the tree loss needs v <= o, v <= %d, o <= 1024 (got v %d, o %d)" % (TREE_MAXV, v, o))
    nn = _node_counts(n_nodes, b, v, o)
    ok = np.zeros(b, bool)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        ones = y[g] == 1
        if not ((ones | (y[g] == 0)).all() and not ones[0].any() and not ones[n:].any()
                and (ones[1:n].sum(axis=1) == 1).all()):
            continue
        heads = np.concatenate([[0], ones[1:n].argmax(axis=1)])
        w = np.arange(1, n)
        if (heads[1:] >= n).any() or (heads[1:] == w).any():
            continue
        pot = p[g, w, heads[1:]]
        if not (np.isfinite(pot) & (pot > 0)).all():
            continue
        if not is_tree(heads, n, bool(single_root)):
            continue
        if family == 1 and not is_projective(heads, n):
            continue
        ok[g] = True
    return ok


def tree_loss_arrays(probs_head, gold_head, n_nodes, family, single_root, target_num, dtype=np.float64):
    """The host form of ``ggnn_tree_loss``: returns (loss_term, marg [b, v, o],
    logz [b], status int32 [b], used int32 [b]).  The graphs that gold_tree_ok
    admits keep their node count, the others get n = 0; the family's
    *_marginals_arrays runs on those counts (so a graph that is not admitted
    has status 0 and marg = a copy of probs_head: the plain cross-entropy and
    its gradient); used = (status == 1) and loss_term = (sum over the used
    graphs of logz) / target_num, what the call adds to head 0's loss.  marg -
    gold_head on a used graph is the gradient of that graph's loss with respect
    to the head logits, times target_num.  Tables / matrices in ``dtype``."""
    family = _tree_loss_family(family)
    p = np.asarray(probs_head, np.float32)
    b, v, o = p.shape
    ok = gold_tree_ok(gold_head, p, n_nodes, family, single_root)
    n_eff = np.where(ok, _node_counts(n_nodes, b, v, o), 0)
    run = projective_marginals_arrays if family == 1 else tree_marginals_arrays
    marg, logz, _, status, _ = run(p, n_eff, single_root, dtype)
    used = (status == 1).astype(np.int32)
    term = float(np.sum(logz[used == 1].astype(np.float64))) / float(target_num)
    return term, marg, logz, status, used


# ------------------------------------------------------- the max-margin loss
# Host form of ``ggnn_margin_loss`` (include/ggnn.h, csrc/k_margin_loss.h): the
# structured hinge loss over cost-augmented decoding (Taskar et al. 2004; the
# objective of MSTParser and of Kiperwasser & Goldberg 2016).  Per graph, with
# p the softmax of the head logits z, y the gold heads and c the margin cost,
#   T* = the best tree of the family under ln p[d][h] + c [h != y_d],
#   l  = sum over the words d with T*_d != y_d of ln p[d][T*_d] - ln p[d][y_d] + c,
#   L  = max(0, l),    dL/dz[d][k] = onehot(T*)[d][k] - y[d][k] where l > 0, else 0
# (every tree has one head per word, so the rows' logsumexp cancels between two
# trees: decoding ln p is decoding the logits, and no softmax term is left in
# the gradient).  T* is found on the integers of tree_scores, so it is the
# maximiser up to their resolution: l may fall short of the true maximum by at
# most 1.5 (n - 1) ln 2 * 2^-k.
MARGIN_LOSS_KINDS = {"nonprojective-margin": 0, "projective-margin": 1}
MARGIN_COST_MAX = 64.0         # keeps |s'| <= 150 * 2^k: the decoders' range rule holds as for tree_scores


def margin_cost(cost):
    """``cost`` as the float32 the library takes, checked: finite, 0 <= cost <= 64."""
    try:
        c = float("nan") if isinstance(cost, (bool, str)) or cost is None else float(np.float32(cost))
    except (TypeError, ValueError):
        c = float("nan")
    if not (np.isfinite(c) and 0.0 <= c <= MARGIN_COST_MAX):
        raise ValueError("the margin cost must be a number in 0..%g, got %r" % (MARGIN_COST_MAX, cost))
    return c


def margin_cost_units(cost, v):
    """C of the cost-augmented scores: rint(cost * 2^k / ln 2), k = tree_score_shift(v)."""
    return int(np.rint(margin_cost(cost) * float(2 ** tree_score_shift(v)) / np.log(2.0)))


def margin_scores(scores, gold_heads, cost, v):
    """s' of one batch: scores int32 [b, v, o] (tree_scores') with C added on
    every allowed arc (d, j) with j != gold_heads[g][d].  gold_heads int [b, v]."""
    s = np.asarray(scores, np.int32)
    y = np.asarray(gold_heads).astype(np.int64)
    j = np.arange(s.shape[2]).reshape(1, 1, -1)
    add = (s != TREE_FORBIDDEN) & (j != y[:, :, None])
    return np.where(add, s.astype(np.int64) + margin_cost_units(cost, v), s).astype(np.int32)


def margin_loss_arrays(probs_head, gold_head, n_nodes, family, single_root, target_num, cost):
    """The host form of ``ggnn_margin_loss``: returns (loss_term, marg float32
    [b, v, o], heads int32 [b, v], value float32 [b], hamming int32 [b], status
    int32 [b], used int32 [b]).  A graph that gold_tree_ok admits is decoded on
    its cost-augmented scores (_max_arborescence / _eisner, always solved);
    status is the decoder's (1 solved, 2 none; 0 for a graph that is not
    admitted), used = admitted and status 1.  For a used graph heads holds T*
    on the words 1..n-1 (-1 elsewhere and on every other graph), hamming the
    words with T*_d != y_d, value max(0, l), and marg onehot(T*) where l > 0, a
    copy of gold_head otherwise; any other graph's marg is a copy of
    probs_head.  loss_term = (sum over the used graphs of max(0, l) + sum_d ln
    p[d][y_d]) / target_num: what the call adds to head 0's loss, the second
    part cancelling the cross-entropy the heads' forward has put there."""
    family = _tree_loss_family(family)
    c = margin_cost(cost)
    p = np.asarray(probs_head, np.float32)
    y = np.asarray(gold_head, np.float32)
    b, v, o = p.shape
    ok = gold_tree_ok(y, p, n_nodes, family, single_root)
    nn = _node_counts(n_nodes, b, v, o)
    gold = np.where((y == 1).any(axis=2), (y == 1).argmax(axis=2), -1)
    s2 = margin_scores(tree_scores(p, nn, v), gold, c, v)
    marg = p.copy()
    heads = np.full((b, v), -1, np.int32)
    value = np.zeros(b, np.float32)
    hamming, status, used = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(b, np.int32)
    total = 0.0
    for g in range(b):
        if not ok[g]:
            continue
        n = int(nn[g])
        if family == 1:
            t = _eisner(s2[g], n, bool(single_root)) if _range_ok(s2[g], n) else None
        else:
            t = _max_arborescence(s2[g], n, bool(single_root))[0]
        if t is None:
            status[g] = 2
            continue
        status[g] = used[g] = 1
        w = np.arange(1, n)
        t, yg = np.asarray(t[1:n], np.int64), gold[g, 1:n]
        heads[g, 1:n] = t
        lp = np.log(p[g].astype(np.float64), where=p[g] > 0, out=np.zeros((v, o)))
        wrong = t != yg
        loss = float((lp[w, t] - lp[w, yg] + c)[wrong].sum())
        hamming[g] = int(wrong.sum())
        value[g] = max(0.0, loss)
        marg[g] = y[g]
        if loss > 0:
            marg[g] = 0
            marg[g, w, t] = 1
        total += max(0.0, loss) + float(lp[w, yg].sum())
    return total / float(target_num), marg, heads, value, hamming, status, used


# ------------------------------------------------ sampling dependency trees
# Host form of ``ggnn_tree_sample`` (include/ggnn.h, csrc/k_tree_sample.h):
# trees drawn from the distribution over ALL dependency trees whose arc
# marginals tree_marginals_arrays gives, by conditional (ancestral) sampling on
# the matrix-tree inverse.  B = inverse of the multi-root matrix A (A[h][d] =
# -w(d, h), A[d][d] = r(d) + sum_h w(d, h)); single_root first draws the one
# ROOT child rho from marg[.][0] among the words with an allowed ROOT arc that
# reach every word, then uses r'(d) = [d == rho] and zeroes rho's word
# potentials.  The words are walked in ascending order; word d takes ROOT with
# mass r'(d) B[d][d] and word h with mass w(d, h) (B[d][d] - B[d][h]) (0 for an
# arc that is not allowed and for an h whose chain of fixed heads ends in d),
# and the drawn head h* is conditioned on by the Sherman-Morrison update
#   B <- B - cvec (x) B[d, :] / den,  cvec = B[:, d] - e_d - [h* > 0] B[:, h*],
#                                     den = B[d][d] - [h* > 0] B[d][h*].
SAMPLE_LDS_MAXN = 199          # GGNN_SAMPLE_LDS_MAXN
SAMPLE_MAX = 4096              # GGNN_SAMPLE_MAX
SAMPLE_STREAM = 0x40000000     # the last Philox counter word of every draw


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) on Python integers: counter four and
    key two 32-bit words; returns the four output words."""
    c = [int(x) & 0xFFFFFFFF for x in counter]
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


def sample_uniform(seed, g, s, d):
    """The uniform of word d's draw (d = 0: the ROOT child's) in sample s of
    graph g: the top 24 bits of Philox word x at counter (d, s, g, 0x40000000)
    under the 64-bit seed as key, times 2^-24 (exact in fp32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((d, s, g, SAMPLE_STREAM), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (x >> 8) * 2.0 ** -24


def _sample_pick(q, u, dt, forced=None):
    """One draw over the masses q (>= 0, ascending column order) in dt: the
    smallest j with q[j] > 0 and c[j] > u * S (c the inclusive prefix sums, S
    their last), the largest j with q[j] > 0 if rounding leaves none.  Returns
    (j, prob, margin); j = -1 when S is not > 0.  With ``forced`` that column
    is taken (prob 0 where its mass is 0 or it is out of range)."""
    c = np.cumsum(q, dtype=dt)
    total = c[-1]
    if not total > 0:
        return -1, 0.0, np.inf
    if forced is not None:
        j = int(forced)
        ok = 0 <= j < len(q) and q[j] > 0
        return j, (float(q[j]) / float(total) if ok else 0.0), np.inf
    pos = q > 0
    hit = np.nonzero(pos & (c > dt.type(u) * total))[0]
    live = np.nonzero(pos)[0]
    j = int(hit[0]) if hit.size else int(live[-1])
    margin = np.inf
    if j != live[0]:
        margin = min(margin, abs(u - float(c[j - 1]) / float(total)))
    if j != live[-1]:
        margin = min(margin, abs(float(c[j]) / float(total) - u))
    return j, float(q[j]) / float(total), margin


def tree_sample_arrays(probs_head, n_nodes, num_samples, seed, single_root=True, dtype=np.float64, forced=None):
    """The host form of ``ggnn_tree_sample`` (include/ggnn.h): num_samples
    dependency trees per graph, drawn from the distribution that
    tree_marginals_arrays(probs_head, n_nodes, single_root) describes.
    Returns (heads int32 [b, K, v], log_prob [b, K], status int32 [b, K],
    margin float64 [b, K]).  heads: the head of word i; -1 on row 0, the rows >=
    n and where status != 1.  log_prob: sum_d ln p[d][head_d] - ln Z in
    float64, -inf where status != 1.  status: 1 drawn; the marginals' status (0
    n < 2, 2 no tree) where that is not 1; 2 on a numerical dead end (a draw
    whose masses do not sum to > 0, an update whose denominator is not finite
    and positive).  margin: the smallest distance, over the sample's draws,
    from u to the nearer end of the chosen head's interval of the CDF (the ends
    at 0 and 1 do not count; inf without one): a form in another precision may
    draw another tree only where this is small.  Sample s of graph g depends
    on (seed, g, s) alone.  ``forced``: heads [b, v] or [b, K, v] to follow in
    place of the draws; log_prob is then the sum of the logs of the
    conditional probabilities met (-inf where one is 0: not a tree of the
    distribution) and heads returns them.  Matrix and updates in ``dtype``."""
    # (the shape rule in the words of tree_marginals_arrays, which runs below)
    p, b, v, o, nn = _head_input(probs_head, n_nodes, "probs_head", np.float32, "tree marginals need")
    K = _count_in_range("num_samples", num_samples, SAMPLE_MAX)
    dt = np.dtype(dtype)
    single_root = bool(single_root)
    marg, logz, _, m_status, _ = tree_marginals_arrays(p, n_nodes, single_root, dt)
    if forced is not None:
        forced = np.asarray(forced, np.int64)
        if forced.ndim == 2:
            forced = np.repeat(forced[:, None, :], K, axis=1)
        if forced.shape != (b, K, v):
            raise ValueError("forced must be [b, v] or [b, num_samples, v]")
    heads = np.full((b, K, v), -1, np.int32)
    log_prob = np.full((b, K), -np.inf, np.float64)
    status = np.repeat(m_status[:, None], K, axis=1).astype(np.int32)
    margin = np.full((b, K), np.inf, np.float64)
    for g in range(b):
        n = int(nn[g])
        if m_status[g] != 1:
            continue
        w, ok, _ = _normalised_potentials(p[g], n, dt)
        m = n - 1
        roots = np.zeros(n, dt)
        if single_root:
            reach = _reach(ok, n)
            cand = np.zeros(n, bool)
            cand[1:] = ok[1:, 0] & reach[1:, 1:].all(axis=1)
            mg = marg[g, :n, 0].astype(dt)
            roots = np.where(cand & (mg > 0), mg, 0).astype(dt)
        inverses = {}
        ln_p = np.log(np.where(ok, p[g, :n, :n], 1).astype(np.float64))
        for s in range(K):
            f = None if forced is None else forced[g, s]
            lp, mar, rho, dead = 0.0, np.inf, 0, False
            if single_root:
                want = None
                if f is not None:
                    took = [d for d in range(1, n) if f[d] == 0]
                    want = took[0] if took else -1
                rho, pr, mr = _sample_pick(roots, sample_uniform(seed, g, s, 0), dt, want)
                if rho < 0:
                    status[g, s] = 2
                    continue
                mar = min(mar, mr)
                lp += np.log(pr) if pr > 0 else -np.inf
                if not pr > 0:
                    heads[g, s, 1:n] = f[1:n]
                    continue
            if rho not in inverses:
                W, r = w[1:, 1:].copy(), w[1:, 0].copy()
                if single_root:
                    r[:] = 0
                    r[rho - 1] = 1
                    W[rho - 1, :] = 0
                A = -W.T.copy()
                A[np.arange(m), np.arange(m)] = W.sum(axis=1, dtype=dt) + r
                inverses[rho] = (W, r, np.linalg.inv(A).astype(dt))
            W, r, B = inverses[rho]
            B = B.copy()
            top = np.arange(n)
            top[rho] = 0                                              # (rho = 0 without single_root: ROOT itself)
            out = np.full(n, -1, np.int64)
            if rho:
                out[rho] = 0
            for d in range(1, n):
                if d == rho:
                    continue
                dp = d - 1
                bdd = B[dp, dp]
                q = np.zeros(n, dt)
                q[0] = r[dp] * bdd
                q[1:] = W[dp, :] * (bdd - B[dp, :])
                q[top == d] = 0                                       # h's fixed chain ends in d: a cycle
                q = np.where(q > 0, q, 0).astype(dt)
                h, pr, mr = _sample_pick(q, sample_uniform(seed, g, s, d), dt, None if f is None else f[d])
                if h < 0:
                    dead = True
                    break
                mar = min(mar, mr)
                if not pr > 0:                                        # (forced only)
                    lp = -np.inf
                    break
                lp += np.log(pr)
                out[d] = h
                den = bdd - (B[dp, h - 1] if h > 0 else 0)
                if not (np.isfinite(den) and den > 0):
                    dead = True
                    break
                cvec = B[:, dp].copy()
                cvec[dp] -= 1
                if h > 0:
                    cvec -= B[:, h - 1]
                B -= np.outer(cvec, B[dp, :] / den)
                top[top == d] = top[h] if h > 0 else 0
            if dead:
                status[g, s] = 2
                continue
            margin[g, s] = mar
            if f is not None:
                heads[g, s, 1:n] = f[1:n]
                log_prob[g, s] = lp
            else:
                heads[g, s, 1:n] = out[1:]
                log_prob[g, s] = float(np.sum(ln_p[np.arange(1, n), out[1:]])) - float(logz[g])
    return heads, log_prob, status, margin


# ------------------------------------------------ sampling projective trees
# Host form of ``ggnn_projective_sample`` (include/ggnn.h,
# csrc/k_proj_sample.h): a top-down walk over _inside's tables.  An item (kind,
# s, t) stands for one table entry and is expanded by one draw over its terms,
# in ascending r:
#   0  ROOT's child (single_root)   r = 0..m-1   CL[0][r] + CR[r][m-1] + psi(r+1 takes ROOT)
#   1  CR[s][t], s < t              r = s+1..t   IR[s][r] + CR[r][t]
#   2  CL[s][t], s < t              r = s..t-1   CL[s][r] + IL[r][t]
#   3  IR[s][t]  (t takes s)        r = s..t-1   CR[s][r] + CL[r+1][t]
#   4  IL[s][t]  (s takes t)        as kind 3
# with masses exp(term - largest term); the chosen term's two entries are the
# item's children (a complete span s = t is a leaf).  Every projective tree has
# exactly one derivation, and the product of its draws' probabilities is its
# weight / Z.
PROJ_SAMPLE_LDS_MAXN = 128     # GGNN_PROJ_SAMPLE_LDS_MAXN
PROJ_SAMPLE_CHUNK = 16         # GGNN_PROJ_SAMPLE_CHUNK
PROJ_SAMPLE_STREAM = 0x50000000    # the last Philox counter word of every draw


def projective_sample_uniform(seed, g, s, kind, a, t):
    """The uniform of item (kind, a, t)'s draw in sample s of graph g: the top
    24 bits of Philox word x at counter (kind << 16 | a << 8 | t, s, g,
    0x50000000) under the 64-bit seed as key, times 2^-24."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((kind << 16 | a << 8 | t, s, g, PROJ_SAMPLE_STREAM), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (x >> 8) * 2.0 ** -24


def _forced_split(kind, s, t, hp, m):
    """The r that the derivation of the heads hp (by position, -1: ROOT or
    none) takes at item (kind, s, t); -1 when there is none."""
    def under(d, x):                                    # d is x or a descendant of x
        for _ in range(m + 1):
            if d == x:
                return True
            if not 0 <= d < m:
                return False
            d = hp[d]
        return False
    if kind == 1:
        return max([d for d in range(s + 1, t + 1) if hp[d] == s], default=-1)
    if kind == 2:
        return min([d for d in range(s, t) if hp[d] == t], default=-1)
    if kind == 3:
        return min(d for d in range(s + 1, t + 1) if under(d, t)) - 1
    return max(d for d in range(s, t) if under(d, s))


def _projective_walk(tables, root, m, lo, dt, uniform, f):
    """One sample: (heads by node [lo + m] or None on a dead end, the sum of
    the logs of the draws' probabilities, margin).  f: heads by node to
    follow, or None."""
    CR, CL, IR, IL = tables
    out = np.full(lo + m, -1, np.int64)
    hp = None
    if f is not None:                                   # by position; ROOT (single_root) and junk: -1
        hp = [int(f[lo + d]) - lo if lo <= f[lo + d] < lo + m else -1 for d in range(m)]
    stack = [(0, 0, 0)] if lo else ([(1, 0, m - 1)] if m > 1 else [])
    lp, mar = 0.0, np.inf
    while stack:
        kind, s, t = stack.pop()
        if kind == 0:
            r = np.arange(m)
            terms = CL[r, 0] + CR[m - 1 - r, r] + root
        elif kind == 1:
            r = np.arange(s + 1, t + 1)
            terms = IR[r - s, s] + CR[t - r, r]
        elif kind == 2:
            r = np.arange(s, t)
            terms = CL[r - s, s] + IL[t - r, r]
        else:
            r = np.arange(s, t)
            terms = CR[r - s, s] + CL[t - r - 1, r + 1]
        top = terms.max()
        if top == -np.inf:
            return None, lp, mar
        q = np.where(terms == -np.inf, 0, np.exp(terms - top)).astype(dt)
        want = None
        if f is not None:
            if kind == 0:
                took = [d for d in range(m) if f[lo + d] == 0]
                want = took[0] if len(took) == 1 else -1
            else:
                want = _forced_split(kind, s, t, hp, m) - int(r[0])
        j, pr, mr = _sample_pick(q, uniform(kind, s, t), dt, want)
        if j < 0:
            return None, lp, mar
        mar = min(mar, mr)
        if not pr > 0:                                  # (forced only)
            return out, -np.inf, mar
        lp += np.log(pr)
        r = int(r[j])
        if kind == 0:
            out[lo + r] = 0
            kids = [(2, 0, r), (1, r, m - 1)]
        elif kind == 1:
            kids = [(3, s, r), (1, r, t)]
        elif kind == 2:
            kids = [(2, s, r), (4, r, t)]
        else:
            if kind == 3:
                out[lo + t] = lo + s
            else:
                out[lo + s] = lo + t
            kids = [(1, s, r), (2, r + 1, t)]
        stack += [k for k in kids if k[1] < k[2]]
    return out, lp, mar


def projective_sample_arrays(probs_head, n_nodes, num_samples, seed, single_root=True, dtype=np.float64, forced=None):
    """The host form of ``ggnn_projective_sample`` (include/ggnn.h):
    num_samples projective dependency trees per graph, drawn from the
    distribution that projective_marginals_arrays(probs_head, n_nodes,
    single_root) describes.  Returns (heads int32 [b, K, v], log_prob [b, K],
    status int32 [b, K], margin float64 [b, K], logz [b]).  heads, log_prob and
    margin: as tree_sample_arrays'.  status: 1 drawn, 0 n < 2, 2 no projective
    tree or a dead end (a draw whose masses do not sum to > 0).  logz: as
    projective_marginals_arrays'.  Sample s of graph g depends on (seed, g, s)
    alone.  ``forced``: heads [b, v] or [b, K, v] to follow in place of the
    draws; log_prob is then the sum of the logs of the conditional
    probabilities met (-inf for a head vector that is no projective tree of
    the distribution) and heads returns them.  Tables in ``dtype``."""
    p, b, v, o, nn = _head_input(probs_head, n_nodes, "probs_head", np.float32, "projective sampling needs")
    K = _count_in_range("num_samples", num_samples, SAMPLE_MAX)
    dt = np.dtype(dtype)
    single_root = bool(single_root)
    lo = 1 if single_root else 0
    if forced is not None:
        forced = np.asarray(forced, np.int64)
        if forced.ndim == 2:
            forced = np.repeat(forced[:, None, :], K, axis=1)
        if forced.shape != (b, K, v):
            raise ValueError("forced must be [b, v] or [b, num_samples, v]")
    heads = np.full((b, K, v), -1, np.int32)
    log_prob = np.full((b, K), -np.inf, np.float64)
    status = np.zeros((b, K), np.int32)
    margin = np.full((b, K), np.inf, np.float64)
    logz = np.zeros(b, dt)
    for g in range(b):
        n = int(nn[g])
        if n < 2:
            continue
        psi, ok = _arc_log_potentials(p[g], n, dt)
        tables, lz, _, root = _inside(psi, n, single_root)
        logz[g] = lz
        if not np.isfinite(lz):
            status[g] = 2
            continue
        ln_p = np.log(np.where(ok, p[g, :n, :n], 1).astype(np.float64))
        for s in range(K):
            f = None if forced is None else forced[g, s]
            out, lp, mar = _projective_walk(tables, root, n - lo, lo, dt,
                                            lambda kind, a, t: projective_sample_uniform(seed, g, s, kind, a, t), f)
            if out is None:
                status[g, s] = 2
                continue
            status[g, s] = 1
            margin[g, s] = mar
            if f is not None:
                heads[g, s, 1:n] = f[1:n]
                log_prob[g, s] = lp if np.array_equal(out[1:], f[1:n]) else -np.inf
            else:
                heads[g, s, 1:n] = out[1:]
                log_prob[g, s] = float(np.sum(ln_p[np.arange(1, n), out[1:]])) - float(lz)
    return heads, log_prob, status, margin, logz
