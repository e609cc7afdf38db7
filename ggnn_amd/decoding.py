"""Decoding: the chain decode -> marginals -> tree / projective pass ->
confidences -> samples -> k-best, written once against a backend with the
device binding's ten methods (``decode``, ``tree_decode``,
``projective_decode``, ``projective_marginals``, ``tree_marginals``,
``arc_confidence``, ``tree_sample``, ``projective_sample``,
``projective_kbest``, ``tree_kbest``):
heads.OutputHeads on the GPU, ``HostDecoder`` over evaluation.*_arrays for a
model on a CPU device; and the model's decoding entries (``DecodingMixin``)."""
from __future__ import annotations

import numpy as np
import torch

from . import evaluation as _eval
from .heads import tree_scores

KEEP_KEYS = ("out_layer_dropout_keep_prob", "graph_state_keep_prob", "edge_weight_dropout_keep_prob",
             "emb_dropout_keep_prob")
_NO_CONFIDENCE = {      # the projective confidence with tree=True / "mbr", in each entry's words
    "_decode_forward": "confidence: a tree of tree=True may cross, it has no probability under the distribution "
                       "over projective trees; use tree=False, \"projective\" or \"projective-mbr\", or "
                       "confidence=\"nonprojective\"",
    "predict_batch": "predict_batch: confidence needs tree=False, \"projective\" or \"projective-mbr\" "
                     "(a crossing tree has no probability under the projective distribution), or "
                     "confidence=\"nonprojective\"",
    "parse": "parse: confidence needs tree=False, \"projective\" or \"projective-mbr\", or "
             "confidence=\"nonprojective\""}
_MBR_FAMILY = {"projective-mbr": "projective", "mbr": "nonprojective"}     # the marginals an MBR mode is built on
SAMPLE_FAMILIES = ("nonprojective", "projective")                          # the distributions samples are drawn from


def _sample_family(family, keyword="sample_family"):
    """The ``sample_family`` / ``kbest_family`` / ``family`` keyword:
    "nonprojective" (all dependency trees) or "projective"; anything else is a
    ValueError (``keyword`` opens its message)."""
    if isinstance(family, str) and family in SAMPLE_FAMILIES:
        return family
    raise ValueError('%s must be "nonprojective" or "projective", got %r' % (keyword, family))


def _confidence_mode(confidence):
    """The ``confidence`` keyword: False, "projective" (True means it) or
    "nonprojective"; anything else is a ValueError."""
    if isinstance(confidence, (bool, np.bool_)):
        return "projective" if confidence else False
    if isinstance(confidence, str) and confidence in ("projective", "nonprojective"):
        return confidence
    raise ValueError('confidence must be False, True, "projective" or "nonprojective", got %r' % (confidence,))


def _tree_mode(tree, confidence=False, caller=None):
    """The ``tree`` keyword of the decoding entries: False, True,
    "projective", "projective-mbr" or "mbr" (returned as given); anything else
    is a ValueError.  The distribution of ``confidence`` must contain the
    returned tree: the projective one (True) with tree=True or "mbr" is a
    ValueError too (``caller``'s text)."""
    projective_conf = _confidence_mode(confidence) == "projective"
    if isinstance(tree, (bool, np.bool_)):
        if tree and projective_conf:
            raise ValueError(_NO_CONFIDENCE[caller])
        return bool(tree)
    if isinstance(tree, str) and tree in ("projective", "projective-mbr", "mbr"):
        if tree == "mbr" and projective_conf:
            raise ValueError(_NO_CONFIDENCE[caller])
        return tree
    raise ValueError('tree must be False, True, "projective", "projective-mbr" or "mbr", got %r' % (tree,))


def _as_np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _targets_rows(heads_row, labels_row, n):
    """The JSON's 'targets' form [[head, label], ...] of nodes 1..n-1 (the label
    one-based) from a graph's zero-based heads [v] and labels [v]."""
    return [[int(h), int(l) + 1] for h, l in zip(heads_row[1:n], labels_row[1:n])]


def _in_place(host_form):
    """A tree / projective pass with OutputHeads' signature over its host
    form: pred and counts are updated in place (the host form returns copies)."""
    def run(self, scores, n_nodes, pred, gold=None, counts=None, single_root=True):
        new_pred, new_counts, status = host_form(scores, n_nodes, pred, single_root, gold, counts)
        pred[...] = new_pred
        if counts is not None:
            counts[...] = new_counts
        return status
    return run


def _float32_marginals(host_form):
    """A marginals pass with OutputHeads' signature over its host form: marg
    and logz as float32, without the host form's span_max / cond."""
    def run(self, probs_head, n_nodes, single_root=True, with_scores=True):
        marg, logz, scores, status, _ = host_form(probs_head, n_nodes, single_root)
        return marg.astype(np.float32), logz.astype(np.float32), scores if with_scores else None, status
    return run


class HostDecoder:
    """OutputHeads' ten decoding methods over the host forms, numpy in and
    out; the marginals as float32, without the host forms' span_max / cond /
    margin."""
    tree_decode = _in_place(_eval.tree_decode_arrays)
    projective_decode = _in_place(_eval.projective_decode_arrays)
    projective_marginals = _float32_marginals(_eval.projective_marginals_arrays)
    tree_marginals = _float32_marginals(_eval.tree_marginals_arrays)

    def decode(self, probs, n_nodes, labels=None):
        return _eval.decode_arrays(probs[0], probs[1], n_nodes, *(labels or (None, None)))

    def arc_confidence(self, marg, n_nodes, pred):
        return _eval.arc_confidence_arrays(marg, n_nodes, pred)

    def tree_sample(self, probs_head, n_nodes, num_samples, seed=0, single_root=True, marginals=None):
        """(heads int32 [b, K, v], log_prob float32 [b, K], status int32 [b, K])
        of evaluation.tree_sample_arrays (float64; it computes its own
        marginals, ``marginals`` is not read)."""
        heads, log_prob, status, _ = _eval.tree_sample_arrays(probs_head, n_nodes, num_samples, seed, single_root)
        return heads, log_prob.astype(np.float32), status

    def projective_sample(self, probs_head, n_nodes, num_samples, seed=0, single_root=True):
        """(heads int32 [b, K, v], log_prob float32 [b, K], status int32
        [b, K], logz float32 [b]) of evaluation.projective_sample_arrays
        (float64)."""
        heads, log_prob, status, _, logz = _eval.projective_sample_arrays(probs_head, n_nodes, num_samples, seed,
                                                                          single_root)
        return heads, log_prob.astype(np.float32), status, logz.astype(np.float32)

    def projective_kbest(self, scores, n_nodes, K, single_root=True):
        """(heads int32 [b, K, v], totals int32 [b, K], count int32 [b], status
        int32 [b]) of evaluation.projective_kbest_arrays."""
        return _eval.projective_kbest_arrays(scores, n_nodes, K, single_root)

    def tree_kbest(self, scores, n_nodes, K, single_root=True):
        """projective_kbest's four arrays of evaluation.tree_kbest_arrays (the
        K best trees over all dependency trees)."""
        return _eval.tree_kbest_arrays(scores, n_nodes, K, single_root)


def _select(keep, x, fill):
    """x where keep, ``fill`` elsewhere: int32, in x's own array type."""
    if isinstance(x, torch.Tensor):
        return torch.where(keep, x, torch.full_like(x, fill))
    return np.where(keep, x, fill).astype(np.int32)


def decode_chain(backend, probs, probs_e, n_nodes, labels, mode, single_root=True, confidence=False, samples=0,
                 sample_seed=0, sample_family="nonprojective", kbest=0, kbest_family="projective"):
    """The decode and what follows it, in launch order and in ``backend``'s
    array type (probs [b, v, o], probs_e [b, v, oe] float32, n_nodes int32
    [b], labels: the two heads' targets or None).  mode True / "projective":
    the MST / projective pass on tree_scores of probs; "projective-mbr" /
    "mbr": the projective / matrix-tree marginals of probs, the decode again
    with them in probs' place, the projective / MST pass on their integer
    scores; confidence ("projective", which True means, or "nonprojective"):
    that distribution's marginals (unless MBR made them) and the gather of the
    returned heads' marginals come last.  The passes and the marginals see n *
    regular; tree_status is the pass's own where a graph is regular (MBR: and
    has marginals), 2 elsewhere.  samples = K > 0: K trees per graph drawn from
    the distribution over all dependency trees (backend.tree_sample on n *
    regular, with the "mbr" marginals where the chain has them) as
    sampled_heads [b, K, v], sample_log_prob [b, K], sample_status [b, K] (2
    where a graph is not regular); sample_family="projective" draws them from
    the distribution over projective trees instead (backend.projective_sample
    on n * regular, which needs no marginals).  kbest = K > 0: the K best
    projective trees per graph in order (backend.projective_kbest on n *
    regular) of tree_scores of the head PROBABILITIES -- the scores the chain
    built for mode True / "projective", never an MBR mode's marginal scores --
    as kbest_heads [b, K, v], kbest_total [b, K], kbest_count [b] and
    kbest_status [b] (2 where a graph is not regular); kbest = 0 launches
    nothing and adds nothing.  kbest_family="nonprojective": the K best trees
    over ALL dependency trees instead (backend.tree_kbest on the same scores
    and counts; the same keys and fills)."""
    sample_family, kbest_family = _sample_family(sample_family), _sample_family(kbest_family, "kbest_family")
    on_device, family, confidence = isinstance(probs, torch.Tensor), _MBR_FAMILY.get(mode), _confidence_mode(confidence)
    marginals = lambda kind: backend.projective_marginals if kind == "projective" else backend.tree_marginals
    head_scores = lambda: (tree_scores if on_device else _eval.tree_scores)(probs, n_nodes, probs.shape[1])
    pred, gold, counts = backend.decode([probs, probs_e], n_nodes, labels)
    regular = counts[:, 4] == 1
    n_reg = _select(regular, n_nodes, 0) if mode or confidence or samples or kbest else None
    if family:
        marg, logz, scores, has_marg = marginals(family)(probs, n_reg, single_root)
        pred, gold, counts = backend.decode([marg, probs_e], n_nodes, labels)
        regular = regular & (has_marg == 1)
    elif mode:
        scores = head_scores()
    out = {"pred": pred, "gold": gold, "counts": counts, "tree_status": None}
    if mode:
        run = backend.tree_decode if mode in (True, "mbr") else backend.projective_decode
        status = run(scores, n_reg, pred, gold, None if gold is None else counts, single_root)
        out["tree_status"] = _select(regular, status, 2)
    if confidence:
        if family != confidence:     # (nothing reads the integer scores)
            marg, logz, _, _ = marginals(confidence)(probs, n_reg, single_root, with_scores=False)
        out["head_confidence"], out["log_partition"] = backend.arc_confidence(marg, n_nodes, pred), logz
    if samples and sample_family == "projective":
        heads, log_prob, status, _ = backend.projective_sample(probs, n_reg, samples, sample_seed, single_root)
    elif samples:
        have = (marg, logz, scores, has_marg) if family == "nonprojective" else None
        heads, log_prob, status = backend.tree_sample(probs, n_reg, samples, sample_seed, single_root, have)
    if samples:
        out["sampled_heads"], out["sample_log_prob"] = heads, log_prob
        out["sample_status"] = _select(counts[:, 4:5] == 1, status, 2)
    if kbest:
        if family or not mode:       # (the chain's scores are the marginals', or there are none)
            scores = head_scores()
        run = backend.projective_kbest if kbest_family == "projective" else backend.tree_kbest
        out["kbest_heads"], out["kbest_total"], out["kbest_count"], status = run(scores, n_reg, kbest, single_root)
        out["kbest_status"] = _select(counts[:, 4] == 1, status, 2)
    return out


class DecodingMixin:
    """DenseGGNNChemModel's decoding entries (ggnn_heads_decode and after)."""

    def _feed_n_nodes(self, ph):
        """The graphs' node counts of a feed (node_mask_edges row sums /
        output_size_edges) as int32 [b], or None when the feed's masks are not
        of get_mask's closed form (the decode kernel rebuilds them from the
        counts alone)."""
        b, v = int(ph["num_graphs"]), int(ph["num_vertices"])
        o, oe = self.params["output_size"], self.output_size_edges
        if v > o or ph.get("node_mask") is None or ph.get("node_mask_edges") is None:
            return None
        m = np.asarray(ph["node_mask"]).reshape(b, v, o)
        m_e = np.asarray(ph["node_mask_edges"]).reshape(b, v, oe)
        n = np.rint(m_e.sum(axis=(1, 2)) / oe).astype(np.int32)
        ref, ref_e = _eval.closed_form_masks(n, v, o, oe)
        if not (np.array_equal(m, ref) and np.array_equal(m_e, ref_e)):
            return None
        return n

    def _eval_forward(self, feed):
        """The dropout-free forward of a feed (a copy of it with the four keep
        probabilities at 1.0 is staged): through its shape's captured step
        when _graph_ok, else build_loss on the eager path.  Returns the loss."""
        feed = dict(feed)
        feed.update((k, 1.0) for k in KEEP_KEYS)
        with torch.no_grad():
            loss = self._graph_step(feed, False) if self._graph_ok(feed) else None
            if loss is None:
                self.graph_stats["eager"] += 1
                self.feed(feed)
                loss = self.build_loss()
        return loss

    def _decode_forward(self, feed_dict, with_gold, tree=False, single_root=True, confidence=False, samples=0,
                        sample_seed=0, sample_family="nonprojective", kbest=0, kbest_family="projective"):
        """_eval_forward of a feed (default: the staged one), then decode_chain
        eagerly on the same stream (never inside a captured step).  Returns a
        dict: loss (scalar tensor), ph (the staged placeholders), b, v, n_nodes
        (host int32 [b], None: masks not in closed form) and the chain's pred /
        gold / counts / tree_status / head_confidence / log_partition: device
        tensors, numpy arrays on a CPU device (HostDecoder), None without
        n_nodes or where tree / confidence (predict_batch's) do not ask; with
        samples > 0 also sampled_heads / sample_log_prob / sample_status, with
        kbest > 0 also kbest_heads / kbest_total / kbest_count / kbest_status."""
        mode = _tree_mode(tree, confidence, "_decode_forward")
        loss = self._eval_forward(self.placeholders if feed_dict is None else feed_dict)
        ph = dict(self.placeholders)
        b, v = int(ph["num_graphs"]), int(ph["num_vertices"])
        o, oe = self.params["output_size"], self.output_size_edges
        r = {"loss": loss.detach(), "ph": ph, "b": b, "v": v, "pred": None, "gold": None, "counts": None,
             "tree_status": None, "head_confidence": None, "log_partition": None}
        n = r["n_nodes"] = self._feed_n_nodes(ph)
        if n is None:
            return r
        probs = self.ops["computed_values"].detach().reshape(b, v, o).contiguous()
        probs_e = self.ops["computed_values_edges"].detach().reshape(b, v, oe)
        if probs.device.type == "cuda":
            backend, n, labels = self._decode_heads(), self._up_nodes(n, self.device), self._last_labels
        else:
            backend, probs, probs_e = HostDecoder(), probs.numpy(), probs_e.numpy()
            labels = [np.asarray(ph["target_values_head"], np.float32).reshape(b, v, o),
                      np.asarray(ph["target_values_edges"], np.float32).reshape(b, v, oe)] if with_gold else None
        r.update(decode_chain(backend, probs, probs_e, n, labels if with_gold else None, mode, single_root, confidence,
                              samples, sample_seed, sample_family, kbest, kbest_family))
        return r

    def _host_pred(self, ph, b, v):
        """pred [b, v, 2] of the staged batch from its fetched probabilities and
        the feed's own masks (a feed whose masks the decode cannot rebuild)."""
        o, oe = self.params["output_size"], self.output_size_edges
        return _eval.pred_from_masks(self.ops["computed_values"].detach().cpu().numpy(),
                                     self.ops["computed_values_edges"].detach().cpu().numpy(),
                                     np.asarray(ph["node_mask"], np.float32).reshape(b, v, o),
                                     np.asarray(ph["node_mask_edges"], np.float32).reshape(b, v, oe))

    def predict_batch(self, feed_dict=None, tree=False, single_root=True, confidence=False, samples=0, sample_seed=0,
                      sample_family="nonprojective", kbest=0, kbest_family="projective"):
        """The predicted tree of every graph of a batch: {'heads': [b, v],
        'labels': [b, v] (int32 numpy, zero-based columns of the two heads'
        arg-max as adj_mat_to_target(is_probability=True) picks them, -1 = no
        prediction: node 0, padding, an all-zero row), 'n_nodes': [b],
        'sentences_id', 'tree_status'}.  Runs the dropout-free forward and
        decodes on the device; 2 * b * v int32 come back instead of both
        probability arrays.  tree: 'heads' of a graph whose arg-max heads are
        not a dependency tree (single_root: with one ROOT child) hold the
        maximum spanning tree of the head scores instead (ggnn_tree_decode on
        tree_scores of the head probabilities) and 'tree_status' [b] int32
        says 0 = was a tree, 1 = repaired, 2 = no tree exists / not attempted
        (left as the arg-max); None without tree.  tree="projective": 'heads'
        of a graph whose arg-max heads are not a PROJECTIVE dependency tree
        (no two arcs cross, ROOT at the leftmost position) hold the best
        projective tree of the same scores instead (ggnn_projective_decode,
        Eisner's algorithm); the MST pass does not run, and 'tree_status' says
        0 = was a projective tree, 1 = repaired, 2 = no projective tree exists
        / not attempted.  tree="projective-mbr": 'heads' hold the minimum
        Bayes risk projective tree, the one with the most expected-correct
        heads under the distribution over projective trees that the head
        probabilities define (ggnn_projective_marginals, then
        ggnn_projective_decode on the marginals' scores); 'tree_status' says 0
        = the arg-max of the marginals was a projective tree, 1 = replaced by
        the MBR tree, 2 = no projective tree / not attempted (the plain
        arg-max).  tree="mbr": the same over ALL dependency trees, crossing
        arcs included (ggnn_tree_marginals, the matrix-tree theorem, then
        ggnn_tree_decode on the marginals' scores); 'tree_status' says 0 =
        the arg-max of the marginals was a tree, 1 = replaced by the MBR
        tree, 2 = no tree / not attempted.  confidence: the dict gains
        'head_confidence' [b, v] float32, the marginal of every returned head
        (0 where there is no prediction), and 'log_partition' [b], ln Z of
        the distribution: True or "projective": over projective trees (with
        tree False, "projective" or "projective-mbr"; ValueError with
        tree=True or "mbr", whose trees that distribution need not contain);
        "nonprojective": over all dependency trees, with every value of tree
        (with tree="mbr" the marginals are computed once).  tree must be
        False, True, "projective", "projective-mbr" or "mbr".  samples = K > 0:
        the dict gains 'sampled_heads' [b, K, v] int32, K trees per graph drawn
        from the distribution over all dependency trees that the head
        probabilities define (ggnn_tree_sample with seed sample_seed;
        single_root: one ROOT child), -1 on node 0, padding and where the
        status is not 1; 'sample_log_prob' [b, K] float32, ln of each tree's
        probability (-inf where the status is not 1); 'sample_status' [b, K]
        int32: 1 = drawn, 0 = fewer than two nodes, 2 = no tree exists, a
        numerical dead end or not attempted (an irregular graph, a feed whose
        masks are not in closed form).  samples = 0 launches nothing.
        sample_family="projective": the samples are drawn from the
        distribution over PROJECTIVE trees instead (ggnn_projective_sample: the
        distribution of tree="projective-mbr", confidence="projective" and
        structured_loss="projective"; every returned tree is projective and
        'sample_log_prob' is normalised by that distribution's Z); the keys and
        their shapes are the same.  Any other value is a ValueError.
        kbest = K in 1..KBEST_MAX: the dict gains 'kbest_heads' [b, K, v]
        int32, the K best PROJECTIVE trees of every graph, best first
        (ggnn_projective_kbest on tree_scores of the head probabilities,
        whatever ``tree`` is; rank 0 has tree="projective"'s total), -1 on node
        0, padding and the ranks >= 'kbest_count' [b] (the trees returned:
        min(K, number of projective trees)); 'kbest_status' [b] int32: 1 = count
        >= 1, 0 = fewer than two nodes, 2 = no projective tree exists, scores
        out of range or not attempted (an irregular graph, a feed whose masks
        are not in closed form: count 0); 'kbest_log_prob' [b, K] float32 =
        total * ln 2 / 2^k, k = tree_score_shift(v), computed on the host in
        float64 from the integer totals: the ln of the product of the tree's
        head probabilities AT THE RESOLUTION OF THE SCORES (every log2 p
        rounded to 2^-k bits and clamped below at -150; not normalised by any
        Z), -inf on the ranks >= count.  kbest = 0 launches nothing and adds
        nothing; anything outside 0..KBEST_MAX is a ValueError.
        kbest_family="nonprojective": the list is over ALL dependency trees
        instead, crossing arcs included (ggnn_tree_kbest on the same scores:
        the family of tree=True, whose total rank 0 has; 'kbest_count' =
        min(K, number of trees), 'kbest_status' 2 = no tree exists, scores out
        of range or not attempted); the keys, their shapes and fills and the
        'kbest_log_prob' formula are the same.  Any other value is a
        ValueError; without kbest the keyword launches nothing."""
        tree = _tree_mode(tree, confidence, "predict_batch")
        sample_family, kbest_family = _sample_family(sample_family), _sample_family(kbest_family, "kbest_family")
        samples = _eval._count_in_range("samples", samples, _eval.SAMPLE_MAX, 0)
        kbest = _eval._count_in_range("kbest", kbest, _eval.KBEST_MAX, 0)
        r = self._decode_forward(feed_dict, False, tree, single_root, confidence, samples, sample_seed, sample_family,
                                 kbest, kbest_family)
        ph, b, v, pred = r["ph"], r["b"], r["v"], r["pred"]
        if pred is None:
            pred = self._host_pred(ph, b, v)
            n = np.rint(np.asarray(ph["node_mask_edges"]).reshape(b, -1).sum(axis=1)
                        / self.output_size_edges).astype(np.int32)
        else:
            n, pred = r["n_nodes"], _as_np(pred)
        out = {"heads": np.ascontiguousarray(pred[:, :, 0]), "labels": np.ascontiguousarray(pred[:, :, 1]),
               "n_nodes": n, "sentences_id": ph.get("sentences_id"), "tree_status": None}
        # what the chain adds: (the keyword that asks for it, key, shape, dtype, the value where nothing was
        # attempted -- masks not in closed form: no repair, no marginals, no samples, no k-best)
        for asked, key, shape, dtype, fill in ((tree, "tree_status", (b,), np.int32, 2),
                                               (confidence, "head_confidence", (b, v), np.float32, 0),
                                               (confidence, "log_partition", (b,), np.float32, np.nan),
                                               (samples, "sampled_heads", (b, samples, v), np.int32, -1),
                                               (samples, "sample_log_prob", (b, samples), np.float32, -np.inf),
                                               (samples, "sample_status", (b, samples), np.int32, 2),
                                               (kbest, "kbest_heads", (b, kbest, v), np.int32, -1),
                                               (kbest, "kbest_count", (b,), np.int32, 0),
                                               (kbest, "kbest_status", (b,), np.int32, 2),
                                               (kbest, "kbest_total", (b, kbest), np.int32, _eval.TREE_FORBIDDEN)):
            if asked:
                out[key] = np.full(shape, fill, dtype) if r.get(key) is None else _as_np(r[key])
        if kbest:
            total = out.pop("kbest_total").astype(np.float64)
            present = np.arange(kbest)[None, :] < out["kbest_count"][:, None]
            scale = np.log(2.0) / 2.0 ** _eval.tree_score_shift(v)
            out["kbest_log_prob"] = np.where(present, total * scale, -np.inf).astype(np.float32)
        return out

    def _predict_raw(self, raw_data, *args, seed=0, **kwargs):
        """predict_batch(feed, *args, **kwargs) over the batches of raw btb
        sentences, as (batch number, result) pairs.  The sentences are copied
        ('targets' may be absent) and carry their input position as 'id', so
        a result's 'sentences_id' index raw_data.  Batch number i draws its
        samples, if any, with sample_seed (seed + i) mod 2^64."""
        raw = [{"targets": [], **d, "id": k} for k, d in enumerate(raw_data)]
        for i, feed in enumerate(self.make_minibatch_iterator(self.process_raw_graphs(raw, False), False)):
            yield i, self.predict_batch(feed, *args, sample_seed=(int(seed) + i) % 2 ** 64, **kwargs)

    def parse_kbest(self, raw_data, k, single_root=True, family="projective"):
        """The k best projective dependency trees of raw btb sentences
        (parse's input), best first (predict_batch(kbest=k)); with
        family="nonprojective" the k best over ALL dependency trees
        (predict_batch(kbest=k, kbest_family="nonprojective"): the first entry
        is parse(tree=True)'s tree where the scores have one best tree).
        Returns (trees,
        log_probs): trees[s] a list of up to k entries in the JSON's 'targets'
        form [[head, label], ...] for nodes 1..n-1 (the label one-based: the
        label head's arg-max, which does not depend on the head), log_probs[s]
        each one's 'kbest_log_prob', aligned and non-increasing.  A sentence
        with fewer than k projective trees yields those it has; a sentence
        process_raw_graphs drops yields []."""
        family = _sample_family(family, "family")
        raw_data = list(raw_data)
        out, log_probs = [[] for _ in raw_data], [[] for _ in raw_data]
        for _, p in self._predict_raw(raw_data, False, single_root, kbest=k, kbest_family=family):
            for g, s in enumerate(p["sentences_id"]):
                for r in range(int(p["kbest_count"][g])):
                    out[s].append(_targets_rows(p["kbest_heads"][g, r], p["labels"][g], int(p["n_nodes"][g])))
                    log_probs[s].append(float(p["kbest_log_prob"][g, r]))
        return out, log_probs

    def sample_trees(self, raw_data, num_samples, single_root=True, seed=0, family="nonprojective"):
        """Dependency trees of raw btb sentences (parse's input) drawn from the
        distribution over all dependency trees that the head probabilities
        define (predict_batch(samples=num_samples)).  Returns (trees,
        log_probs): trees[k] a list of up to num_samples entries in the JSON's
        'targets' form [[head, label], ...] for nodes 1..n-1 (the label
        one-based: the label head's arg-max, which does not depend on the
        head), log_probs[k] the ln of each one's probability, aligned.  A
        sample whose status is not 1 is left out; a sentence
        process_raw_graphs drops yields [].  Batch number i of the iterator
        draws with seed (seed + i) mod 2^64: the same call gives the same
        trees.  family="projective": the trees are drawn from the distribution
        over projective trees (predict_batch(sample_family="projective"))."""
        family = _sample_family(family)
        raw_data = list(raw_data)
        out, log_probs = [[] for _ in raw_data], [[] for _ in raw_data]
        for _, p in self._predict_raw(raw_data, False, single_root, samples=num_samples, sample_family=family,
                                      seed=seed):
            for g, k in enumerate(p["sentences_id"]):
                for s in np.nonzero(p["sample_status"][g] == 1)[0]:
                    out[k].append(_targets_rows(p["sampled_heads"][g, s], p["labels"][g], int(p["n_nodes"][g])))
                    log_probs[k].append(float(p["sample_log_prob"][g, s]))
        return out, log_probs

    def parse(self, raw_data, tree=False, single_root=True, confidence=False):
        """Parse raw btb sentences (the dicts process_raw_graphs accepts;
        'targets' may be absent): one entry per input sentence, in input
        order, in the JSON's own 'targets' form [[head, label], ...] for nodes
        1..n-1 with the label one-based -- what adj_mat_to_target(...,
        is_probability=True) + merge_head_and_edge_graph give for the sentence.
        A sentence process_raw_graphs drops (empty graph) yields [].  tree: as
        predict_batch(tree=True): every sentence for which a dependency tree
        exists comes back as one.  tree="projective": every sentence for which
        a projective dependency tree exists comes back as one (no crossing
        arcs; predict_batch(tree="projective")).  tree="projective-mbr": the
        minimum Bayes risk projective tree, tree="mbr": the minimum Bayes
        risk tree over all dependency trees (predict_batch).  confidence:
        returns (trees, confidences) with confidences[k] a list of floats
        aligned with trees[k], the marginal of each returned head: True or
        "projective" under the distribution over projective trees (ValueError
        with tree=True or "mbr"), "nonprojective" under the one over all
        dependency trees (every value of tree)."""
        tree = _tree_mode(tree, confidence, "parse")
        raw_data = list(raw_data)
        out, conf = [[] for _ in raw_data], [[] for _ in raw_data]
        for _, p in self._predict_raw(raw_data, tree, single_root, confidence):
            for g, (k, heads, labels) in enumerate(zip(p["sentences_id"], p["heads"], p["labels"])):
                rg_h = [[int(x), 1] for x in heads[1:] if x >= 0]
                rg_e = [[0, int(x) + 1] for x in labels[1:] if x >= 0]
                out[k] = _eval.merge_head_and_edge_graph(rg_h, rg_e)
                if confidence:
                    conf[k] = [float(c) for x, c in zip(heads[1:], p["head_confidence"][g, 1:]) if x >= 0]
        return (out, conf) if confidence else out

    def score_epoch(self, data, tree=False, single_root=True):
        """The validation pass of run_epoch with the scoring on the device:
        per batch only the loss and the decode's counts [b, 5] are fetched
        (pred / gold too for a batch with an irregular graph, scored through
        the reference's lists; both probability arrays only for a feed whose
        masks are not in closed form).  One batch in flight and the sums over
        the ranks as in run_epoch.  Returns (loss, las, uas, label_acc,
        instances_per_sec, steps) -- run_epoch's values.  ``decode_stats``
        holds the pass's graphs, host-fallback graphs and fetched bytes.  tree:
        the scores are those of the tree-constrained heads (ggnn_tree_decode
        after the decode, its status [b] fetched beside the counts);
        ``decode_stats`` counts the repaired graphs and those without a tree
        (a graph on the host fallback is scored from its arg-max lists).
        tree="projective": the same with the projective pass
        (ggnn_projective_decode) in the MST pass's place; the same keys count
        the graphs it repaired and those without a projective tree.
        tree="projective-mbr": the MBR chain of predict_batch; the same bytes
        are fetched, 'repaired_graphs' counts the graphs whose marginals'
        arg-max was replaced by the MBR tree.  tree="mbr": the same with the
        chain over all dependency trees (ggnn_tree_marginals, ggnn_tree_decode)."""
        tree = _tree_mode(tree)
        stats = self.decode_stats = {"graphs": 0, "fallback_graphs": 0, "d2h_bytes": 0, "repaired_graphs": 0,
                                     "infeasible_graphs": 0}
        keys = ("counts", "tree_status") if tree else ("counts",)     # what a batch's scoring fetches

        def step(feed, all_reduce):
            r = self._decode_forward(feed, True, tree, single_root)
            r["event"] = None
            if r["counts"] is None:          # the host scorer decides: fetch what it reads
                r["scored"] = self._score_batch()[:3]
                r["host"] = [r["loss"].cpu()]
                stats["d2h_bytes"] += 4 + 4 * r["b"] * r["v"] * (self.params["output_size"] + self.output_size_edges)
                stats["fallback_graphs"] += r["b"]
            elif isinstance(r["counts"], np.ndarray):   # a CPU device: HostDecoder's arrays
                r["host"] = [r["loss"].reshape(1)] + [torch.from_numpy(r[k]) for k in keys]
            else:
                dev = [r["loss"].reshape(1)] + [r[k] for k in keys]
                r["host"], r["event"] = self._fetch_counts.fetch(dev)
                stats["d2h_bytes"] += sum(t.numel() * t.element_size() for t in dev)
            return r

        def consume(r):
            batch_loss = float(r["host"][0].sum())
            if r["counts"] is None:
                scores = r["scored"]
                if tree:
                    stats["infeasible_graphs"] += r["b"]
            else:
                if tree:
                    status = r["host"][2].numpy()
                    stats["repaired_graphs"] += int((status == 1).sum())
                    stats["infeasible_graphs"] += int((status == 2).sum())
                lists = {}

                def fallback(i):
                    if not lists:
                        lists["pred"], lists["gold"] = _as_np(r["pred"]), _as_np(r["gold"])
                        if isinstance(r["pred"], torch.Tensor):
                            stats["d2h_bytes"] += 2 * lists["pred"].nbytes
                    stats["fallback_graphs"] += 1
                    return _eval.graph_scores_from_lists(lists["pred"][i], lists["gold"][i])

                scores = _eval.scores_from_counts(r["host"][1].numpy(), fallback)
            stats["graphs"] += r["b"]
            return (r["b"], batch_loss) + tuple(scores)

        processed, loss, las, uas, uas_e, steps, _, elapsed = self._epoch(data, False, step, consume)
        return loss / processed, las / processed, uas / processed, uas_e / processed, processed / elapsed, steps
