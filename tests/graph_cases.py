"""What the captured-step tests share (test_gpu_graphs.py,
test_gpu_graph_lifecycle.py): the bit-for-bit comparison of a captured model
with its eager twin, and the small synthetic model and batches of the
lifecycle cases.

The twin is built identically with hip_graphs off and fed the same batches: it
draws the same seeds in the same order, and every reduction of the library is
order-fixed, so after every step the two agree in every bit (torch.equal, no
tolerance) on the loss, both probability arrays, the flat gradient buffer,
the Adam slots, the variables and optimizer.t."""
import numpy as np

from decode_cases import _synthetic_model, _torch

# the training feeds' dropouts: all four on, so the three device seeds matter
KEEPS = {"edge_weight_dropout_keep_prob": 0.9, "graph_state_keep_prob": 0.9, "emb_dropout_keep_prob": 0.55,
         "out_layer_dropout_keep_prob": 0.85}
BATCH = 5
# 360 synthetic sentences (seed 2) bucket, in input order, into six full
# batches of 5 x 24 nodes with 111..114 edges (shape A), nine of 5 x 40 (shape
# B) and tails; counted on the host, and asserted again by lifecycle_feeds
N_SENTENCES, TREEBANK_SEED, V_A, V_B = 360, 2, 24, 40

_CACHE = {}


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def assert_same_state(ea, gr, tag):
    """The flat gradient buffer, the Adam slots, the variables and the step
    count of two models, bit for bit."""
    torch = _torch()
    fa, fg = ea.train_buffer().flat, gr.train_buffer().flat
    assert torch.equal(fg, fa), (tag, "gradients", _rel(fg, fa))
    for i, (ma, mb) in enumerate(zip(ea.optimizer.m + ea.optimizer.v, gr.optimizer.m + gr.optimizer.v)):
        assert torch.equal(ma, mb), (tag, "Adam slot", i, _rel(mb, ma))
    for i, (pe, pg) in enumerate(zip(ea.trainable_variables(), gr.trainable_variables())):
        assert torch.equal(pe.detach(), pg.detach()), (tag, "variable", i, _rel(pg.detach(), pe.detach()))
    assert ea.optimizer.t == gr.optimizer.t, (tag, ea.optimizer.t, gr.optimizer.t)


def outputs(m, loss):
    """Clones of a step's loss and both probability arrays (on a captured
    step the originals are the graph's static outputs)."""
    return [loss.detach().clone(), m.ops["computed_values"].detach().clone(),
            m.ops["computed_values_edges"].detach().clone()]


def assert_same_outputs(a, b, tag):
    torch = _torch()
    for name, x, y in zip(("loss", "computed_values", "computed_values_edges"), a, b):
        assert torch.equal(x, y), (tag, name, _rel(y, x))


def train_both(ea, gr, feed, tag, **kw):
    """One train_step of ``feed`` on the eager model and on the captured one:
    the same bits everywhere (same weights, inputs and seeds).  Returns the
    eager step's (loss, probabilities, edge probabilities) clones."""
    torch = _torch()
    oa = outputs(ea, ea.train_step(dict(feed), **kw))
    ob = outputs(gr, gr.train_step(dict(feed), **kw))
    torch.cuda.synchronize()
    assert_same_outputs(oa, ob, tag)
    assert_same_state(ea, gr, tag)
    return oa


def model_pair(hidden=64, **params):
    """(eager, captured): the same model but for params['hip_graphs']."""
    return _synthetic_model(False, hidden, **params), _synthetic_model(True, hidden, **params)


def n_edges(feed) -> int:
    return sum(len(g) for g in feed["adjacency_edges"])


def lifecycle_raw():
    from ggnn_amd.batching import synthetic_treebank
    return synthetic_treebank(N_SENTENCES, num_edge_types=6, output_size_edges=12, pos_size=46, vocab_size=200,
                              max_nodes=40, seed=TREEBANK_SEED)


class Feeds:
    """The lifecycle cases' training feeds, in the treebank's own order (no
    shuffle): A, B: the full batches of the two shapes, tail: a batch of fewer
    graphs.  Read-only: the tests step copies."""

    def __init__(self, m):
        data = m.process_raw_graphs(lifecycle_raw(), False)
        feeds = [dict(f, **KEEPS) for f in m.make_minibatch_iterator(data, False)]
        full = lambda v: [f for f in feeds if f["num_graphs"] == BATCH and f["num_vertices"] == v]
        self.A, self.B = full(V_A), full(V_B)
        tails = [f for f in feeds if f["num_graphs"] < BATCH]
        # the conditions of the fixture, on the host before any GPU work
        assert len(self.A) >= 6 and len(self.B) >= 2 and tails
        counts = [n_edges(f) for f in self.A]
        assert len(set(counts)) >= 4, counts
        for i, f in enumerate(self.A):
            assert n_edges(f) < BATCH * V_A
            for g in self.A[:i]:
                assert not np.array_equal(f["word_inputs"], g["word_inputs"])
        assert not np.array_equal(self.B[0]["word_inputs"], self.B[1]["word_inputs"])
        self.tail = tails[0]
        # four batches of shape A with four edge counts, one with the most
        # edges followed by one with the fewest
        by = {}
        for f in self.A:
            by.setdefault(n_edges(f), f)
        c = sorted(by)
        self.a_max, self.a_min = by[c[-1]], by[c[0]]
        self.A4 = [by[c[1]], self.a_max, self.a_min, by[c[-2]]]


def lifecycle_feeds(m=None) -> Feeds:
    """Built once (batching reads no weight: any of the synthetic models gives
    the same feeds) and shared."""
    if "feeds" not in _CACHE:
        _CACHE["feeds"] = Feeds(m if m is not None else _synthetic_model(False))
    return _CACHE["feeds"]
