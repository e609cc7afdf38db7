"""What the tree-structured loss tests share (test_tree_loss.py on the host,
test_gpu_tree_loss.py on the GPU): the probabilities, the gold trees, the
batches of the ABI test with their float64 host results, and the real dev
model.  Imports no GPU.

Probabilities are the softmax of N(0, 2^2) logits over all o columns (every
row of the [b, v, o] array, the padding rows included), seeds 0..2.  With the
float64 host form every such graph at n = 9, 33, 65, 129 and 200 has status 1
in both root modes, a condition number of at most 426 and n * cond * 2^-24 <=
5.1e-3, inside the 2^-6 cap of the matrix-tree tests: no case is left out and
the tests allow none.  The gold tree is the chain i -> i - 1: projective and
single-rooted, so it is eligible under both families and both root modes.
"""
import functools
import json
import os

import numpy as np

from ggnn_amd import evaluation as E

SEEDS = (0, 1, 2)
SPECIALS = ("n=1", "gold cycle", "infeasible")
# (b, v, o) per family; the last shape of each crosses the family's workspace tier (199 / 107 nodes)
SHAPES = {0: [(6, 9, 12), (5, 33, 40), (4, 65, 70), (3, 129, 150), (2, 200, 200)],
          1: [(6, 9, 12), (4, 65, 70), (3, 108, 120)]}


def softmax_probs(b, v, o, seed):
    """float32 [b, v, o]: the softmax of N(0, 2^2) logits; also returns the logits (float64)."""
    z = np.random.default_rng(seed).normal(0.0, 2.0, (b, v, o))
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32), z


def heads_to_gold(heads, v, o):
    """One graph's gold_head [v, o] from heads[1..n-1] (heads[0] ignored)."""
    y = np.zeros((v, o), np.float32)
    for i in range(1, len(heads)):
        y[i, int(heads[i])] = 1.0
    return y


def chain_gold(n, v, o):
    return heads_to_gold([0] + list(range(0, n - 1)), v, o)


def uneven_counts(b, v):
    """b node counts from v down, at least 2: graph 0 is full."""
    step = max(1, v // (2 * b))
    return np.asarray([max(2, v - g * step) for g in range(b)], np.int32)


@functools.lru_cache(maxsize=None)
def abi_batch(family, shape, seed):
    """One launch of the ABI test: (p [B, v, o], y, n [B], kinds) with B = b +
    3: b chain-gold graphs of uneven sizes, then a graph with n = 1, one whose
    gold heads hold a cycle and one without a tree over its allowed arcs (word
    1 has no positive potential; its gold arc has potential 0).  Read-only."""
    b, v, o = shape
    B = b + len(SPECIALS)
    p, _ = softmax_probs(B, v, o, seed)
    n = np.concatenate([uneven_counts(b, v), [1, min(v, 5), min(v, 4)]]).astype(np.int32)
    y = np.zeros((B, v, o), np.float32)
    for g in range(b):
        y[g] = chain_gold(int(n[g]), v, o)
    cyc = [0] + list(range(0, int(n[b + 1]) - 1))
    cyc[1], cyc[2] = 2, 1
    y[b + 1] = heads_to_gold(cyc, v, o)
    y[b + 2] = chain_gold(int(n[b + 2]), v, o)
    p[b + 2, 1, :] = 0.0
    for a in (p, y, n):
        a.setflags(write=False)
    return p, y, n, ["chain"] * b + list(SPECIALS)


def target_num_of(y):
    """The btb normaliser of a batch: the number of gold heads + SMALL_NUMBER."""
    return float(np.asarray(y, np.float64).sum() + 1e-7)


@functools.lru_cache(maxsize=None)
def abi_reference(family, shape, seed, single_root):
    """The float64 host result of abi_batch: dict(term, marg, logz, status,
    used, bar [B]: the family's error bar of a marginal per used graph (n *
    cond * 2^-24 of the matrix-tree tests, 4 n (log2 n + 4 + span_max) 2^-24
    of the projective ones), tn).  Computed once, left unchanged."""
    p, y, n, _ = abi_batch(family, shape, seed)
    tn = target_num_of(y)
    term, marg, logz, status, used = E.tree_loss_arrays(p, y, n, family, single_root, tn)
    n_eff = np.where(used == 1, n, 0)
    if family == 0:
        m2, z2, _, s2, cond = E.tree_marginals_arrays(p, n_eff, single_root)
        bar = n * cond * 2.0 ** -24
    else:
        m2, z2, _, s2, span = E.projective_marginals_arrays(p, n_eff, single_root)
        bar = 4 * n * (np.log2(np.maximum(n, 1)) + 4 + span) * 2.0 ** -24
    assert np.array_equal(s2, status) and m2.tobytes() == marg.tobytes() and z2.tobytes() == logz.tobytes()
    out = dict(term=term, marg=marg, logz=logz, status=status, used=used, bar=np.where(used == 1, bar, 0.0), tn=tn)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the real dev model
def dev_model(device=None, hidden=128, batch_size=6, **params):
    """test_gpu_heads._dev_model's construction (the 48 real dev sentences of
    tests/golden/batching_golden.npz, every dropout off) with compact feeds, so
    that a step can be captured, and ``params`` on top.  Returns (model, raw
    sentences)."""
    from ggnn_amd.model import DenseGGNNChemModel
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batching_golden.npz"))
    data = json.loads(str(g["raw_json"]))
    vocab = 1 + max(max(d["words_index"]) for d in data)
    ps = {"hidden_size": hidden, "num_timesteps": 2, "batch_size": batch_size, "learning_rate": 0.003,
          "graph_state_dropout_keep_prob": 1.0, "emb_dropout_keep_prob": 1.0, "out_layer_dropout_keep_prob": 1.0,
          "compact_adjacency": True}
    ps.update(params)
    m = DenseGGNNChemModel(params=ps, num_edge_types=int(g["num_edge_types"]),
                           output_size_edges=int(g["output_size_edges"]), pos_size=int(g["pos_size"]),
                           bucket_max_nodes=int(g["bucket_max_nodes"]), precision="fp32", vocab_size=vocab,
                           embedding_sizes=dict(loc=16, pos=8, word=16, edge=8), device=device)
    return m, data


def dev_feeds(m, data, count=30):
    return list(m.make_minibatch_iterator(m.process_raw_graphs(data[:count], True), True))
