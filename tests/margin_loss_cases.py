"""What the max-margin loss tests share (test_margin_loss.py on the host,
test_gpu_margin_loss.py and test_gpu_guard_margin_loss.py on the GPU): the
batches of the ABI test with their host results.  Imports no GPU.

A batch is tree_loss_cases.abi_batch (chain-gold graphs of uneven sizes, then
n = 1, a gold cycle and a graph without a tree) plus three graphs of its own:

  confident      logits + 30 on the gold arcs: T* = y for every cost the tests
                 use, so the graph is used but inactive (l = 0 exactly);
  crossing gold  a gold tree with two crossing arcs: eligible under family 0
                 (all trees) only;
  near ties      every word's gold arc leads one rival by half the cost (by
                 0.1 nats at cost 0) and everything else by 6 nats or more: the
                 cost decides which of the two the decoder takes.

Probabilities are the softmax of N(0, 2^2) logits as in tree_loss_cases.
"""
import functools

import numpy as np

import tree_loss_cases as TL
from ggnn_amd import evaluation as E

SEEDS = (0, 1, 2)
COSTS = (0.0, 1.0, 2.5)
SPECIALS = ("confident", "crossing gold", "near ties")
# (b, v, o) per family: (2, 9, 300) takes the o > 256 template, (2, 200, 200) the largest graphs, (2, 130, 140)
# is above GGNN_PROJ_LDS_MAXN = 128 nodes: the projective decoder's tables are in the workspace
SHAPES = {0: [(6, 9, 12), (4, 65, 70), (2, 9, 300), (2, 200, 200)],
          1: [(6, 9, 12), (4, 65, 70), (2, 130, 140)]}
CROSSING = [0, 0, 4, 1, 1, 4]          # (2, 4) crosses (3, 1); a tree with one ROOT child
ABI_CASES = [(f, s) for f in (0, 1) for s in SHAPES[f]]
ABI_IDS = ["%s-%dx%dx%d" % (("all", "proj")[f], *s) for f, s in ABI_CASES]


def _softmax32(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(family, shape, seed, cost):
    """One launch of the ABI test: (p [B, v, o], y, n [B], kinds) with B = b +
    6: abi_batch's graphs, then the three specials.  Read-only."""
    b, v, o = shape
    p0, y0, n0, kinds = TL.abi_batch(family, shape, seed)
    rng = np.random.default_rng(7000 + seed)
    k = len(SPECIALS)
    p, y = np.zeros((k, v, o), np.float32), np.zeros((k, v, o), np.float32)
    n = np.asarray([min(v, 7), len(CROSSING), min(v, 8)], np.int32)
    # confident
    z = rng.normal(0.0, 2.0, (v, o))
    chain = [0] + list(range(0, int(n[0]) - 1))
    for d in range(1, int(n[0])):
        z[d, chain[d]] += 30.0
    p[0], y[0] = _softmax32(z), TL.heads_to_gold(chain, v, o)
    # crossing gold
    p[1], y[1] = _softmax32(rng.normal(0.0, 2.0, (v, o))), TL.heads_to_gold(CROSSING, v, o)
    # near ties
    z = rng.normal(0.0, 2.0, (v, o))
    chain = [0] + list(range(0, int(n[2]) - 1))
    lead = 0.5 * cost if cost > 0 else 0.1
    for d in range(1, int(n[2])):
        rival = d - 2 if d >= 2 else d + 1
        top = z[d].max() + 6.0
        z[d, chain[d]], z[d, rival] = top + lead, top
    p[2], y[2] = _softmax32(z), TL.heads_to_gold(chain, v, o)
    out = (np.concatenate([p0, p]), np.concatenate([y0, y]), np.concatenate([n0, n]).astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out + (list(kinds) + list(SPECIALS),)


def gold_heads(y):
    """int [b, v]: each row's first 1.0, -1 for a row without one."""
    ones = np.asarray(y) == 1
    return np.where(ones.any(axis=2), ones.argmax(axis=2), -1)


def raw_loss(p, gold, heads, n, cost):
    """l of one graph in float64 from the float32 p [v, o]: the sum over the
    words with heads[d] != gold[d] of ln p[d][heads[d]] - ln p[d][gold[d]] + cost."""
    total = 0.0
    for d in range(1, int(n)):
        if int(heads[d]) != int(gold[d]):
            total += float(np.log(np.float64(p[d, int(heads[d])])) - np.log(np.float64(p[d, int(gold[d])]))) + cost
    return total


@functools.lru_cache(maxsize=None)
def reference(family, shape, seed, single_root, cost):
    """The host result of ``batch``: dict(term, marg, heads, value, hamming,
    status, used, raw [B]: l itself (0 where not used), tn).  Computed once,
    left unchanged."""
    p, y, n, _ = batch(family, shape, seed, cost)
    tn = TL.target_num_of(y)
    term, marg, heads, value, hamming, status, used = E.margin_loss_arrays(p, y, n, family, single_root, tn, cost)
    gold = gold_heads(y)
    c = float(np.float32(cost))
    raw = np.asarray([raw_loss(p[g], gold[g], heads[g], n[g], c) if used[g] else 0.0 for g in range(len(n))])
    out = dict(term=term, marg=marg, heads=heads, value=value, hamming=hamming, status=status, used=used, raw=raw, tn=tn)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def expected_used(family, b):
    """used of a batch: the chains, not abi_batch's three specials, then
    confident, crossing gold (family 0 only) and near ties."""
    return [1] * b + [0] * len(TL.SPECIALS) + [1, 1 if family == 0 else 0, 1]
