"""What tests/test_projective_sample.py and tests/test_gpu_projective_sample.py
share: the inputs (a table built as test_gpu_projective_marginals._reference
builds its own, around GGNN_PROJ_SAMPLE_LDS_MAXN in that suite's
GGNN_MARG_LDS_MAXN's place), the float64 host samples of every launch
(computed once, left unchanged), the checks of a batch of samples and the rule
that explains a differing sample.

A sampler in another precision may return another tree than the float64 host
form only where a draw's u lies within the error of the CDF it is compared
with: a sample is EXPLAINED when its float64 margin (the smallest distance,
over its draws, from u to the nearer end of the chosen term's CDF interval) is
below marg_bar(n, span_max) of test_projective_marginals.py.  A term is the
sum of two inside entries, each within marg_bar / 4 (the bound the marginals
suite holds ln Z to); c_r / S is a ratio of sums of exp of such terms, hence
off by at most marg_bar."""
import numpy as np

import tree_sample_cases as TS
from ggnn_amd import evaluation as E
from ggnn_amd._lib import PROJ_SAMPLE_CHUNK as CHUNK  # noqa: F401  (re-exported)
from ggnn_amd._lib import PROJ_SAMPLE_LDS_MAXN as P
from test_projective_decode import only_crossing_tree
from test_projective_marginals import marg_bar, probs_of_scores, random_probs
from test_tree_decode import F, closed_group, forbidden_row

K = 4
SEED = 0x5EED0000C0FFEE                                          # (both key words non-zero)
DIFFER_SHARE = 0.02

SHAPES = [(4, 4, 150),                       # the smallest bucket
          (3, 8, 8),                         # v = o
          (2, 64, 64),                       # exact wave width: the one-segment draw's last size
          (2, 65, 150),                      # one past it: the four-segment draw
          (3, P, max(P, 150)),               # the largest graphs with tables in LDS
          (3, P + 1, max(P + 1, 150)),       # both storage tiers in one grid
          (5, P + 1, max(P + 1, 150)),       # n = P - 1, P, P + 1 and 5 in one grid (one launch)
          (1, 198, 198),                     # the largest reference bucket
          (1, 256, 256)]                     # GGNN_TREE_MAXV
KINDS = ("flat", "sparse", "peaked", "tiny")


def _node_counts(v):
    """2, an interior value and v; around P also P - 1, P and one short
    graph."""
    out = [v, 5] if v == P + 1 else [v]      # (first: n = P + 1 and n = 5 share a launch)
    out += [2, max(2, min(v - 1, v // 2 + 1))]
    if v in (P, P + 1):
        out += [x for x in (P - 1, P) if x < v]
    return list(dict.fromkeys(out))


def launches(shape):
    """The launches of a shape as lists of b (n, kind): every node count with
    every kind of input; graph 1 of every launch (b = 1: launches of their
    own) has no projective tree."""
    b, v, o = shape
    if b == 5:
        return [[(P - 1, "flat"), (P, "infeasible"), (P, "sparse"), (P + 1, "peaked"), (5, "tiny")]]
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
_SAMPLES = {}


def reference(shape, k):
    """One launch's input and the float64 host marginals (single_root False /
    True: marg, logz, scores, status, span_max), computed once and left
    unchanged.  Graph 0 carries a NaN in a row < n; rows and columns >= n hold
    values that must never be read as arcs."""
    key = (shape, k)
    if key not in _REFERENCE:
        b, v, o = shape
        part = launches(shape)[k]
        rng = np.random.default_rng(9000 + 100 * v + k)
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


ALL_LAUNCHES = [(shape, k) for shape in SHAPES for k in range(len(launches(shape)))]


def launch_ids(x):
    return "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


def sample_reference(shape, k, single_root):
    """(heads, log_prob, status, margin, logz) of the float64 host form for
    one launch of the table, K samples per graph under SEED."""
    key = (shape, k, bool(single_root))
    if key not in _SAMPLES:
        p, n = reference(shape, k)[:2]
        out = E.projective_sample_arrays(p, n, K, SEED, single_root)
        for a in out:
            a.setflags(write=False)
        _SAMPLES[key] = out
    return _SAMPLES[key]


def check_samples(p, n, allowed, m_status, single_root, heads, log_prob, status):
    """tree_sample_cases.check_samples, and every status-1 sample is
    projective."""
    TS.check_samples(p, n, allowed, m_status, single_root, heads, log_prob, status)
    v = heads.shape[2]
    for g, s in np.argwhere(np.asarray(status) == 1):
        m = min(max(int(n[g]), 0), v)
        assert E.is_projective(heads[g, s], m), (g, s, heads[g, s, :m])


differing = TS.differing


def unexplained(diff, margin, n, span_max):
    """The differing samples that the rule above does not explain, as (graph,
    sample, margin, bar)."""
    out = []
    for g, s in np.argwhere(diff):
        bar = marg_bar(int(n[g]), float(span_max[g]))
        if not margin[g, s] < bar:
            out.append((int(g), int(s), float(margin[g, s]), bar))
    return out


def flat_five():
    """The flat 5-node graph of test_gpu_tree_sample.py."""
    rng = np.random.default_rng(77)
    return (0.2 + rng.random((1, 5, 8))).astype(np.float32), np.asarray([5], np.int32)
