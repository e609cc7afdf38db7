"""What tests/test_tree_sample.py and tests/test_gpu_tree_sample.py share: the
inputs (the table of test_tree_marginals.reference over ALL_LAUNCHES:
GGNN_SAMPLE_LDS_MAXN equals GGNN_LAPL_LDS_MAXN, so its launches around L
already put L - 1, L and L + 1 nodes in one grid), the float64 host samples of
every launch (computed once, left unchanged), the checks of a batch of samples
and the rule that explains a differing sample.

A sampler in another precision may return another tree than the float64 host
form only where a draw's u lies within the error of the CDF it is compared
with: a sample is EXPLAINED when its float64 margin (the smallest distance,
over its draws, from u to the nearer end of the chosen head's CDF interval) is
below lapl_bar(n, cond) = n * cond * 2^-24, the bar of test_tree_marginals.py
on a marginal (the masses are marginals of the conditioned distribution)."""
import numpy as np

from ggnn_amd import evaluation as E
from ggnn_amd._lib import LAPL_LDS_MAXN, SAMPLE_LDS_MAXN
from test_tree_marginals import ALL_LAUNCHES, lapl_bar, launch_ids, reference  # noqa: F401  (re-exported)

assert SAMPLE_LDS_MAXN == LAPL_LDS_MAXN == E.SAMPLE_LDS_MAXN      # else: launches around SAMPLE_LDS_MAXN are due here
K = 4
SEED = 0x5EED0000C0FFEE                                          # (both key words non-zero)
DIFFER_SHARE = 0.02

# Random123's known-answer vectors of philox4x32_10 (kat_vectors): counter, key, output
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

_SAMPLES = {}


def sample_reference(shape, k, single_root):
    """(heads, log_prob, status, margin) of the float64 host form for one
    launch of the table, K samples per graph under SEED."""
    key = (shape, k, bool(single_root))
    if key not in _SAMPLES:
        p, n = reference(shape, k)[:2]
        out = E.tree_sample_arrays(p, n, K, SEED, single_root)
        for a in out:
            a.setflags(write=False)
        _SAMPLES[key] = out
    return _SAMPLES[key]


def check_samples(p, n, allowed, m_status, single_root, heads, log_prob, status):
    """The contract of a batch of samples [b, K', v]: the statuses (1, or the
    marginals' where that is not 1, or 2), every status-1 sample a dependency
    tree over allowed arcs with the right number of ROOT children, -1 and -inf
    exactly where the contract says."""
    b, ks, v = heads.shape
    assert log_prob.shape == (b, ks) and status.shape == (b, ks)
    rows = np.arange(v)
    for g in range(b):
        m = min(max(int(n[g]), 0), v)
        for s in range(ks):
            h = heads[g, s]
            if m_status[g] != 1:
                assert status[g, s] == m_status[g], (g, s)
            assert status[g, s] in (1, 2) or (status[g, s] == 0 and m < 2), (g, s)
            if status[g, s] != 1:
                assert (h == -1).all() and log_prob[g, s] == -np.inf, (g, s)
                continue
            assert (h[rows >= m] == -1).all() and h[0] == -1, (g, s)
            assert E.is_tree(h, m, single_root), (g, s, h[:m])
            assert allowed[g, np.arange(1, m), h[1:m]].all(), (g, s)      # (a NaN, a zero: never an arc)
            assert np.isfinite(log_prob[g, s]), (g, s)


def differing(ref_heads, heads, status):
    """[b, K] bool: the status-1 samples whose heads are not the reference's."""
    return (np.asarray(ref_heads) != np.asarray(heads)).any(axis=2) & (np.asarray(status) == 1)


def unexplained(diff, margin, n, cond):
    """The differing samples that the rule above does not explain, as (graph,
    sample, margin, bar)."""
    out = []
    for g, s in np.argwhere(diff):
        bar = lapl_bar(int(n[g]), float(cond[g]))
        if not margin[g, s] < bar:
            out.append((int(g), int(s), float(margin[g, s]), bar))
    return out
