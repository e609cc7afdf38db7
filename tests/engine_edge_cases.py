"""Case tables, input builders and float64 references shared by
tests/test_gpu_engine_edges.py (GPU) and tests/test_engine_edge_inputs.py (CPU).

numpy and the oracle only: nothing here touches the GPU.  The tier predicates
restate the dispatch of ggnn_amd/csrc/ggnn_api.hip (make_cfg, fused_fwd, by_gru_rt,
launch_gru_fwd, wg_plan with WgPlan::lists, backward_impl) for the fp32-parity mode,
so the CPU module can assert that the tables reach every tier.
"""
import functools
from collections import namedtuple

import numpy as np

import ggnn_oracle as O

GRADS = ("h0", "edge_weights", "edge_biases", "gates_kernel", "gates_bias", "candidate_kernel", "candidate_bias")
FUSED_MAXT = 16          # k_fused.h
WG_LIST_MAX = 256        # k_wgrad.h

# kind: "dense" = SURVEY §8d synthetic adjacency (every channel given an edge),
# "tree" = dependency trees (graph_to_adj_mat_bd, C = 2E), "empty" = dense with
# graph 0 and the last channel cleared, "edges" = trees staged from edge lists
Case = namedtuple("Case", "name b v h C T ek sk seed kind bias generic")


def _c(name, b, v, h, C, T, ek=1.0, sk=1.0, seed=0, kind="dense", bias=True, generic=False):
    return Case(name, b, v, h, C, T, ek, sk, seed, kind, bias, generic)


# --------------------------------------------------------------- case tables
# Section C of the issue: one row per dispatch tier (the comment names what the
# row reaches; tiers() below recomputes it)
TIER_CASES = [
    _c("n32_c1_t1", 1, 1, 128, 1, 1),               # N = 32, padded, RT = 1, KC = 32 -> k_wgrad<32>, C = 1, v = 1
    _c("dense_t1", 1, 32, 128, 2, 1),               # dense, T = 1: first && last, dhT and dh0 in place
    _c("h256_n64", 2, 32, 256, 3, 2),               # k_gru_fwd<256, 2>, 128-tile wgrad, KC = 64, odd C
    _c("v33", 3, 33, 256, 4, 2),                    # v just over 32, N = 192
    _c("v31", 2, 31, 128, 4, 2),                    # pad boundary below 32
    _c("v64", 2, 64, 128, 4, 2),                    # dense at 64
    _c("v65_fused_b1", 1, 65, 256, 2, 3),           # fused, padded, b = 1
    _c("dense_sd_256", 2, 64, 256, 4, 2, sk=0.8, seed=3),   # dense + state dropout outside the fused forward
    _c("dense_sd_128", 1, 128, 128, 3, 2, sk=0.8, seed=4),  # the same branch at hidden 128
    _c("fused_t1_c1", 1, 128, 256, 1, 1),           # fused, dense, T = 1, C = 1
    _c("fused_t1_c1_sd", 1, 128, 256, 1, 1, sk=0.7, seed=5),  # sbits read by the first and only step
    _c("v127_128", 1, 127, 128, 5, 2),              # v just under 128
    _c("v127_256", 1, 127, 256, 5, 2),
    _c("ed_cpt2", 16, 32, 128, 4, 1, ek=0.7, seed=6),  # edge dropout, cpt = 2 timestep-aligned chunks
    # FUSED_MAXT exactly.  Sixteen steps of the saturated GRU amplify rounding
    # by a factor that depends on the data: the bar (4e-3, test_gpu_parity's
    # rule for T > 8) can only be asked of inputs on which the reference itself
    # is well conditioned.  Rule (MAXT_FP32_REF_ERR): the oracle evaluated in
    # float32 (unit roundoff 2^-24) stays within FP32_TOL / 4 = 2.5e-4 of
    # float64, so the split mode's 2^-22 operands are expected near 1e-3, a
    # quarter of the bar.  Seed 2 is the first case seed that meets it (0:
    # 2.1e-3, 1: 1.2e-3, 2: 6.3e-5; tests/test_engine_edge_inputs.py asserts it)
    _c("fused_maxt", 1, 128, 256, 2, 16, seed=2),
]
MAXT_FP32_REF_ERR = 2.5e-4
# Section A beyond the tier table: both dropouts on padded / fused / unfused
# shapes, the general path, no edge bias
EXTRA_CASES = [
    _c("v33_both", 3, 33, 256, 4, 2, ek=0.8, sk=0.8, seed=7),
    _c("v31_both", 2, 31, 128, 4, 2, ek=0.7, sk=0.8, seed=8),
    _c("v65_fused_both", 2, 65, 256, 2, 3, ek=0.8, sk=0.8, seed=9),
    _c("fused_dense_both", 2, 128, 256, 2, 2, ek=0.8, sk=0.8, seed=10),
    _c("nobias_128", 3, 20, 128, 4, 2, bias=False),
    _c("nobias_256_fused", 1, 100, 256, 3, 2, bias=False),
    _c("gen_h100", 3, 37, 100, 4, 2, generic=True),
    _c("gen_h100_both", 3, 37, 100, 4, 2, ek=0.8, sk=0.8, seed=11, generic=True),
    _c("gen_h128_forced", 2, 33, 128, 4, 2, generic=True),
    _c("gen_h128_forced_both", 2, 33, 128, 4, 2, ek=0.8, sk=0.8, seed=12, generic=True),
]
# skip_empty_channels = False (GGNN_DENSE_CHANNELS) on one shape per V and hidden size
DENSE_CHANNEL_CASES = ["n32_c1_t1", "h256_n64", "v64", "v65_fused_b1", "fused_t1_c1_sd", "ed_cpt2"]
# graph 0 without an edge, channel 5 without an edge in any graph
EMPTY_CASES = [
    _c("empty_n192", 3, 40, 256, 6, 2, kind="empty"),       # N % 128 != 0
    _c("empty_lists", 2, 128, 256, 6, 2, kind="empty"),     # WgPlan::lists
    _c("empty_h128", 3, 20, 128, 6, 2, kind="empty"),       # hidden 128, v -> 32: k_wgrad reads every dM^T row
]
# the 16-bit modes' statistical bars need dependency-tree adjacency
# (test_bf16_within_north_star_on_dependency_trees explains why)
BIT16_CASES = [
    _c("tree_v33", 3, 33, 256, 4, 2, kind="tree"),
    _c("tree_v128", 1, 128, 256, 2, 2, kind="tree"),
]
# pair mode: edge lists, C = 2E = 8
PAIR_CASES = [
    _c("pair_h20", 3, 11, 20, 8, 2, kind="edges"),
    _c("pair_h400", 4, 30, 400, 8, 2, kind="edges"),
    _c("pair_h20_ed", 3, 11, 20, 8, 2, ek=0.7, sk=0.8, seed=13, kind="edges"),
    _c("pair_h400_ed", 4, 30, 400, 8, 2, ek=0.7, sk=0.8, seed=14, kind="edges"),
]
ALL_CASES = {c.name: c for c in TIER_CASES + EXTRA_CASES + EMPTY_CASES + BIT16_CASES + PAIR_CASES}
assert len(ALL_CASES) == len(TIER_CASES + EXTRA_CASES + EMPTY_CASES + BIT16_CASES + PAIR_CASES)


def dropout_of(c):
    """The oracle's dropout dict of a case (None: no dropout)."""
    if c.ek >= 1.0 and c.sk >= 1.0:
        return None
    return dict(edge_keep=c.ek, state_keep=c.sk, seed=0x5EED_0000 + c.seed)


# ------------------------------------------------------------ input builders
def trees(b, v, E, seed):
    rng = np.random.default_rng(seed)
    graphs = []
    for _ in range(b):
        n = int(rng.integers(max(2, v // 2), v + 1))
        graphs.append([(int(rng.integers(0, i)), int(rng.integers(1, E + 1)), i) for i in range(1, n)])
    return graphs


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(A [b, C, v, v] fp32, h0, dhT, w, graphs or None); cached, read-only."""
    c = ALL_CASES[name]
    seed = 1000 + 17 * c.b + c.v + c.h + c.C + c.seed
    graphs = None
    if c.kind in ("tree", "edges"):
        E = c.C // 2
        graphs = trees(c.b, c.v, E, seed)
        A = np.stack([O.graph_to_adj_mat_bd(g, c.v, E, dtype=np.float32) for g in graphs])
        h0 = np.random.default_rng(seed + 1).uniform(-0.2, 0.2, (c.b, c.v, c.h)).astype(np.float32)
    else:
        A, h0 = O.synthetic_batch(c.b, c.v, c.h, c.C, seed=seed, density=0.1)
        A = np.array(A, np.float32)
        nonempty = c.C - 1 if c.kind == "empty" else c.C
        for ch in range(nonempty):      # every channel the case calls non-empty has an edge
            if not A[:, ch].any():
                A[-1, ch, 0, 0] = 1.0
        if c.kind == "empty":
            A[0] = 0.0
            A[:, c.C - 1] = 0.0
    w = O.synthetic_weights(c.h, c.C, seed=seed)
    if not c.bias:
        w["edge_biases"] = np.zeros_like(w["edge_biases"])
    dhT = np.random.default_rng(seed + 2).standard_normal((c.b, c.v, c.h)).astype(np.float32)
    out = dict(A=A, h0=h0, dhT=dhT, w=w)
    for x in (A, h0, dhT) + tuple(w.values()):
        x.setflags(write=False)
    out["graphs"] = graphs
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(h_T, gradients, h_T without dropout or None) of the float64 oracle; cached, read-only."""
    c = ALL_CASES[name]
    x = inputs(name)
    A64, h64 = x["A"].astype(np.float64), x["h0"].astype(np.float64)
    w64 = {k: a.astype(np.float64) for k, a in x["w"].items()}
    dr = dropout_of(c)
    ref, caches = O.forward(A64, h64, w64, c.T, use_edge_bias=c.bias, dropout=dr)
    gref = O.backward(A64, x["dhT"].astype(np.float64), caches, w64, use_edge_bias=c.bias)
    nodrop = None
    if dr is not None:
        nodrop, _ = O.forward(A64, h64, w64, c.T, use_edge_bias=c.bias, keep_cache=False)
        nodrop.setflags(write=False)
    ref.setflags(write=False)
    for g in gref.values():
        g.setflags(write=False)
    return ref, gref, nodrop


def reference_fp32_error(name, seed=None):
    """max |h_T| difference of the oracle evaluated in float32 and in float64:
    the conditioning of a case's data (seed: another case seed's data)."""
    c = ALL_CASES[name]
    if seed is not None:
        s = 1000 + 17 * c.b + c.v + c.h + c.C + seed
        A, h0 = O.synthetic_batch(c.b, c.v, c.h, c.C, seed=s, density=0.1)
        w = O.synthetic_weights(c.h, c.C, seed=s)
    else:
        x = inputs(name)
        A, h0, w = x["A"], x["h0"], x["w"]
    r32, _ = O.forward(A.astype(np.float32), h0.astype(np.float32), w, c.T, use_edge_bias=c.bias, keep_cache=False)
    r64, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), {k: a.astype(np.float64) for k, a in w.items()},
                       c.T, use_edge_bias=c.bias, keep_cache=False)
    return float(np.abs(r32 - r64).max())


# ------------------------------------------------------------ tier predicates
def pad_v(v):
    return 32 if v <= 32 else 64 if v <= 64 else 128 if v <= 128 else -1


def _wg256_kc(N, C):
    KC = 8192
    while KC > 128 and (N % KC != 0 or (6 + C) * (N // KC) < 224):
        KC //= 2
    return KC


def tiers(c, skip=True):
    """The dispatch decisions of the fp32-parity mode for a specialised-path
    case (hidden 128 / 256, v <= 128, not forced generic)."""
    assert c.h in (128, 256) and c.v <= 128 and not c.generic
    V = pad_v(c.v)
    N = c.b * V
    ed, sd = c.ek < 1.0, c.sk < 1.0
    dense = c.v == V
    fused = c.h == 256 and V == 128 and c.T <= FUSED_MAXT
    t32 = N // 32
    rt = 2 if t32 % 2 == 0 else 1                      # kSplitRT = 2 (forward and backward)
    big = c.h == 256 and N % 128 == 0
    tile = 256 if big else 128
    tiles = (6 + c.C) * (c.h // tile) ** 2
    if big:
        KC = _wg256_kc(N, c.C)
    else:
        KC = 4096
        while KC > 32 and N % KC != 0:
            KC //= 2
        while KC > 256 and tiles * (N // KC) < 256:
            KC //= 2
    nchunks = max(N // KC, 1)
    cpt = KCt = 0
    if ed:
        cpt = 1
        while cpt * c.T < nchunks and N % (cpt * 2 * 32) == 0:
            cpt *= 2
        KCt = N // cpt
    lists = (big and skip and (c.b + (cpt if ed else nchunks) - 1) // (cpt if ed else nchunks) <= WG_LIST_MAX
             and V % 32 == 0)
    if fused:
        gru_fwd = "k_fwd_fused"
    elif c.h == 256 and N % 128 == 0:
        gru_fwd = "k_gru_fwd2"
    else:
        gru_fwd = "k_gru_fwd<%d,%d>" % (c.h, rt)
    return dict(V=V, N=N, dense=dense, fused=fused, rt=rt, big=big, KC=KC, kc64=(KC % 64 == 0 and KCt % 64 == 0),
                cpt=cpt, in_place=dense and (not sd or fused), sbits=sd and fused, first_and_last=c.T == 1 and dense
                and (not sd or fused), lists=lists, gru_fwd=gru_fwd, gru_grid=N // (32 * rt), nchunks=nchunks)
