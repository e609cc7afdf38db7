"""The cases of the guard-band tests (tests/test_gpu_guard_*.py) and the byte
counts of their regions, shared with tests/test_guard_arena.py, which asserts
on the CPU that every case gets a size from each *_bytes function the GPU half
uses for it and fits the arena.  numpy, the oracle and libggnn's host-side
entry points only: nothing here touches the GPU.
"""
import functools
from collections import namedtuple

import numpy as np

import engine_edge_cases as EC
import ggnn_oracle as O

CAPACITY = 64 << 20       # of every arena of the GPU half (test_guard_arena asserts that each case fits)

# ------------------------------------------------------------------ engine
# c: an engine_edge_cases.Case; local: not a row of EC.ALL_CASES (inputs built here)
GCase = namedtuple("GCase", "id c precision skip batch_pack local")

RAGGED_HIDDEN = [(2, 40, 65, 2), (2, 20, 3, 2), (1, 12, 1, 1)]     # test_generic_edge_dropout_hidden_not_multiple_of_4


def _local_cases():
    out = []
    for b, v, h, C in RAGGED_HIDDEN:        # the general path's masked copies at hidden % 4 != 0 (copy mode 2)
        out.append(EC.Case("ragged_h%d" % h, b, v, h, C, 2, 0.7, 1.0, 98765 + h, "dense", True, True))
    out.append(EC.Case("v150_dense", 2, 150, 128, 4, 2, 1.0, 1.0, 0, "dense", True, True))
    out.append(EC.Case("v150_pairs", 2, 150, 128, 4, 2, 1.0, 1.0, 0, "edges", True, True))
    # pair mode at its capacity: edges == b * v exactly (trees over all v nodes plus one extra edge per graph)
    out.append(EC.Case("pair_full", 3, 11, 20, 8, 2, 1.0, 1.0, 0, "full", True, True))
    return out


LOCAL = {c.name: c for c in _local_cases()}


def _engine_cases():
    out = []
    for c in EC.TIER_CASES:
        if c.name != "fused_maxt":
            out += [GCase("%s-%s" % (c.name, p), c, p, True, False, False) for p in ("fp32", "fp16", "bf16")]
    for c in EC.EXTRA_CASES + EC.EMPTY_CASES:
        out.append(GCase(c.name, c, "fp32", True, False, False))
    for c in EC.PAIR_CASES:
        out.append(GCase(c.name, c, "fp32", True, False, False))
        if c.ek < 1.0:
            out.append(GCase(c.name + "-batch_pack", c, "fp32", True, True, False))
    for name in EC.DENSE_CHANNEL_CASES:
        out.append(GCase(name + "-dense_channels", EC.ALL_CASES[name], "fp32", False, False, False))
    for c in LOCAL.values():
        out.append(GCase(c.name, c, "fp32", True, False, True))
    return out


ENGINE_CASES = _engine_cases()
ENGINE_IDS = [g.id for g in ENGINE_CASES]
assert len(set(ENGINE_IDS)) == len(ENGINE_IDS)


def dropout_of(c):
    """dict(edge_keep, state_keep, seed) of a case (never None)."""
    if c.name in LOCAL:
        return dict(edge_keep=c.ek, state_keep=c.sk, seed=c.seed)
    return EC.dropout_of(c) or dict(edge_keep=1.0, state_keep=1.0, seed=0)


def _edge_arrays(graphs):
    sizes = [len(g) for g in graphs]
    offs = np.zeros(len(graphs) + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    n = int(offs[-1])
    edges = (np.concatenate([np.asarray(g, np.int32).reshape(-1, 3) for g in graphs if len(g)])
             if n else np.zeros((0, 3), np.int32))
    return np.ascontiguousarray(edges), offs


@functools.lru_cache(maxsize=None)
def engine_inputs(name):
    """dict(A [b, C, v, v] fp32, h0, dhT, w, edges int32 [n, 3] / offsets int32
    [b + 1] or None for a dense feed); cached, read-only."""
    if name not in LOCAL:
        x = dict(EC.inputs(name))
    else:
        c = LOCAL[name]
        E = c.C // 2
        rng = np.random.default_rng(4242 + c.v + c.h)
        graphs = None
        if c.kind == "dense":
            A, h0 = O.synthetic_batch(c.b, c.v, c.h, c.C, seed=c.h * 3 + c.C, density=0.1)
            A = np.array(A, np.float32)
        else:
            if c.kind == "full":
                graphs = []
                for _ in range(c.b):
                    g = [(int(rng.integers(0, i)), int(rng.integers(1, E + 1)), i) for i in range(1, c.v)]
                    g.append((c.v - 1, 1, 1))           # (node 1's tree edge comes from node 0: no repeat)
                    graphs.append(g)
            else:
                graphs = EC.trees(c.b, c.v, E, 150)
            A = np.stack([O.graph_to_adj_mat_bd(g, c.v, E, dtype=np.float32) for g in graphs])
            h0 = rng.uniform(-0.2, 0.2, (c.b, c.v, c.h)).astype(np.float32)
        x = dict(A=A, h0=np.array(h0, np.float32), w=O.synthetic_weights(c.h, c.C, seed=c.h * 3 + c.C),
                 dhT=rng.standard_normal((c.b, c.v, c.h)).astype(np.float32), graphs=graphs)
    x["edges"], x["offsets"] = _edge_arrays(x["graphs"]) if x["graphs"] is not None else (None, None)
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def local_reference(name):
    """(h_T, gradients) of the float64 oracle for a LOCAL case; cached."""
    c, x = LOCAL[name], engine_inputs(name)
    A64, w64 = x["A"].astype(np.float64), {k: a.astype(np.float64) for k, a in x["w"].items()}
    dr = dropout_of(c)
    ref, caches = O.forward(A64, x["h0"].astype(np.float64), w64, c.T,
                            dropout=dr if min(c.ek, c.sk) < 1.0 else None)
    return ref, O.backward(A64, x["dhT"].astype(np.float64), caches, w64)


def make_engine(g, device=None):
    from ggnn_amd.engine import PropagationEngine
    c = g.c
    return PropagationEngine(c.h, c.C, use_edge_bias=c.bias, precision=g.precision, skip_empty_channels=g.skip,
                             force_generic=c.generic and c.h in (128, 256), device=device)


def uses_edges(c):
    return c.kind in ("edges", "full")


def engine_plan(eng, g):
    """The engine's four byte buffers for a case, as PropagationEngine sizes
    them: [(name, nbytes)] for adjacency, pack, ws.train, ws.inf, and the
    workspace keys.  Sets eng._sparse the way the staging call will."""
    from ggnn_amd import _lib
    c, x = g.c, engine_inputs(g.c.name)
    dr = dropout_of(c)
    ek, ed = dr["edge_keep"], dr["edge_keep"] < 1.0
    eng._sparse = eng._use_pairs(c.b, c.v, int(x["edges"].shape[0])) if uses_edges(c) else False
    pb, pv = (c.b, c.v) if (g.batch_pack and ed) else (1, 1)
    wd = eng.dims(c.b, c.v, c.T, edge_keep=0.5 if ed else 1.0)       # (PropagationEngine.workspace)
    plan = [("adjacency", _lib.adjacency_bytes(eng.dims(c.b, c.v, 1))),
            ("pack", _lib.weight_pack_bytes(eng.dims(pb, pv, c.T if ed else 1, edge_keep=ek, seed=dr["seed"]))),
            ("ws.train", _lib.workspace_bytes(wd, True)),
            ("ws.inf", _lib.workspace_bytes(wd, False))]
    keys = {"ws.train": (c.b, c.v, c.T, True, ed, eng._sparse), "ws.inf": (c.b, c.v, c.T, False, ed, eng._sparse)}
    return plan, keys


def engine_typed_bytes(g):
    """The byte counts of the typed regions of a case (inputs, outputs, masks)."""
    c, x = g.c, engine_inputs(g.c.name)
    n = [a.nbytes for a in x["w"].values()] + [x["h0"].nbytes] * 5 + [a.nbytes for a in x["w"].values()]
    n += [x["A"].nbytes] if not uses_edges(c) else [x["edges"].nbytes, x["offsets"].nbytes]
    n += [c.C * c.h * c.h, c.b * c.v * c.h]
    return n


# -------------------------------------------------------------------- gemm
GEMM_SHAPES = [(1, 1, 1), (37, 150, 61), (130, 129, 257), (132, 260, 40), (28, 400, 88), (33, 148, 1000),
               (96, 32, 264)]
GEMM_KERNELS = (1, 2, 3, 4, 5)      # ggnn_dbg_gemm_ex: 1 k_gemm, 2 k_gemm_ring, 3 / 4 / 5 k_gemm_ks with 1 / 2 / 4 column blocks


def gemm_admits(kernel, M, N, K, b_layout):
    """A [M, K] row-major fp32 and B [K, N] (b_layout 0) or [N, K] (1), both
    16-byte aligned: k_gemm takes everything; the ring and k_gemm_ks need every
    16-byte chunk inside one operand row (generic_path.h ring_ok, the rules
    test_gpu_generic.py states): K % 4 == 0, and N % 4 == 0 for B [K, N]."""
    return kernel == 1 or (K % 4 == 0 and (b_layout == 1 or N % 4 == 0))


GEMM_CASES = [(M, N, K, kern, bl) for (M, N, K) in GEMM_SHAPES for kern in GEMM_KERNELS for bl in (0, 1)
              if gemm_admits(kern, M, N, K, bl)]


# ------------------------------------------------------------------ decode
# call -> the largest n its kernel keeps in LDS (include/ggnn.h; tree_decode
# has no second tier and takes the projective pass's batch)
def decode_lds_maxn(call):
    from ggnn_amd import _lib
    return {"tree_decode": _lib.PROJ_LDS_MAXN, "projective_decode": _lib.PROJ_LDS_MAXN,
            "projective_marginals": _lib.MARG_LDS_MAXN, "tree_marginals": _lib.LAPL_LDS_MAXN,
            "tree_loss0": _lib.LAPL_LDS_MAXN, "tree_loss1": _lib.MARG_LDS_MAXN,
            "tree_sample1": _lib.SAMPLE_LDS_MAXN, "tree_sample3": _lib.SAMPLE_LDS_MAXN}[call]


DECODE_CALLS = ("tree_decode", "projective_decode", "projective_marginals", "tree_marginals", "tree_loss0",
                "tree_loss1", "tree_sample1", "tree_sample3")
DECODE_BATCHES = ("tiers", "tiny")
DECODE_CASES = [(call, batch, sr) for call in DECODE_CALLS for batch in DECODE_BATCHES for sr in (1, 0)]


@functools.lru_cache(maxsize=None)
def decode_batch(call, batch):
    """(probs float32 [b, v, v], n int32 [b], gold_head float32 [b, v, v],
    scores int32 [b, v, v], pred int32 [b, v, 2], gold int32 [b, v, 2], counts
    int32 [b, 5]).  "tiers": graphs of n = 1, 2, L, L + 1 and v with v = L + 3,
    L the call's LDS_MAXN: the workspace has both tiers and its global part
    the fewest users; "tiny": b = 1, v = 2.  pred holds each word's arg-max
    head over the columns < n (seldom a tree: the passes have work to do),
    gold the chain i -> i - 1.  Read-only."""
    import tree_loss_cases as TL
    from ggnn_amd import evaluation as E
    if batch == "tiny":
        v, n = 2, np.asarray([2], np.int32)
    else:
        L = decode_lds_maxn(call)
        v, n = L + 3, np.asarray([1, 2, L, L + 1, L + 3], np.int32)
    b = len(n)
    p, _ = TL.softmax_probs(b, v, v, 5)
    y = np.stack([TL.chain_gold(int(m), v, v) for m in n])
    scores = np.ascontiguousarray(E.tree_scores(p, n, v), np.int32)
    pred = np.full((b, v, 2), -1, np.int32)
    gold = np.full((b, v, 2), -1, np.int32)
    counts = np.zeros((b, 5), np.int32)
    for g, m in enumerate(n):
        m = int(m)
        for i in range(1, m):
            pred[g, i] = (int(np.argmax(p[g, i, :m])), 0)
            gold[g, i] = (i - 1, 0)
        counts[g] = (m - 1 if m > 1 else 0, 0, int((pred[g, 1:m, 0] == gold[g, 1:m, 0]).sum()), max(m - 1, 0), 1)
    out = (p, n, y, scores, pred, gold, counts)
    for a in out:
        a.setflags(write=False)
    return out


def decode_workspaces(lib, call, b, v):
    """[(region name, nbytes)] of a decode case's workspaces, from the
    library's own size functions."""
    if call.startswith("tree_loss"):
        return [("ws", int(lib.ggnn_tree_loss_workspace_bytes(b, v, int(call[-1]))))]
    if call.startswith("tree_sample"):
        return [("ws.marginals", int(lib.ggnn_tree_marginals_workspace_bytes(b, v))),
                ("ws", int(lib.ggnn_tree_sample_workspace_bytes(b, v, int(call[-1]))))]
    return [("ws", int(getattr(lib, "ggnn_%s_workspace_bytes" % call)(b, v)))]


# ------------------------------------------- heads, embedding, clip + Adam
# (b, v, H, output sizes): the axes of tests/test_gpu_heads_edges.py (every NI
# branch of the softmax, H % 4 != 0, H % 64 != 0, the dW split-K chunks, the
# second grid-stride trips); (1, 7, 12, (5, 3)) has b = 1 and odd output sizes
HEADS_SHAPES = [
    (3, 11, 64, (1,)), (3, 11, 64, (1000, 63)), (3, 11, 64, (64, 65, 129, 128)), (3, 11, 64, (257, 256, 1024, 1)),
    (3, 11, 3, (65, 7)), (3, 11, 50, (65, 7)), (3, 11, 100, (65, 7)), (3, 11, 400, (65, 7)), (3, 11, 128, (65, 7)),
    (1, 1, 12, (5, 3)), (1, 7, 12, (5, 3)), (1, 257, 64, (5, 3)), (3, 100, 12, (5, 3)), (17, 241, 12, (5, 3)),
    (1, 12289, 64, (5, 3)), (130, 127, 12, (5, 3)),
]
# (b, v, o, oe) of ggnn_heads_decode (v <= o): odd sizes, b = 1, the widest o
DECODE_HEAD_SHAPES = [(3, 11, 65, 7), (1, 7, 7, 3), (4, 33, 1024, 13)]
# (layout, b, v, keep, out-of-range ids): tests/test_gpu_embed_edges.py's, plus its capped backward grid
EMBED_CASES = [("exact10", 1, 1, 1.0, None), ("exact10", 3, 7, 0.6, "near"), ("exact10", 2, 5, 0.6, "far"),
               ("wide200", 1, 3, 1.0, None), ("wide200", 5, 23, 0.55, "far"), ("eight64", 3, 7, 0.7, None),
               ("eight64", 2, 5, 1.0, "near"), ("full24", 3, 7, 0.7, "far"), ("cap256", 130, 127, 0.8, "far")]
# the element counts of the tensors of one flat buffer, none a multiple of 4
# (150 and 46: the biases of a btb model; 262147: a second element-by-element
# trip): all but two of the tensors start off a 16-byte boundary
ADAM_FLAT = (1, 2, 3, 5, 1023, 150, 1025, 46, 262147)
ADAM_SCRATCH_PER_TENSOR = 256       # include/ggnn.h GGNN_ADAM_SCRATCH_PER_TENSOR

_DUMMY = 256                        # a non-NULL address for the size functions, which read no memory


def heads_workspace_bytes(lib, b, v, h, os_):
    import ctypes
    from ggnn_amd import _lib
    from ggnn_amd.heads import OutputHead
    tab = (OutputHead * len(os_))()
    for i, o in enumerate(os_):
        tab[i] = OutputHead(_DUMMY, _DUMMY, o, None, _DUMMY, None, None)
    d, n = _lib.dims(b, v, h, 1, 1, True, "fp32"), ctypes.c_size_t(0)
    _lib.check(lib.ggnn_heads_workspace_bytes(ctypes.byref(d), tab, len(os_), ctypes.byref(n)),
               "ggnn_heads_workspace_bytes")
    return int(n.value)


def embed_workspace_bytes(lib, layout):
    import ctypes
    from ggnn_amd import _lib
    from ggnn_amd.heads import EmbedSegment
    from test_gpu_embed_edges import LAYOUTS
    L = LAYOUTS[layout]
    segs = (EmbedSegment * len(L["segs"]))()
    for s, ti in enumerate(L["segs"]):
        rows, width = L["tables"][ti]
        segs[s] = EmbedSegment(_DUMMY, _DUMMY, rows, width, s)
    n = ctypes.c_size_t(0)
    _lib.check(lib.ggnn_embed_workspace_bytes(segs, len(L["segs"]), ctypes.byref(n)), "ggnn_embed_workspace_bytes")
    return int(n.value)
