"""Uneven batches and per-slice gradient errors, shared by
tests/test_slice_inputs.py (CPU) and tests/test_gpu_slice_parity.py (GPU).

numpy and the oracle only: nothing here touches the GPU.

Every other gradient check of the propagation engine measures one number per
tensor, max |got - ref| / max |ref| (_nmax), on inputs whose graphs and
channels all carry equally large gradients.  Training batches do not: the btb
loss masks rows out, confident sentences carry gradients orders of magnitude
below hard ones, and most of the 92 labels occur in a handful of sentences.
The backward runs on S * dL/dh_T with ONE power of two S for the batch
(ggnn_common.h gscale), sums every graph into one tile per channel (k_wgrad,
the general path's split-K slabs) and decides per graph and per channel what to
compute at all (WgPlan::lists, the pair rows, empty-channel skipping).  uneven()
builds batches of that kind and slice_errors() measures every graph's dL/dh0
and every channel's dW_c / dbeta_c against its OWN maximum.
"""
import functools
from collections import namedtuple

import numpy as np

import ggnn_oracle as O
from engine_edge_cases import GRADS, dropout_of, trees

SPREAD = 8               # graph g's dL/dh_T is scaled by 2^(-SPREAD g / (b - 1))
DENSITY = 0.1
SLICE_BAR = 1e-3         # FP32_TOL of the GPU suites
HARD = 1.0 / 64          # the quiet slices' share of their tensor's maximum, at most

# kind: "dense" = Bernoulli(DENSITY) adjacency, "edges" = dependency trees staged
# from edge lists (C = 2E).  lscale: a power of two on the whole dL/dh_T.
# unused: an edge label that occurs nowhere (its two channels are empty), or 0
Case = namedtuple("Case", "name b v h C T ek sk seed kind bias generic lscale unused")


def _c(name, b, v, h, C, T, ek=1.0, sk=1.0, seed=0, kind="dense", generic=False, lscale=1.0, unused=0):
    return Case(name, b, v, h, C, T, ek, sk, seed, kind, True, generic, lscale, unused)


# The smallest shapes that still reach each backward tier (the comment names
# it; tests/test_slice_inputs.py recomputes it from engine_edge_cases.tiers).
# Seeds: a case's seed is the first one whose EMULATED per-slice error meets
# 6e-4 (test_slice_inputs.py, test_gpu_bar_is_attainable) and whose quiet slices
# are at most 1/64 of their tensors (test_inputs_are_hard_enough); the rejected
# ones stand next to the case.
# (worst emulated slice; largest rare dW_c, dbeta_c share of the tensor's
# maximum.  At b = 4 the rule puts graph b-2 at 2^-5.3 of graph 0, so its
# channel meets 1/64 = 0.0156 only on some data: most rejections are that)
CASES = [
    _c("u128", 8, 32, 128, 6, 2),                              # specialised 128, k_wgrad<64> (N = 256)
    # seed 0: 8.4e-4
    _c("u128_kc32", 7, 32, 128, 6, 2, seed=1),                 # N = 224: KC = 32, k_wgrad<32>, RT = 1
    # seeds 0..4: dW / dbeta shares 0.029 / 0.021, 0.014 / 0.025, 0.038 / 0.033, 0.029 / 0.037, 0.025 / 0.027
    _c("u256_pad", 4, 40, 256, 6, 3, seed=5),                  # v -> 64, N = 256: k_wgrad256 over graph lists
    _c("u256_n320", 5, 40, 256, 6, 3),                         # N % 128 != 0: k_gru_fwd<256, 2>, 128-tile k_wgrad
    # b = 4 rather than 2: the target-less graph 1 and the two rare channels'
    # graphs 2 and 3 stay distinct (N = 512, still a fraction of a second).
    # seed 0: 6.3e-4 and 0.034 / 0.043; 1: 0.018 / 0.022; 2: 0.052 / 0.082
    _c("u256_v128", 4, 128, 256, 4, 2, seed=3),                # config 3's tile shape: fused forward, WgPlan::lists
    # seed 0: dbeta share 0.017
    _c("u128_drop", 8, 32, 128, 6, 2, ek=0.9, sk=0.9, seed=1),  # dropout masks on a rare channel
    _c("u256_lossscale", 4, 40, 256, 6, 3, seed=5, lscale=2.0 ** -14),  # u256_pad's data under another S
    # seed 0: 0.052 / 0.043; 1: 0.040 / 0.017
    _c("ugen_h100", 4, 37, 100, 6, 2, seed=2, generic=True),   # general tiles, h % 4 == 0 but not 32
    _c("upair_h400", 6, 30, 400, 8, 2, kind="edges"),          # pair mode
    # label 1 occurs nowhere: its two channels are empty.  seed 0: a rare
    # channel's dW_c is exactly 0 (one target in the last graph); 1: 0.027 /
    # 0.022; 2: 6.5e-4; 3: 6.3e-4
    _c("upair_h20_drop", 4, 11, 20, 8, 2, ek=0.7, sk=0.8, seed=4, kind="edges", unused=1),  # pair mode, tiny h, dropout
]
ALL = {c.name: c for c in CASES}
assert len(ALL) == len(CASES)
GRAPH_ORDER_CASES = ("u128", "upair_h400")
BIT16_CASES = ("u128", "upair_h400")


def zero_graph(c):
    return 1


def quiet_graph(c):
    return c.b - 1


def rare_channels(c):
    """{channel: the only graph that occupies it}."""
    if c.kind == "dense":
        return {c.C - 2: c.b - 1, c.C - 1: c.b - 2}
    E = c.C // 2
    la, lb = _rare_labels(c)
    return {la - 1: c.b - 1, la - 1 + E: c.b - 1, lb - 1: c.b - 2, lb - 1 + E: c.b - 2}


def _rare_labels(c):
    # label E shares its channels with the previous / next-word edges
    # (graph_to_adj_mat_bd), so it is in every graph whatever the rule
    return (2, 3)


def _seed(c):
    return 2000 + 17 * c.b + c.v + c.h + c.C + c.seed


# ------------------------------------------------------------ input builders
@functools.lru_cache(maxsize=None)
def uneven(name, spread=SPREAD):
    """dict(A [b, C, v, v] fp32, h0, dhT, w, graphs or None, sizes [b],
    mask [b, v] bool: the rows with a target); cached, read-only.
      * n_g ~ U{v/2..v} nodes; padded rows and columns of A are 0, padded rows
        of dhT exactly 0 (h0's are random, as in O.synthetic_batch);
      * dhT[g] = N(0,1) 2^(-spread g / (b - 1)) in fp32, times the case's lscale;
      * a Bernoulli(0.5) row mask zeroes whole rows of dhT (the target mask);
      * graph 1 has dhT == 0 everywhere and keeps its edges;
      * dense: channels 0..C-3 at density 0.1 in every graph, channel C-2 in
        graph b-1 (the quietest) only, channel C-1 in graph b-2 only;
      * edges: label 2 occurs in the last graph only, label 3 in the one before
        it only (each label is two channels); the others carry label 1, or
        label E where the case leaves label 1 unused."""
    c = ALL[name]
    seed = _seed(c)
    rng = np.random.default_rng(seed)
    graphs = None
    if c.kind == "edges":
        E = c.C // 2
        la, lb = _rare_labels(c)
        common = E if c.unused == 1 else 1
        graphs = []
        for g, edges in enumerate(trees(c.b, c.v, E, seed)):
            keep = {la: g == c.b - 1, lb: g == c.b - 2}
            out = [(s, e if keep.get(e, e != c.unused) else common, d) for s, e, d in edges]
            rare = la if g == c.b - 1 else lb if g == c.b - 2 else 0
            if rare and not any(e == rare for _, e, _ in out):
                s, _, d = out[0]
                out[0] = (s, rare, d)
            graphs.append(out)
        sizes = np.array([len(g) + 1 for g in graphs])
        A = np.stack([O.graph_to_adj_mat_bd(g, c.v, E, dtype=np.float32) for g in graphs])
    else:
        sizes = rng.integers(c.v // 2, c.v + 1, c.b)
        A = np.zeros((c.b, c.C, c.v, c.v), np.float32)
        for g, n in enumerate(sizes):
            chans = list(range(c.C - 2))
            if g == c.b - 1:
                chans.append(c.C - 2)
            if g == c.b - 2:
                chans.append(c.C - 1)
            for ch in chans:
                A[g, ch, :n, :n] = rng.random((n, n)) < DENSITY
    h0 = rng.uniform(-0.2, 0.2, (c.b, c.v, c.h)).astype(np.float32)
    w = O.synthetic_weights(c.h, c.C, seed=seed)
    rng2 = np.random.default_rng(seed + 2)
    dhT = rng2.standard_normal((c.b, c.v, c.h)).astype(np.float32)
    mask = rng2.random((c.b, c.v)) < 0.5
    mask &= np.arange(c.v)[None, :] < sizes[:, None]
    mask[zero_graph(c)] = False
    scale = np.exp2(-spread * np.arange(c.b) / (c.b - 1)).astype(np.float32)
    dhT = dhT * scale[:, None, None] * np.float32(c.lscale)
    dhT = np.where(mask[:, :, None], dhT, np.float32(0.0)).astype(np.float32)
    out = dict(A=A, h0=h0, dhT=dhT, w=w, sizes=sizes, mask=mask)
    for x in (A, h0, dhT, sizes, mask) + tuple(w.values()):
        x.setflags(write=False)
    out["graphs"] = graphs
    return out


def _f64(x):
    return (x["A"].astype(np.float64), x["h0"].astype(np.float64), x["dhT"].astype(np.float64),
            {k: a.astype(np.float64) for k, a in x["w"].items()})


@functools.lru_cache(maxsize=None)
def _caches(name):
    """(h_T, caches) of the float64 oracle (they do not depend on the spread)."""
    c = ALL[name]
    A, h0, _, w = _f64(uneven(name))
    return O.forward(A, h0, w, c.T, dropout=dropout_of(c))


def _frozen(g):
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name, spread=SPREAD):
    """(h_T, gradients) of the float64 oracle; cached, read-only."""
    A, _, dhT, w = _f64(uneven(name, spread))
    hT, caches = _caches(name)
    hT.setflags(write=False)
    return hT, _frozen(O.backward(A, dhT, caches, w))


def grad_scale(dhT):
    """S = 2^-floor(log2 max |dL/dh_T|), the engine's one scale per batch
    (ggnn_common.h gscale_exp; normal, non-zero maxima)."""
    m = float(np.abs(dhT).max())
    assert m > 0.0 and np.isfinite(m)
    _, e = np.frexp(m)              # m = f 2^e, f in [0.5, 1): floor(log2 m) = e - 1
    return 2.0 ** -(int(e) - 1)


def policy(c):
    """The arguments of O.backward_operand_policy that restate a case's path:
    the specialised kernels (hidden 128 / 256) take their limb corrections on
    the fp8 MFMA; the general path (pair mode included) keeps split limbs in
    the chain and single f16 weight-gradient operands (generic_path.h, WPREC),
    the function's defaults."""
    if c.h in (128, 256) and not c.generic and c.kind != "edges":
        return ("f16x2", "f8lo", "f8corr", "f16")
    return ()


@functools.lru_cache(maxsize=None)
def emulated(name, spread=SPREAD):
    """The oracle's operand-policy backward on S dhT, divided by S."""
    c = ALL[name]
    A, _, dhT, w = _f64(uneven(name, spread))
    S = grad_scale(uneven(name, spread)["dhT"])
    g = O.backward_operand_policy(A, S * dhT, _caches(name)[1], w, *policy(c))
    return _frozen({k: a / S for k, a in g.items()})


# ------------------------------------------------------------------- slices
def slices(grads, sizes=None):
    """(name, view) of every slice a bug can hide in: dL/dh0 per graph (with
    sizes: its real rows, and its padded rows as a slice of their own), dW_c
    and dbeta_c per channel, the four h x h blocks of the gates kernel (rows
    [x; h], columns [r | u]), the halves of the gates bias, the row halves of
    the candidate kernel ([x; r h]) and the candidate bias."""
    h0 = grads["h0"]
    hd = h0.shape[-1]
    for g in range(h0.shape[0]):
        n = h0.shape[1] if sizes is None else int(sizes[g])
        yield "h0[%d]" % g, h0[g, :n]
        if n < h0.shape[1]:
            yield "h0[%d] padded" % g, h0[g, n:]
    ew = grads["edge_weights"]
    eb = np.asarray(grads["edge_biases"]).reshape(ew.shape[0], hd)
    for ch in range(ew.shape[0]):
        yield "edge_weights[%d]" % ch, ew[ch]
    for ch in range(ew.shape[0]):
        yield "edge_biases[%d]" % ch, eb[ch]
    gk = np.asarray(grads["gates_kernel"]).reshape(2 * hd, 2 * hd)
    for i, rn in enumerate("xh"):
        for j, cn in enumerate("ru"):
            yield "gates_kernel[%s,%s]" % (rn, cn), gk[i * hd:(i + 1) * hd, j * hd:(j + 1) * hd]
    gb = np.asarray(grads["gates_bias"]).reshape(2 * hd)
    yield "gates_bias[r]", gb[:hd]
    yield "gates_bias[u]", gb[hd:]
    ck = np.asarray(grads["candidate_kernel"]).reshape(2 * hd, hd)
    yield "candidate_kernel[x]", ck[:hd]
    yield "candidate_kernel[rh]", ck[hd:]
    yield "candidate_bias", np.asarray(grads["candidate_bias"]).reshape(hd)


def slice_errors(got, ref, sizes=None):
    """({slice: max |got - ref| / max |ref|}, zero): a slice whose reference is
    0 everywhere has no scale and goes into no ratio; `zero` lists those, and
    not_exactly_zero() compares them with 0."""
    errs, zero = {}, []
    for (name, x), (name_r, r) in zip(slices(got, sizes), slices(ref, sizes)):
        assert name == name_r and x.shape == r.shape, (name, name_r, x.shape, r.shape)
        m = float(np.abs(r).max())
        if m == 0.0:
            zero.append(name)
        else:
            errs[name] = float(np.abs(x - r).max() / m)
    return errs, zero


def not_exactly_zero(got, names, sizes=None):
    """Those of the slices `names` that hold anything but +-0 (a NaN is not 0)."""
    return [n for n, x in slices(got, sizes) if n in set(names) and not np.all(x == 0.0)]


def tensor_of(slice_name):
    return slice_name.split("[")[0]


def worst_per_tensor(errs):
    """{tensor: (its worst slice, that slice's error)}."""
    out = {}
    for n, e in errs.items():
        k = tensor_of(n)
        if k not in out or e > out[k][1]:
            out[k] = (n, e)
    return out


def whole_tensor_errors(got, ref):
    """The old metric, _nmax per gradient."""
    return {k: float(np.abs(np.asarray(got[k]).reshape(ref[k].shape) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30))
            for k in GRADS}


def reverse_graphs(x):
    """The same batch with its graph order reversed (inputs of uneven())."""
    out = dict(x)
    for k in ("A", "h0", "dhT", "sizes", "mask"):
        out[k] = np.ascontiguousarray(x[k][::-1])
    if x["graphs"] is not None:
        out["graphs"] = list(x["graphs"][::-1])
    return out
