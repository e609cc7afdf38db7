"""Edge-shape tests of the propagation engine (ggnn_forward / ggnn_backward
behind PropagationEngine): poisoned buffers, one engine across many batch
shapes, and the dispatch tiers against the float64 oracle.

A. Every buffer the engine only writes -- the weight pack, the staged
   adjacency, the workspace, `out` and the gradient dict -- is filled with 0xFF
   (NaN as fp32, f16 and bf16) and with 0 before the call.  The outputs must be
   finite, bit-identical between the two fills, and in the fp32 mode within the
   parity bars of tests/test_gpu_parity.py (h_T max |err| <= 1e-3, gradients
   max |err| / max |ref| <= 1e-3).  A fresh allocation is usually zeros; a
   training run recycles the caching allocator's blocks.
B. One engine and one pack are driven through a sequence of (b, v, T,
   training) steps; every output equals bit for bit the same step on a freshly
   constructed engine.
C. The case table (tests/engine_edge_cases.py) walks the tiers of
   ggnn_api.hip's dispatch; tests/test_engine_edge_inputs.py asserts on the CPU
   that it reaches each of them and that the inputs are what they claim.

Measured on an MI355X: the whole module runs in about 4 s (77 tests); the
T = 16 test's docstring holds its maxima.
"""
import numpy as np
import pytest

import engine_edge_cases as EC

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
FP16_RMS_TOL = 1e-2
BF16_RMS_CAP = 2e-2
GRAD_RMS_TOL = 5e-2
GRADS = EC.GRADS


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _nrms(x, ref):
    return float(np.sqrt(np.mean((x - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def _nmax(x, ref):
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-30))


def _engine(c, precision="fp32", skip=True, **kw):
    _torch()
    from ggnn_amd.engine import PropagationEngine
    return PropagationEngine(c.h, c.C, use_edge_bias=c.bias, precision=precision, skip_empty_channels=skip,
                             force_generic=c.generic and c.h in (128, 256), **kw)


def _dev(eng, x):
    torch = _torch()
    return torch.from_numpy(np.array(x, order="C")).to(eng.device)      # (a copy: the cached inputs are read-only)


def _poison(t, fill):
    """Every byte of a contiguous tensor = fill."""
    torch = _torch()
    if t is not None and fill is not None:
        t.view(torch.uint8).fill_(fill)
    return t


def _step(eng, adj, h0, w, T, dr, dhT, fill, batch_pack=False, pack=None, between=None, inference=True):
    """One training step (forward + backward; skipped when dhT is None) and
    one inference forward (skipped when inference is False) on `eng`, with
    every buffer the calls only write filled with the byte `fill` first (fill
    None: the engine's own allocations).
    adj: a dense [b, C, v, v] array, or (graphs, num_edge_types) edge lists.
    dr: dict(edge_keep, state_keep, seed) or None.  pack: a WeightPack to use
    instead of packing `w`.  between: called between forward and backward."""
    torch = _torch()
    from ggnn_amd import _lib
    dev = eng.device
    dr = dr or dict(edge_keep=1.0, state_keep=1.0, seed=0)
    ek, sk, seed = dr["edge_keep"], dr["state_keep"], dr["seed"]
    b, v, h = h0.shape

    def full(n):
        return torch.full((n,), fill, dtype=torch.uint8, device=dev)

    # ---- staging, into a preallocated poisoned buffer
    if isinstance(adj, np.ndarray):
        if fill is not None:
            eng._sparse = False     # (what set_adjacency sets before it sizes the buffer)
            eng._adj = full(_lib.adjacency_bytes(eng.dims(b, v, 1)))
        eng.set_adjacency(_dev(eng, adj))
    else:
        graphs, E = adj
        if fill is not None:
            eng._sparse = eng._use_pairs(b, v, sum(len(g) for g in graphs))
            eng._adj = full(_lib.adjacency_bytes(eng.dims(b, v, 1)))
        eng.set_adjacency_edges(graphs, v, E)
    # ---- the pack
    if pack is None:
        out = None
        if fill is not None:
            pb, pv = (b, v) if (batch_pack and ek < 1.0) else (1, 1)
            out = full(_lib.weight_pack_bytes(eng.dims(pb, pv, T if ek < 1.0 else 1, edge_keep=ek, seed=seed)))
        pack = eng.pack_weights({k: _dev(eng, x) for k, x in w.items()}, T=T, edge_keep=ek, seed=seed,
                                batch=batch_pack, out=out)
    h0d = _dev(eng, h0)
    res = {}
    # ---- training step
    if dhT is not None:
        _poison(eng.workspace(b, v, T, True, ek < 1.0), fill)
        out = _poison(torch.empty((b, v, h), dtype=torch.float32, device=dev), fill)
        hT = eng.forward(h0d, pack, T, training=True, out=out, state_keep=sk)
        grads = eng.alloc_grads(b, v)
        for g in grads.values():
            _poison(g, fill)
        if between is not None:
            between()
        eng.backward(_dev(eng, dhT), grads)
        res["hT"] = hT.cpu().numpy()
        res.update({k: (None if g is None else g.cpu().numpy()) for k, g in grads.items()})
    # ---- inference forward (its own workspace; the same pack and masks)
    if inference:
        _poison(eng.workspace(b, v, T, False, ek < 1.0), fill)
        out = _poison(torch.empty((b, v, h), dtype=torch.float32, device=dev), fill)
        res["hT_inf"] = eng.forward(h0d, pack, T, training=False, out=out, state_keep=sk).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(h0d.cpu().numpy(), h0)      # inputs read in place stay untouched
    return res


def _adj_of(c, x):
    return (x["graphs"], c.C // 2) if c.kind == "edges" else x["A"]


def _check_finite(res, tag):
    for k, a in res.items():
        if a is not None:
            assert np.isfinite(a).all(), (tag, k)


def _check_same(r1, r0):
    for k in r1:
        if r1[k] is None:
            assert r0[k] is None, k
        else:
            assert np.array_equal(r1[k], r0[k]), (k, float(np.abs(r1[k] - r0[k]).max()))


def _errors(c, res, ref, gref):
    e = {"hT": float(np.abs(res["hT"] - ref).max()), "hT_inf": float(np.abs(res["hT_inf"] - ref).max())}
    for k in GRADS:
        if k == "edge_biases" and not c.bias:
            assert res[k] is None
            continue
        e[k] = _nmax(res[k].reshape(gref[k].shape), gref[k])
    return e


def _poisoned_pair(c, precision="fp32", skip=True, batch_pack=False, **kw):
    """The case through _step on two fresh engines, 0xFF- and 0-filled:
    (a) finite, (b) bit-identical; returns the 0xFF run."""
    x = EC.inputs(c.name)
    runs = []
    for fill in (0xFF, 0x00):
        eng = _engine(c, precision, skip, **kw)
        runs.append(_step(eng, _adj_of(c, x), x["h0"], x["w"], c.T, EC.dropout_of(c), x["dhT"], fill,
                          batch_pack=batch_pack))
        if c.kind == "edges":
            assert eng.sparse
        _check_finite(runs[-1], "fill %#x" % fill)
    _check_same(runs[0], runs[1])
    return runs[0]


def _check_fp32(c, res, tol=FP32_TOL):
    ref, gref, nodrop = EC.reference(c.name)
    e = _errors(c, res, ref, gref)
    for k, x in e.items():
        assert x <= tol, (k, e)
    if nodrop is not None:      # dropout is really on (asserted for the oracle alone on the CPU)
        assert np.abs(nodrop - ref).max() > 0.05
    return e


# ------------------------------------------------- A + C: the tier table
@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in EC.TIER_CASES if c.name != "fused_maxt"])
def test_tier_poisoned_buffers(name, precision):
    """Every row of the tier table in all three precisions, 0xFF- against
    0-filled buffers; the fp32 mode also against the float64 oracle (forward,
    inference forward and all seven gradients).  The 16-bit modes add the hb
    buffers and inference's k_pad_state branch; their accuracy bars need
    dependency-tree data (test_16bit_statistical_poisoned)."""
    c = EC.ALL_CASES[name]
    res = _poisoned_pair(c, precision)
    if precision == "fp32":
        _check_fp32(c, res)


def test_fused_maxt_poisoned_buffers():
    """T = FUSED_MAXT = 16 exactly: the longest unroll the fused forward takes
    (T = 17 falls back, test_unfused_forward_paths_fp32_parity), training and
    inference.  Bar 4 x FP32_TOL, test_gpu_parity's rule for T > 8 (the split
    mode's ~2^-22 rounding amplified through the recurrence).  The data is
    chosen on the CPU by the reference's own conditioning (float32 oracle
    within 2.5e-4 of float64, engine_edge_cases.MAXT_FP32_REF_ERR).
    Measured on an MI355X: h_T 8.9e-4 (training and inference alike), gradients
    1.8e-4 .. 3.0e-4 (largest: gates_kernel).  On the first seed tried, where
    the float32 oracle itself is 2.1e-3 off float64, the engine measured
    1.1e-2 on h_T and 0.8e-2 .. 1.3e-2 on every gradient (largest:
    candidate_bias): the amplification of the recurrence, about 5 x the
    float32 reference's own error as on the well-conditioned data (14 x)."""
    c = EC.ALL_CASES["fused_maxt"]
    assert c.T == EC.FUSED_MAXT and EC.tiers(c)["fused"]
    res = _poisoned_pair(c)
    ref, gref, _ = EC.reference(c.name)
    e = _errors(c, res, ref, gref)
    print("T = 16 fused forward, measured maxima:", e)
    for k, x in e.items():
        assert x <= 4 * FP32_TOL, (k, e)
    assert _nrms(res["hT"], ref) <= 1e-4


@pytest.mark.parametrize("name", EC.DENSE_CHANNEL_CASES)
def test_dense_channels_poisoned_buffers(name):
    """skip_empty_channels = False (GGNN_DENSE_CHANNELS: the identity channel
    list, every dM^T row written, no per-channel graph lists)."""
    c = EC.ALL_CASES[name]
    _check_fp32(c, _poisoned_pair(c, skip=False))


@pytest.mark.parametrize("name", [c.name for c in EC.EXTRA_CASES])
def test_extra_poisoned_buffers(name):
    """Both dropouts on padded / fused / unfused shapes, use_edge_bias = False,
    and the general path (hidden 100 at v = 37; hidden 128 forced generic)."""
    c = EC.ALL_CASES[name]
    _check_fp32(c, _poisoned_pair(c))


@pytest.mark.parametrize("name,batch_pack", [(c.name, bp) for c in EC.PAIR_CASES
                                             for bp in ((False, True) if c.ek < 1.0 else (False,))])
def test_pair_mode_poisoned_buffers(name, batch_pack):
    """Pair mode from edge lists (hidden 20 and 400), without and with edge
    dropout, the latter also with the pack made for the staged batch
    (pack_weights(batch=True): the channels the batch leaves unused keep the
    poison and must not be read)."""
    c = EC.ALL_CASES[name]
    _check_fp32(c, _poisoned_pair(c, batch_pack=batch_pack))


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name", [c.name for c in EC.BIT16_CASES])
def test_16bit_statistical_poisoned(name, precision):
    """The 16-bit modes at their statistical bars on dependency-tree graphs:
    h_T normalised RMS <= 1e-2 (fp16) / 2e-2 (bf16), every gradient <= 5e-2."""
    c = EC.ALL_CASES[name]
    res = _poisoned_pair(c, precision)
    ref, gref, _ = EC.reference(c.name)
    e = {"hT": _nrms(res["hT"], ref), "hT_inf": _nrms(res["hT_inf"], ref)}
    for k in GRADS:
        e[k] = _nrms(res[k].reshape(gref[k].shape), gref[k])
    cap = FP16_RMS_TOL if precision == "fp16" else BF16_RMS_CAP
    assert e["hT"] <= cap and e["hT_inf"] <= cap, e
    for k in GRADS:
        assert e[k] <= GRAD_RMS_TOL, (k, e)


# ------------------------------------------- C: empty graph, empty channel
@pytest.mark.parametrize("name", [c.name for c in EC.EMPTY_CASES])
def test_empty_graph_and_empty_channel(name):
    """Graph 0 has no edge and the last channel has no edge in any graph: its
    dW_c and dbeta_c are stored as exact zeros (an empty k_chan_graphs list
    through k_wgrad_reduce; k_prop_bwd's zero dbeta partials), with and without
    channel skipping, from poisoned buffers; the rest holds the oracle bars and
    h_T / dL/dh0 are bit-identical between skipping and the dense loop."""
    c = EC.ALL_CASES[name]
    ref, gref, _ = EC.reference(c.name)
    last = c.C - 1
    assert not gref["edge_weights"][last].any() and not gref["edge_biases"][last].any()
    runs = {}
    for skip in (True, False):
        assert EC.tiers(c, skip)["lists"] == (name == "empty_lists" and skip)
        res = runs[skip] = _poisoned_pair(c, skip=skip)
        assert np.all(res["edge_weights"][last] == 0.0), skip
        assert np.all(res["edge_biases"][last] == 0.0), skip
        _check_fp32(c, res)
    for k in ("hT", "hT_inf", "h0"):
        assert np.array_equal(runs[True][k], runs[False][k]), k


# ------------------------------------------------ B: one engine, many shapes
# (b, v, T, training, dropout); v <= 128 on the specialised paths.  The keys
# (b, v, T, training, edge dropout) of the first five steps are distinct, so
# the fifth clears the engine's workspace cache.
_SPEC_STEPS = [
    (8, 128, 2, True, None),        # large, dense; fused at hidden 256
    (2, 33, 2, True, None),         # small after large: a shrinking adjacency payload; padded, unfused
    (2, 64, 3, False, None),        # dense, inference after training
    (3, 100, 2, True, None),        # padded again; fused at hidden 256; training after inference
    (2, 64, 2, True, dict(edge_keep=0.8, state_keep=0.8, seed=99)),   # dropout with its own pack
    (2, 64, 2, True, None),         # the same shape without dropout
    (1, 128, 1, False, None),       # fused, dense, inference
    (4, 20, 1, True, None),         # v -> 32
    (8, 128, 2, True, None),        # the first shape again
]
_GEN_STEPS = [
    (6, 37, 2, True, None),
    (2, 9, 2, True, None),
    (3, 128, 1, False, None),
    (1, 37, 3, True, None),
    (2, 64, 2, True, dict(edge_keep=0.8, state_keep=0.8, seed=99)),
    (2, 64, 2, True, None),
    (4, 8, 1, False, None),
    (6, 37, 2, True, None),
]
_PAIR_STEPS = [
    (6, 30, 2, True, None),
    (2, 7, 2, True, None),
    (3, 25, 1, False, None),
    (1, 30, 3, True, None),
    (2, 16, 2, True, dict(edge_keep=0.8, state_keep=0.8, seed=99)),
    (2, 16, 2, True, None),
    (4, 5, 1, False, None),
    (6, 30, 2, True, None),
]


def _seq_inputs(path, h, C, i, b, v):
    rng = np.random.default_rng(7000 + 31 * i + b + v)
    if path == "pair":
        graphs = EC.trees(b, v, C // 2, 7000 + i)
        adj = (graphs, C // 2)
        h0 = rng.uniform(-0.2, 0.2, (b, v, h)).astype(np.float32)
    else:
        import ggnn_oracle as O
        A, h0 = O.synthetic_batch(b, v, h, C, seed=7000 + i, density=0.1)
        adj = np.ascontiguousarray(A, np.float32)
    dhT = rng.standard_normal((b, v, h)).astype(np.float32)
    return adj, h0, dhT


@pytest.mark.parametrize("path,h,steps", [
    ("spec256", 256, _SPEC_STEPS),
    ("spec128", 128, _SPEC_STEPS),
    ("general", 100, _GEN_STEPS),
    ("pair", 400, _PAIR_STEPS),
])
def test_one_engine_many_shapes(path, h, steps):
    """Bucketed batches change (b, v) at every step, `_adj` only grows, `_ws`
    keeps four shapes and then clears, one pack serves every shape of a hidden
    size, training and inference interleave: after every step every output
    equals bit for bit the same step on a freshly constructed engine."""
    import ggnn_oracle as O
    from ggnn_amd.engine import PropagationEngine
    C = 8 if path == "pair" else 4
    w = O.synthetic_weights(h, C, seed=77)

    def mk():
        return PropagationEngine(h, C, precision="fp32")
    _torch()
    eng = mk()
    pack = eng.pack_weights({k: _dev(eng, x) for k, x in w.items()})
    keys = set()
    cleared = False
    for i, (b, v, T, training, dr) in enumerate(steps):
        adj, h0, dhT = _seq_inputs(path, h, C, i, b, v)
        between = None
        if i == 3:
            # a fifth workspace key between a training forward and its
            # backward: _ws.clear() while _trained still holds the workspace
            def between():
                assert len(eng._ws) == 4
                eng.workspace(b, v, T + 1, True)
                assert len(eng._ws) == 1
            cleared = True
        got = _step(eng, adj, h0, w, T, dr, dhT if training else None, None, pack=None if dr else pack,
                    between=between, inference=not training)
        fresh = _step(mk(), adj, h0, w, T, dr, dhT if training else None, None, inference=not training)
        assert eng.sparse == (path == "pair")
        assert set(got) == set(fresh) and ("h0" in got) == training
        _check_finite(got, i)
        for k in got:
            assert np.array_equal(got[k], fresh[k]), (i, k)
        keys.add((b, v, T, training, dr is not None))
    assert cleared and len(keys) >= 6


def test_engine_guards():
    """backward() without its training forward's state, and packs that do not
    fit the call, are refused."""
    import ggnn_oracle as O
    torch = _torch()
    from ggnn_amd.engine import PropagationEngine
    b, v, h, C, T = 2, 20, 128, 4, 2
    A, h0 = O.synthetic_batch(b, v, h, C, seed=1, density=0.1)
    w = O.synthetic_weights(h, C, seed=1)
    eng = PropagationEngine(h, C)
    wd = {k: _dev(eng, x) for k, x in w.items()}
    pack = eng.pack_weights(wd)
    Ad, h0d = _dev(eng, A), _dev(eng, h0)
    dhT = torch.ones((b, v, h), device=eng.device)
    eng.set_adjacency(Ad)
    eng.forward(h0d, pack, T, training=True)
    eng.forward(h0d, pack, T, training=False)
    with pytest.raises(RuntimeError):          # after an inference forward
        eng.backward(dhT)
    eng.forward(h0d, pack, T, training=True)
    eng.set_adjacency(Ad)
    with pytest.raises(RuntimeError):          # after a re-staging
        eng.backward(dhT)
    ed = eng.pack_weights(wd, T=T, edge_keep=0.8, seed=5)
    with pytest.raises(ValueError):            # edge-dropout masks of another T
        eng.forward(h0d, ed, T + 1, training=True)
    bp = eng.pack_weights(wd, T=T, edge_keep=0.8, seed=5, batch=True)
    eng.forward(h0d, bp, T, training=True)
    eng.set_adjacency(Ad)
    with pytest.raises(RuntimeError):          # a batch=True pack after a re-staging
        eng.forward(h0d, bp, T, training=True)
    torch.cuda.synchronize()
