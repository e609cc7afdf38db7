"""Where the propagation engine writes: ggnn_set_adjacency,
ggnn_set_adjacency_edges, ggnn_pack_weights, ggnn_pack_weights_batch,
ggnn_forward (training and inference workspaces), ggnn_backward and
ggnn_dropout_mask with every buffer an exact region of a guard arena
(tests/guard_arena.py): the staged adjacency, the pack, both workspaces, h0,
dhT, both outs, the seven gradients, the six weights, the dense feed or the
edge and offset arrays, and the two masks.

Per case (tests/guard_cases.py ENGINE_CASES: the tier table in three
precisions, the extra, empty, pair and dense-channel cases, the general
path's ragged hidden sizes under edge dropout, v = 150 dense and in pair mode,
a pair batch with edges == b * v), one sequence stage -> pack -> training
forward -> backward -> inference forward -> masks runs under pattern guards,
NaN guards and on plain allocations (guard_arena.run_guarded): no guard byte
changes, the inputs (and, once written, the pack and on the specialised path
the staged adjacency) stay as they were, the outputs are bit-identical across
the three runs, and in the fp32 mode within test_gpu_engine_edges' bars of
the float64 oracle.
"""
import ctypes

import numpy as np
import pytest

import guard_arena as GA
import guard_cases as GC
from test_gpu_engine_edges import FP32_TOL, GRADS, _check_fp32, _nmax, _torch

pytestmark = pytest.mark.gpu


def _sequence(g, mem):
    torch = _torch()
    from ggnn_amd import _lib
    c, x = g.c, GC.engine_inputs(g.c.name)
    eng = GC.make_engine(g)
    dr = GC.dropout_of(c)
    ek, sk, seed = dr["edge_keep"], dr["state_keep"], dr["seed"]
    b, v, h, C, T = c.b, c.v, c.h, c.C, c.T
    plan, keys = GC.engine_plan(eng, g)
    sparse = eng._sparse
    inputs = []

    def feed(name, a):
        t = mem.tensor(name, a.shape, {np.float32: torch.float32, np.int32: torch.int32}[a.dtype.type], a)
        mem.snapshot(name)
        inputs.append(name)
        return t

    w = {k: feed("w." + k, a) for k, a in x["w"].items()}
    h0, dhT = feed("h0", x["h0"]), feed("dhT", x["dhT"])
    byte = {}
    # ---- staging
    if GC.uses_edges(c):
        edges, offs = feed("edges", x["edges"]), feed("offsets", x["offsets"])
        eng._adj = byte["adjacency"] = mem.region(*plan[0])
        eng.set_adjacency_edges((edges, offs), v, C // 2)
        assert eng.sparse and sparse
    else:
        A = feed("A", x["A"])
        eng._adj = byte["adjacency"] = mem.region(*plan[0])
        eng.set_adjacency(A)
    assert eng._adj is byte["adjacency"]
    if c.h in (128, 256) and c.v <= 128 and not c.generic and not sparse:
        # the specialised path only reads what the staging wrote (the general
        # path rebuilds its channel lists in there on every forward, and pair
        # mode its reverse lists on every backward: generic_path.h gen_lists,
        # gen_pairs_rev)
        mem.snapshot("adjacency")
    # ---- the pack (after the staging: ggnn_pack_weights_batch reads it)
    byte["pack"] = mem.region(*plan[1])
    pack = eng.pack_weights(w, T=T, edge_keep=ek, seed=seed, batch=g.batch_pack, out=byte["pack"])
    assert pack.buf is byte["pack"] and (pack.batch_gen is not None) == (g.batch_pack and ek < 1.0)
    mem.snapshot("pack")
    # ---- training forward + backward
    for name, nbytes in plan[2:]:
        eng._ws[keys[name]] = byte[name] = mem.region(name, nbytes)
    out = {}
    out["hT"] = eng.forward(h0, pack, T, training=True, out=mem.tensor("out.train", (b, v, h), torch.float32),
                            state_keep=sk)
    assert eng._trained[4] is byte["ws.train"]
    shapes = {"h0": (b, v, h), "edge_weights": (C, h, h), "edge_biases": (C, 1, h) if c.bias else None,
              "gates_kernel": (2 * h, 2 * h), "gates_bias": (2 * h,), "candidate_kernel": (2 * h, h),
              "candidate_bias": (h,)}
    grads = {k: None if s is None else mem.tensor("d." + k, s, torch.float32) for k, s in shapes.items()}
    eng.backward(dhT, grads)
    out.update(grads)
    # ---- inference forward (its own workspace; the same pack and masks)
    out["hT_inf"] = eng.forward(h0, pack, T, training=False, out=mem.tensor("out.inf", (b, v, h), torch.float32),
                                state_keep=sk)
    assert eng._ws[keys["ws.inf"]] is byte["ws.inf"] and len(eng._ws) == 2
    # ---- the masks of the last timestep (ggnn_dropout_mask: the binding allocates its own, so through the ABI)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kind, name, shape, keep in ((0, "mask.edge", (C, h, h), ek), (1, "mask.state", (b, v, h), sk)):
        keep = keep if keep < 1.0 else 0.9
        d = eng.dims(b, v, T, keep if kind == 0 else 1.0, keep if kind == 1 else 1.0, seed)
        out[name] = mem.tensor(name, shape, torch.uint8)
        _lib.check(eng._lib.ggnn_dropout_mask(ctypes.byref(d), kind, T - 1, ctypes.c_void_p(out[name].data_ptr()), s),
                   "ggnn_dropout_mask")
    return out


@pytest.mark.parametrize("gid", GC.ENGINE_IDS)
def test_engine_writes_inside_its_buffers(gid):
    g = GC.ENGINE_CASES[GC.ENGINE_IDS.index(gid)]
    c = g.c
    res = GA.run_guarded(lambda mem: _sequence(g, mem), _torch().device("cuda", 0), GC.CAPACITY)
    for name in ("mask.edge", "mask.state"):
        # 0 / 1 bytes; kept elements exist wherever a mask of keep >= 0.7 has 64 or more
        assert set(np.unique(res[name]).tolist()) <= {0, 1} and (res[name].any() or res[name].size < 64), name
    if g.precision != "fp32":
        return
    if not g.local:
        _check_fp32(c, res)
        return
    ref, gref = GC.local_reference(c.name)
    assert np.abs(res["hT"] - ref).max() <= FP32_TOL and np.abs(res["hT_inf"] - ref).max() <= FP32_TOL
    for k in GRADS:
        # (hidden 1: test_generic_edge_dropout_hidden_not_multiple_of_4's bar
        # for the three products' gradients, a cancelling sum of single-f16 products)
        tol = 5e-3 if (c.h == 1 and k in ("edge_weights", "gates_kernel", "candidate_kernel")) else FP32_TOL
        assert _nmax(res[k].reshape(gref[k].shape), gref[k]) <= tol, k


def test_checker_sees_device_writes():
    GA.device_self_test(_torch().device("cuda", 0))
