"""Where the decoders, the tree loss and the sampler write: ggnn_tree_decode,
ggnn_projective_decode, ggnn_projective_marginals, ggnn_tree_marginals,
ggnn_tree_loss (both families), ggnn_tree_sample (1 and 3 samples) and
ggnn_arc_confidence (after either marginals call) through the C ABI, with
every input, every output (pred, counts, status, marg, logz, scores, used,
loss[2], heads, log_prob, conf) and the workspace of exactly
ggnn_*_workspace_bytes an exact region of a guard arena (tests/guard_arena.py;
a size of 0 is a zero-length region).

Two batches per call (tests/guard_cases.py decode_batch): graphs of n = 1, 2,
LDS_MAXN, LDS_MAXN + 1 and v at v = LDS_MAXN + 3, so that the workspace has
both tiers and its global part the fewest users; and b = 1, v = 2.  Single-
and multi-root.  Each call runs under pattern guards, NaN guards and on plain
allocations: no guard byte changes, the inputs stay as they were, and every
output is bit-identical across the three runs.
"""
import ctypes

import numpy as np
import pytest

import guard_arena as GA
import guard_cases as GC
from test_gpu_engine_edges import _torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0FFEE


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _call(mem, call, batch, single_root):
    torch = _torch()
    from ggnn_amd import _lib
    import tree_loss_cases as TL
    lib = _lib.load()
    p_np, n_np, y_np, sc_np, pred_np, gold_np, counts_np = GC.decode_batch(call, batch)
    b, v, o = p_np.shape
    i32, f32 = torch.int32, torch.float32
    d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def feed(name, a):
        t = mem.tensor(name, a.shape, {np.float32: f32, np.int32: i32}[a.dtype.type], a)
        mem.snapshot(name)
        return t

    n = feed("n_nodes", n_np)
    ws = {name: mem.region(name, nbytes) for name, nbytes in GC.decode_workspaces(lib, call, b, v)}
    if batch == "tiers" and call != "tree_decode":
        assert ws["ws"].numel() > 0          # the global-memory tier is in the launch
    out = {}
    if call in ("tree_decode", "projective_decode"):
        scores, gold = feed("scores", sc_np), feed("gold", gold_np)
        out["pred"] = mem.tensor("pred", pred_np.shape, i32, pred_np)
        out["counts"] = mem.tensor("counts", counts_np.shape, i32, counts_np)
        out["status"] = mem.tensor("status", (b,), i32)
        _lib.check(getattr(lib, "ggnn_" + call)(ctypes.byref(d), _P(scores), o, _P(n), single_root, _P(out["pred"]),
                                                _P(gold), _P(out["counts"]), _P(out["status"]), _P(ws["ws"]),
                                                ws["ws"].numel(), s), call)
        return out
    p = feed("probs_head", p_np)
    out["marg"] = mem.tensor("marg", (b, v, o), f32)
    out["logz"] = mem.tensor("logz", (b,), f32)
    if call.startswith("tree_loss"):
        y = feed("gold_head", y_np)
        out["status"] = mem.tensor("status", (b,), i32)
        out["used"] = mem.tensor("used", (b,), i32)
        out["loss"] = mem.tensor("loss", (2,), f32, np.asarray([0.5, 0.25], np.float32))
        _lib.check(lib.ggnn_tree_loss(ctypes.byref(d), _P(p), o, _P(y), _P(n), int(call[-1]), single_root,
                                      float(TL.target_num_of(y_np)), _P(out["marg"]), _P(out["logz"]),
                                      _P(out["status"]), _P(out["used"]), _P(out["loss"]), _P(ws["ws"]),
                                      ws["ws"].numel(), s), call)
        return out
    mws = ws["ws.marginals"] if call.startswith("tree_sample") else ws["ws"]
    name = "tree_marginals" if call.startswith("tree_sample") else call
    out["scores"] = mem.tensor("scores", (b, v, o), i32)
    out["marg_status"] = mem.tensor("marg_status", (b,), i32)
    _lib.check(getattr(lib, "ggnn_" + name)(ctypes.byref(d), _P(p), o, _P(n), single_root, _P(out["marg"]),
                                            _P(out["logz"]), _P(out["scores"]), _P(out["marg_status"]), _P(mws),
                                            mws.numel(), s), name)
    if not call.startswith("tree_sample"):     # ggnn_arc_confidence: the gather of the arg-max heads' marginals
        pred = feed("pred", pred_np)
        mem.snapshot("marg")
        out["conf"] = mem.tensor("conf", (b, v), f32)
        _lib.check(lib.ggnn_arc_confidence(ctypes.byref(d), _P(out["marg"]), o, _P(n), _P(pred), _P(out["conf"]), s),
                   "ggnn_arc_confidence")
    if call.startswith("tree_sample"):
        K = int(call[-1])
        for k in ("marg", "logz", "marg_status"):     # the sampler's inputs from here on
            mem.snapshot(k)
        out["heads"] = mem.tensor("heads", (b, K, v), i32)
        out["log_prob"] = mem.tensor("log_prob", (b, K), f32)
        out["status"] = mem.tensor("status", (b, K), i32)
        _lib.check(lib.ggnn_tree_sample(ctypes.byref(d), _P(p), o, _P(n), single_root, _P(out["marg"]),
                                        _P(out["logz"]), _P(out["marg_status"]), K, SEED, _P(out["heads"]),
                                        _P(out["log_prob"]), _P(out["status"]), _P(ws["ws"]), ws["ws"].numel(), s),
                   call)
    return out


@pytest.mark.parametrize("call,batch,single_root", GC.DECODE_CASES)
def test_decoders_write_inside_their_buffers(call, batch, single_root):
    res = GA.run_guarded(lambda mem: _call(mem, call, batch, single_root), _torch().device("cuda", 0), 16 << 20)
    n = GC.decode_batch(call, batch)[1]
    st = res["marg_status"] if "marg_status" in res else res["status"]
    # the batch does what it is for: every graph answered by the contract's
    # statuses, the one-word graph worked on, and the passes repair the large
    # graphs of both storage tiers (test_guard_arena asserts on the CPU that
    # their arg-max heads are no tree)
    assert np.isin(st, (0, 1, 2)).all() and (st[n < 2] == 0).all(), st
    if call in ("tree_decode", "projective_decode"):
        if batch == "tiers":
            assert (st[2:] == 1).all(), st
    else:
        assert (st[n == 2] == 1).all(), st
    if call.startswith("tree_loss"):
        assert np.array_equal(res["used"], (st == 1).astype(np.int32)), (res["used"], st)
    if call.startswith("tree_sample"):
        off = st != 1
        assert (res["status"][off] == st[off][:, None]).all(), res["status"]


def test_checker_sees_device_writes():
    GA.device_self_test(_torch().device("cuda", 0))
