"""Where ggnn_tree_kbest writes: the call through the C ABI with every input,
every output (heads, totals, count, status) and the workspace of exactly
ggnn_tree_kbest_workspace_bytes an exact region of a guard arena
(tests/guard_arena.py), as tests/test_gpu_guard_projective_kbest.py does for
the projective list.

Two batches: graphs of n = 1, 2, 33, 34 and v at v = 36 (25 % forbidden arcs);
and b = 1, v = 2.  K = 1 (take(0) alone) and K = 16 (31 launches: every rank's
record and pool row is written), single- and multi-root.  Each call runs under
pattern guards, NaN guards and on plain allocations: no guard byte changes, the
inputs stay as they were, and every output is bit-identical across the three
runs and equal to the host form's."""
import ctypes
import functools

import numpy as np
import pytest

import guard_arena as GA
from test_gpu_engine_edges import _torch
from tree_kbest_cases import scores_batch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _batch(batch):
    """(scores int32 [b, v, v], n int32 [b]).  Read-only."""
    if batch == "tiny":
        v, n = 2, np.asarray([2], np.int32)
    else:
        v, n = 36, np.asarray([1, 2, 33, 34, 36], np.int32)
    s = scores_batch(n, v, v, "soft" if batch == "tiny" else "forbid", 5)
    s.setflags(write=False)
    n.setflags(write=False)
    return s, n


def _call(mem, batch, K, single_root):
    torch = _torch()
    from ggnn_amd import _lib
    lib = _lib.load()
    s_np, n_np = _batch(batch)
    b, v, o = s_np.shape
    i32 = torch.int32
    d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def feed(name, a):
        t = mem.tensor(name, a.shape, i32, a)
        mem.snapshot(name)
        return t

    s, n = feed("scores", s_np), feed("n_nodes", n_np)
    ws = mem.region("ws", int(lib.ggnn_tree_kbest_workspace_bytes(b, v, K)))
    assert ws.numel() == b * 4 * (K * (2 * v + 16) + 16)
    out = {"heads": mem.tensor("heads", (b, K, v), i32), "totals": mem.tensor("totals", (b, K), i32),
           "count": mem.tensor("count", (b,), i32), "status": mem.tensor("status", (b,), i32)}
    _lib.check(lib.ggnn_tree_kbest(ctypes.byref(d), P(s), o, P(n), single_root, K, P(out["heads"]), P(out["totals"]),
                                   P(out["count"]), P(out["status"]), P(ws), ws.numel(), stream), "ggnn_tree_kbest")
    return out


@pytest.mark.parametrize("single_root", [1, 0], ids=["single", "multi"])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("batch", ["main", "tiny"])
def test_kbest_writes_inside_its_buffers(batch, K, single_root):
    from ggnn_amd import evaluation as E
    res = GA.run_guarded(lambda mem: _call(mem, batch, K, single_root), _torch().device("cuda", 0), 16 << 20)
    s, n = _batch(batch)
    ref = E.tree_kbest_arrays(s, n, K, bool(single_root))
    for name, a in zip(("heads", "totals", "count", "status"), ref):
        assert res[name].tobytes() == a.tobytes(), name
    # the batch does what it is for: the one-word graph passes through, the others return lists
    st = res["status"]
    assert (st[n < 2] == 0).all() and (st[n > 2] == 1).all(), st
    if batch == "main":
        assert (res["count"][n > 2] == K).all()
