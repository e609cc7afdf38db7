"""Where ggnn_projective_sample writes: the call through the C ABI with every
input, every output (heads, log_prob, status, logz) and the workspace of
exactly ggnn_projective_sample_workspace_bytes an exact region of a guard arena
(tests/guard_arena.py; a size of 0 is a zero-length region), as
tests/test_gpu_guard_decode.py does for the other decoding calls.

Two batches (tests/guard_cases.py decode_batch's inputs at this call's tier):
graphs of n = 1, 2, P, P + 1 and v at v = P + 3, P = GGNN_PROJ_SAMPLE_LDS_MAXN,
so that the workspace has both tiers and its global part the fewest users; and
b = 1, v = 2.  K = 1 and K = GGNN_PROJ_SAMPLE_CHUNK + 1 (a second workgroup
and a second workspace slice per graph), single- and multi-root, logz given
and NULL.  Each call runs under pattern guards, NaN guards and on plain
allocations: no guard byte changes, the inputs stay as they were, and every
output is bit-identical across the three runs."""
import ctypes
import functools

import numpy as np
import pytest

import guard_arena as GA
from test_gpu_engine_edges import _torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000C0FFEE


@functools.lru_cache(maxsize=None)
def _batch(batch):
    """(probs float32 [b, v, v], n int32 [b]): decode_batch's softmax rows at
    this call's tier.  Read-only."""
    import tree_loss_cases as TL
    from ggnn_amd._lib import PROJ_SAMPLE_LDS_MAXN as P
    if batch == "tiny":
        v, n = 2, np.asarray([2], np.int32)
    else:
        v, n = P + 3, np.asarray([1, 2, P, P + 1, P + 3], np.int32)
    p, _ = TL.softmax_probs(len(n), v, v, 5)
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


def _call(mem, batch, K, single_root, with_logz):
    torch = _torch()
    from ggnn_amd import _lib
    lib = _lib.load()
    p_np, n_np = _batch(batch)
    b, v, o = p_np.shape
    i32, f32 = torch.int32, torch.float32
    d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def feed(name, a):
        t = mem.tensor(name, a.shape, {np.float32: f32, np.int32: i32}[a.dtype.type], a)
        mem.snapshot(name)
        return t

    p, n = feed("probs_head", p_np), feed("n_nodes", n_np)
    ws = mem.region("ws", int(lib.ggnn_projective_sample_workspace_bytes(b, v, K)))
    if batch == "tiers":
        assert ws.numel() == b * -(-K // _lib.PROJ_SAMPLE_CHUNK) * 8 * v * (v + 1) > 0    # the global tier is in the launch
    out = {"heads": mem.tensor("heads", (b, K, v), i32), "log_prob": mem.tensor("log_prob", (b, K), f32),
           "status": mem.tensor("status", (b, K), i32), "logz": mem.tensor("logz", (b,), f32) if with_logz else None}
    _lib.check(lib.ggnn_projective_sample(ctypes.byref(d), P(p), o, P(n), single_root, K, SEED, P(out["heads"]),
                                          P(out["log_prob"]), P(out["status"]), P(out["logz"]), P(ws), ws.numel(), s),
               "ggnn_projective_sample")
    return out


@pytest.mark.parametrize("with_logz", [True, False], ids=["logz", "nologz"])
@pytest.mark.parametrize("single_root", [1, 0], ids=["single", "multi"])
@pytest.mark.parametrize("many", [False, True], ids=["K1", "Kchunk+1"])
@pytest.mark.parametrize("batch", ["tiers", "tiny"])
def test_sampler_writes_inside_its_buffers(batch, many, single_root, with_logz):
    from ggnn_amd import evaluation as E
    from ggnn_amd._lib import PROJ_SAMPLE_CHUNK
    K = PROJ_SAMPLE_CHUNK + 1 if many else 1
    res = GA.run_guarded(lambda mem: _call(mem, batch, K, single_root, with_logz), _torch().device("cuda", 0), 16 << 20)
    p, n = _batch(batch)
    st = res["status"]
    # the batch does what it is for: the one-word graph passes through, every
    # other graph (softmax rows: every arc allowed) is drawn at both tiers
    assert (st[n < 2] == 0).all() and (st[n >= 2] == 1).all(), st
    for g, s in np.argwhere(st == 1):
        h = res["heads"][g, s]
        assert E.is_tree(h, int(n[g]), bool(single_root)) and E.is_projective(h, int(n[g])), (g, s)
        assert (h[int(n[g]):] == -1).all() and np.isfinite(res["log_prob"][g, s])
    assert (res["heads"][n < 2] == -1).all() and (res["log_prob"][n < 2] == -np.inf).all()
    if with_logz:
        assert (res["logz"][n < 2] == 0).all() and np.isfinite(res["logz"]).all()
