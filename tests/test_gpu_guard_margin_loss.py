"""Where ggnn_margin_loss writes: both families through the C ABI, with every
input, every output (marg, heads, value, hamming, status, used, loss[2]) and
the workspace of exactly ggnn_margin_loss_workspace_bytes an exact region of a
guard arena (tests/guard_arena.py).

The batches are the projective decoder's of tests/guard_cases.py decode_batch:
graphs of n = 1, 2, GGNN_PROJ_LDS_MAXN, GGNN_PROJ_LDS_MAXN + 1 and v at v =
GGNN_PROJ_LDS_MAXN + 3, so that the projective family's tables are in the
workspace for two graphs and in LDS for one; and b = 1, v = 2.  Single- and
multi-root, cost 1.  Each call runs under pattern guards, NaN guards and on
plain allocations: no guard byte changes, the inputs stay as they were, and
every output is bit-identical across the three runs.
"""
import ctypes

import numpy as np
import pytest

import guard_arena as GA
import guard_cases as GC
import tree_loss_cases as TL
from test_gpu_engine_edges import _torch

pytestmark = pytest.mark.gpu

CASES = [(family, batch, sr) for family in (0, 1) for batch in GC.DECODE_BATCHES for sr in (1, 0)]


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _call(mem, family, batch, single_root):
    torch = _torch()
    from ggnn_amd import _lib
    lib = _lib.load()
    p_np, n_np, y_np = GC.decode_batch("projective_decode", batch)[:3]
    b, v, o = p_np.shape
    i32, f32 = torch.int32, torch.float32
    d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def feed(name, a):
        t = mem.tensor(name, a.shape, {np.float32: f32, np.int32: i32}[a.dtype.type], a)
        mem.snapshot(name)
        return t

    n, p, y = feed("n_nodes", n_np), feed("probs_head", p_np), feed("gold_head", y_np)
    need = int(lib.ggnn_margin_loss_workspace_bytes(b, v, o, family))
    assert need >= 4 * b * v * o
    if batch == "tiers" and family == 1:
        assert need > 4 * b * v * o + 8 * b * v * (v + 1)          # the decoder's global-memory tier is in the launch
    ws = mem.region("ws", need)
    out = {"marg": mem.tensor("marg", (b, v, o), f32), "heads": mem.tensor("heads", (b, v), i32),
           "value": mem.tensor("value", (b,), f32), "hamming": mem.tensor("hamming", (b,), i32),
           "status": mem.tensor("status", (b,), i32), "used": mem.tensor("used", (b,), i32),
           "loss": mem.tensor("loss", (2,), f32, np.asarray([0.5, 0.25], np.float32))}
    _lib.check(lib.ggnn_margin_loss(ctypes.byref(d), _P(p), o, _P(y), _P(n), family, single_root, 1.0,
                                    float(TL.target_num_of(y_np)), _P(out["marg"]), _P(out["heads"]),
                                    _P(out["value"]), _P(out["hamming"]), _P(out["status"]), _P(out["used"]),
                                    _P(out["loss"]), _P(ws), ws.numel(), s), "ggnn_margin_loss")
    return out


@pytest.mark.parametrize("family,batch,single_root", CASES)
def test_margin_loss_writes_inside_its_buffers(family, batch, single_root):
    from ggnn_amd import evaluation as E
    res = GA.run_guarded(lambda mem: _call(mem, family, batch, single_root), _torch().device("cuda", 0), 16 << 20)
    p, n, y = GC.decode_batch("projective_decode", batch)[:3]
    # the batch does what it is for: every graph with two nodes or more is decoded and used, the one-word graph is
    # left alone, and the results are the host form's
    ref = E.margin_loss_arrays(p, y, n, family, bool(single_root), TL.target_num_of(y), 1.0)
    assert ref[6].tolist() == [int(m >= 2) for m in n] and np.array_equal(res["used"], ref[6])
    assert np.array_equal(res["status"], ref[5]) and np.array_equal(res["heads"], ref[2])
    assert np.array_equal(res["hamming"], ref[4]) and res["marg"].tobytes() == ref[1].tobytes()
    assert res["loss"][1] == np.float32(0.25)
    assert abs(float(res["loss"][0]) - (0.5 + ref[0])) <= 2.0 ** -22 * (0.5 + abs(ref[0]))
