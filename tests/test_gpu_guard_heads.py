"""Where the callers either side of the propagation path write:
ggnn_embed_forward, ggnn_embed_backward_ws (shared tables, sq_out),
ggnn_embed_lookup_rows, ggnn_embed_backward (its fp32 atomics: the guards and
the inputs only), ggnn_heads_forward, ggnn_heads_forward_dev,
ggnn_heads_backward, ggnn_heads_backward_dev, ggnn_heads_decode and the clip +
Adam step on flat buffers (ggnn_adam_step, ggnn_adam_step_dev), with every input, output and
workspace an exact region of a guard arena (tests/guard_arena.py), on the edge
shapes of tests/test_gpu_heads_edges.py, tests/test_gpu_embed_edges.py and
tests/test_gpu_optim.py (tests/guard_cases.py lists them).

Each sequence runs under pattern guards, NaN guards and on plain allocations:
no guard byte changes, the inputs stay as they were, every output is
bit-identical across the three runs, and the embedding workspace, whose
contract is "zero-filled before and after", is zero in every byte afterwards.
"""
import ctypes

import numpy as np
import pytest

import guard_arena as GA
import guard_cases as GC
import test_gpu_embed_edges as EE
import test_gpu_heads_edges as HE
from test_gpu_engine_edges import _torch

pytestmark = pytest.mark.gpu

KEEP, SEED = 0.85, 99


def _dev():
    return _torch().device("cuda", 0)


def _feeder(mem):
    torch = _torch()
    kinds = {np.float32: torch.float32, np.int32: torch.int32, np.int64: torch.int64}

    def feed(name, a):
        a = np.asarray(a)
        t = mem.tensor(name, a.shape, kinds[a.dtype.type], a)
        mem.snapshot(name)
        return t
    return feed


# ------------------------------------------------------------------- heads
def _heads_sequence(mem, b, v, h, os_):
    torch = _torch()
    from ggnn_amd import _lib
    from ggnn_amd.heads import OutputHeads
    f32 = torch.float32
    feed = _feeder(mem)
    tn = float(b) + 1e-7
    hT_np, h0_np, heads_np, _ = HE._inputs(b, v, h, os_, seed=b * v * 1000 + h + len(os_), spread=False)
    hT, h0 = feed("hT", hT_np), feed("h0", h0_np)
    heads = [(feed("W.%d" % i, hd["W"]), feed("bias.%d" % i, hd["b"])) for i, hd in enumerate(heads_np)]
    labels = [feed("labels.%d" % i, hd["labels"]) for i, hd in enumerate(heads_np)]
    tn_dev = feed("target_num", np.asarray([tn], np.float32))
    d_loss = feed("d_loss", np.asarray([HE.D_LOSS], np.float32))
    oh = OutputHeads(h)
    ws = oh._ws = mem.region("ws", GC.heads_workspace_bytes(_lib.load(), b, v, h, os_))
    out = {}
    for tag, target in (("", tn), (".dev", tn_dev)):       # ggnn_heads_forward, ggnn_heads_forward_dev
        probs = [mem.tensor("probs%s.%d" % (tag, i), (b, v, o), f32) for i, o in enumerate(os_)]
        loss = mem.tensor("loss" + tag, (len(os_),), f32)
        oh.forward(hT, h0, heads, labels, KEEP, SEED, target, loss_out=loss, probs_out=probs)
        assert oh._ws is ws
        out["loss" + tag] = loss
        out.update(("probs%s.%d" % (tag, i), p) for i, p in enumerate(probs))
    for i in range(len(os_)):
        mem.snapshot("probs.dev.%d" % i)                    # the backward reads them
    dws = [mem.tensor("dW.%d" % i, (2 * h, o), f32) for i, o in enumerate(os_)]
    dbs = [mem.tensor("db.%d" % i, (o,), f32) for i, o in enumerate(os_)]
    out["dhT"], out["dh0"] = mem.tensor("dhT", (b, v, h), f32), mem.tensor("dh0", (b, v, h), f32)
    oh.backward(hT, h0, heads, labels, probs, tn, d_loss=d_loss, dws=dws, dbs=dbs, dhT=out["dhT"], dh0=out["dh0"])
    assert oh._ws is ws
    out.update(("dW.%d" % i, t) for i, t in enumerate(dws))
    out.update(("db.%d" % i, t) for i, t in enumerate(dbs))
    # ggnn_heads_backward_dev: the same from the device target_num, into buffers of its own
    dws2 = [mem.tensor("dW.dev.%d" % i, (2 * h, o), f32) for i, o in enumerate(os_)]
    dbs2 = [mem.tensor("db.dev.%d" % i, (o,), f32) for i, o in enumerate(os_)]
    out["dhT.dev"], out["dh0.dev"] = mem.tensor("dhT.dev", (b, v, h), f32), mem.tensor("dh0.dev", (b, v, h), f32)
    oh.backward(hT, h0, heads, labels, probs, tn_dev, d_loss=d_loss, dws=dws2, dbs=dbs2, dhT=out["dhT.dev"],
                dh0=out["dh0.dev"])
    out.update(("dW.dev.%d" % i, t) for i, t in enumerate(dws2))
    out.update(("db.dev.%d" % i, t) for i, t in enumerate(dbs2))
    return out


@pytest.mark.parametrize("b,v,h,os_", GC.HEADS_SHAPES)
def test_heads_write_inside_their_buffers(b, v, h, os_):
    res = GA.run_guarded(lambda mem: _heads_sequence(mem, b, v, h, os_), _dev(), GC.CAPACITY)
    # the device target_num gives the host value's bits (include/ggnn.h)
    assert np.array_equal(res["loss"], res["loss.dev"]) and np.isfinite(res["loss"]).all()
    for i in range(len(os_)):
        assert np.array_equal(res["probs.%d" % i], res["probs.dev.%d" % i]), i
        assert np.array_equal(res["dW.%d" % i], res["dW.dev.%d" % i]), i
        assert np.array_equal(res["db.%d" % i], res["db.dev.%d" % i]), i
    assert np.array_equal(res["dhT"], res["dhT.dev"]) and np.array_equal(res["dh0"], res["dh0.dev"])


def _node_counts(b, v):
    import tree_loss_cases as TL
    return TL.uneven_counts(b, v)


def _decode_sequence(mem, b, v, o, oe):
    torch = _torch()
    import tree_loss_cases as TL
    from ggnn_amd import _lib
    feed = _feeder(mem)
    rng = np.random.default_rng(b * 100 + v + o)
    n_np = TL.uneven_counts(b, v)
    p_h, _ = TL.softmax_probs(b, v, o, 3)
    p_l, _ = TL.softmax_probs(b, v, oe, 4)
    y_h = np.stack([TL.chain_gold(int(m), v, o) for m in n_np])
    y_l = np.zeros((b, v, oe), np.float32)
    y_l.reshape(b * v, oe)[np.arange(b * v), rng.integers(0, oe, b * v)] = 1.0
    ins = [feed(k, a) for k, a in (("probs_head", p_h), ("probs_label", p_l), ("gold_head", y_h), ("gold_label", y_l),
                                   ("n_nodes", n_np))]
    out = {"pred": mem.tensor("pred", (b, v, 2), torch.int32), "gold": mem.tensor("gold", (b, v, 2), torch.int32),
           "counts": mem.tensor("counts", (b, _lib.DECODE_COUNTS), torch.int32)}
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
    _lib.check(_lib.load().ggnn_heads_decode(ctypes.byref(d), P(ins[0]), o, P(ins[1]), oe, P(ins[2]), P(ins[3]),
                                             P(ins[4]), P(out["pred"]), P(out["gold"]), P(out["counts"]),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "ggnn_heads_decode")
    return out


@pytest.mark.parametrize("b,v,o,oe", GC.DECODE_HEAD_SHAPES)
def test_heads_decode_writes_inside_its_buffers(b, v, o, oe):
    res = GA.run_guarded(lambda mem: _decode_sequence(mem, b, v, o, oe), _dev(), 16 << 20)
    assert (res["pred"][:, 0] == -1).all() and (res["gold"][:, 0] == -1).all()      # row 0 by the contract
    assert (res["counts"][:, 0] == np.maximum(_node_counts(b, v) - 1, 0)).all()          # n_kept: the gold chain's words


# --------------------------------------------------------------- embedding
def _embed_sequence(mem, layout, b, v, keep, oor):
    torch = _torch()
    from ggnn_amd import _lib
    from ggnn_amd.heads import EmbeddingFrontEnd
    f32 = torch.float32
    feed = _feeder(mem)
    c = EE.Case(torch, layout, b, v, seed=b * 100 + v, oor=oor)
    tables = [feed("table.%d" % i, t) for i, t in enumerate(c.tables)]
    segs = [(tables[ti], c.cols[s]) for s, ti in enumerate(c.seg_table)]
    wi, G, G2 = feed("word_inputs", c.wi.astype(np.int32)), feed("dh0", c.G), feed("dh0_add", c.G2)
    fe = EmbeddingFrontEnd(c.H, deterministic=True)
    assert fe.deterministic
    out = {"h0": fe.forward(segs, wi, keep, EE.BIG_SEED, out=mem.tensor("h0", (b, v, c.H), f32))}
    ws = out["ws"] = mem.region("ws", GC.embed_workspace_bytes(_lib.load(), layout))
    ws.zero_()                                  # the contract: zero-filled by the caller before its first use
    fe._ws[tuple((t.data_ptr(), tuple(t.shape)) for t, _ in segs)] = ws
    dts = [mem.tensor("dtable.%d" % i, t.shape, f32) for i, t in enumerate(c.tables)]
    out["sq"] = mem.tensor("sq", (len(segs),), f32)
    fe.backward(segs, wi, G, keep, EE.BIG_SEED, dh0_add=G2, dtables=[dts[ti] for ti in c.seg_table], sq_out=out["sq"])
    assert len(fe._ws) == 1
    out.update(("dtable.%d" % i, t) for i, t in enumerate(dts))
    seg = len(segs) - 1                         # the IndexedSlices of the last segment, cap past the batch
    cap = b * v + 3
    out["rows"] = mem.tensor("rows", (cap, c.tables[c.seg_table[seg]].shape[1]), f32)
    out["ids"] = mem.tensor("ids", (cap,), torch.int32)
    fe.lookup_rows(segs, seg, wi, G, keep, EE.BIG_SEED, out["rows"], out["ids"], dh0_add=G2)
    return out


@pytest.mark.parametrize("layout,b,v,keep,oor", GC.EMBED_CASES)
def test_embedding_writes_inside_its_buffers(layout, b, v, keep, oor):
    res = GA.run_guarded(lambda mem: _embed_sequence(mem, layout, b, v, keep, oor), _dev(), GC.CAPACITY)
    assert res["ws"].size > 0 and not res["ws"].any()       # (e) zero in every byte afterwards
    assert (res["ids"][b * v:] == -1).all() and not res["rows"][b * v:].any()


@pytest.mark.parametrize("layout,b,v,keep,oor", [GC.EMBED_CASES[i] for i in (1, 4, 5)])
def test_embedding_atomics_backward_writes_inside_its_buffers(layout, b, v, keep, oor):
    """ggnn_embed_backward adds fp32 atomics in whatever order they land: its
    bits differ from run to run, so of the properties only these are asked: no
    guard byte changes under either fill, the inputs stay as they were, the
    table gradients and norms are finite."""
    torch = _torch()
    from ggnn_amd.heads import EmbeddingFrontEnd
    for fill in GA.FILLS:
        mem = GA.Arena(_dev(), fill=fill, capacity=16 << 20)
        feed = _feeder(mem)
        c = EE.Case(torch, layout, b, v, seed=b * 100 + v, oor=oor)
        tables = [feed("table.%d" % i, t) for i, t in enumerate(c.tables)]
        segs = [(tables[ti], c.cols[s]) for s, ti in enumerate(c.seg_table)]
        wi, G, G2 = feed("word_inputs", c.wi.astype(np.int32)), feed("dh0", c.G), feed("dh0_add", c.G2)
        dts = [mem.tensor("dtable.%d" % i, t.shape, torch.float32) for i, t in enumerate(c.tables)]
        sq = mem.tensor("sq", (len(segs),), torch.float32)
        fe = EmbeddingFrontEnd(c.H, deterministic=False)
        fe.backward(segs, wi, G, keep, EE.BIG_SEED, dh0_add=G2, dtables=[dts[ti] for ti in c.seg_table], sq_out=sq)
        torch.cuda.synchronize()
        mem.check()
        assert all(mem.unchanged(k) for k in mem.snapshots())
        assert all(bool(torch.isfinite(t).all()) for t in dts + [sq]), fill


# -------------------------------------------------------------- clip + Adam
def _adam_sequence(mem, dev_step):
    torch = _torch()
    from ggnn_amd import _lib
    from ggnn_amd.optim import AdamTensor
    f32 = torch.float32
    feed = _feeder(mem)
    ns = GC.ADAM_FLAT
    total, offs = sum(ns), np.concatenate([[0], np.cumsum(ns)])
    rng = np.random.default_rng(17)
    flat = {"param": mem.tensor("param", (total,), f32, (rng.standard_normal(total) * 0.1).astype(np.float32)),
            "m": mem.tensor("m", (total,), f32, np.zeros(total, np.float32)),
            "v": mem.tensor("v", (total,), f32, np.zeros(total, np.float32))}
    # (norms on both sides of the clip: tensor i's gradient has norm 0.3 or 2 after grad_scale)
    g = np.concatenate([rng.standard_normal(n) for n in ns])
    for i, n in enumerate(ns):
        s = g[offs[i]:offs[i + 1]]
        s *= (0.3 if i % 2 else 2.0) / 0.5 / max(np.sqrt(np.sum(s * s)), 1e-30)
    grad = feed("grad", g.astype(np.float32))
    sq = feed("sqnorm", np.asarray([9.0], np.float32))      # the IndexedSlices norm of tensor 4
    scratch = mem.tensor("scratch", (len(ns) * GC.ADAM_SCRATCH_PER_TENSOR,), f32)
    step = feed("step", np.asarray([1], np.int64)) if dev_step else None
    tab = (AdamTensor * len(ns))()
    for i, n in enumerate(ns):
        at = lambda t: t.data_ptr() + 4 * int(offs[i])  # noqa: E731
        tab[i] = AdamTensor(at(flat["param"]), at(grad), at(flat["m"]), at(flat["v"]), n,
                            sq.data_ptr() if i == 4 else None)
    lib = _lib.load()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = ctypes.c_void_p(scratch.data_ptr())
    for t in (1, 2):
        if dev_step:
            _lib.check(lib.ggnn_adam_step_dev(tab, len(ns), 0.003, 0.9, 0.999, 1e-8, 1.0,
                                              ctypes.c_void_p(step.data_ptr()), 0.5, sp, s), "ggnn_adam_step_dev")
        else:
            _lib.check(lib.ggnn_adam_step(tab, len(ns), 0.003, 0.9, 0.999, 1e-8, 1.0, t, 0.5, sp, s), "ggnn_adam_step")
    return flat


@pytest.mark.parametrize("dev_step", [False, True])
def test_adam_writes_inside_its_flat_buffers(dev_step):
    res = GA.run_guarded(lambda mem: _adam_sequence(mem, dev_step), _dev(), 16 << 20)
    assert all(np.isfinite(a).all() for a in res.values()) and res["m"].all() and (res["v"] > 0).all()


def test_checker_sees_device_writes():
    GA.device_self_test(_dev())
