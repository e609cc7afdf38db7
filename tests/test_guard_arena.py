"""The guard arena (tests/guard_arena.py) on CPU tensors: the checker can fail
-- a stray byte at a region's end + 0, at start - 1, in the slack before the
next 256-byte boundary, in the last byte of the trailing guard, and a 16-byte
write straddling a region's end are each reported with the region, the side
and the offsets; a write inside a region is not -- and the case tables of the
GPU half (tests/guard_cases.py) reach every *_bytes function they are meant
to, with dims ggnn_check_dims accepts, inside the arenas' capacity.
"""
import ctypes

import numpy as np
import pytest
import torch

import guard_arena as GA
import guard_cases as GC


def _arena(fill="pattern", guard=4096):
    a = GA.Arena("cpu", guard=guard, fill=fill, capacity=1 << 17)
    a.region("first", 1000)
    a.region("mid", 300)
    a.region("empty", 0)
    a.tensor("last", (5, 7), torch.float32, np.arange(35, dtype=np.float32).reshape(5, 7))
    return a


def _stray(a, offset, n=1):
    """n bytes flipped at an arena offset: a torch store into memory the test owns."""
    a.buf[offset:offset + n] ^= 0x5A


def _report(a):
    with pytest.raises(GA.GuardError) as e:
        a.check()
    e = e.value
    assert e.region in str(e) and e.side in str(e)
    return e.region, e.side, e.first, e.last, e.count


# -------------------------------------------------------------- the layout
@pytest.mark.parametrize("fill", GA.FILLS)
def test_layout(fill):
    a = _arena(fill)
    ext = [a.extent(n) for n in a.names()]
    assert a.names() == ["first", "mid", "empty", "last"]
    assert [e - s for s, e in ext] == [1000, 300, 0, 140]              # the exact size asked
    assert ext[0][0] >= a.guard                                        # a guard before the first region
    for (s, e), (s2, _) in zip(ext, ext[1:]):
        assert s2 - e >= a.guard and e <= s2                           # never overlapping, a guard between
    assert all(s % GA.ALIGN == 0 for s, _ in ext)
    assert a.buf.data_ptr() % GA.ALIGN == 0                            # offsets are addresses mod 256
    assert a.total - ext[-1][1] >= a.guard + GA.TAIL                   # 1 MiB at the end
    # every byte outside the regions is guard: the gaps and the regions tile the arena
    covered = sum(b - s for s, b, _, _ in a.gaps()) + sum(e - s for s, e in ext)
    assert covered == a.total
    k = np.arange(a.total, dtype=np.int64)
    want = ((k * 131 + 89) & 0xFF).astype(np.uint8) if fill == "pattern" else np.full(a.total, 0xFF, np.uint8)
    got = a.buf.numpy().copy()
    s, e = a.extent("last")
    assert np.array_equal(got[s:e].view(np.float32), np.arange(35, dtype=np.float32))
    got[s:e] = want[s:e]
    assert np.array_equal(got, want)
    a.check()


def test_views_and_errors():
    a = _arena()
    r = a.region("bytes", 77)
    assert r.dtype == torch.uint8 and r.numel() == 77 and r.data_ptr() % GA.ALIGN == 0
    t = a.tensor("half", (3, 5), torch.float16)
    assert t.shape == (3, 5) and t.dtype == torch.float16 and t.is_contiguous()
    assert a.extent("half")[1] - a.extent("half")[0] == 30
    assert a.region("none", 0).numel() == 0
    with pytest.raises(ValueError):
        a.region("bytes", 1)
    with pytest.raises(ValueError):
        a.tensor("bad", (2,), torch.float32, np.zeros(3, np.float32))
    with pytest.raises(MemoryError):
        a.region("huge", 1 << 17)
    with pytest.raises(ValueError):
        GA.Arena("cpu", fill="zeros")
    bare = GA.Arena("cpu", guard=256, capacity=4096)                   # no region: all guard
    bare.check()
    bare.buf[10] ^= 1
    with pytest.raises(GA.GuardError) as e:
        bare.check()
    assert (e.value.region, e.value.first, e.value.count) == (None, 10, 1)
    assert GA.capacity_for([1000, 300, 0, 140], 4096) == a.extent("last")[1] + 4096 + (-(a.extent("last")[1] + 4096)) % 256


# ------------------------------------------------------- the checker fails
@pytest.mark.parametrize("fill", GA.FILLS)
def test_stray_writes_are_reported(fill):
    s, e = _arena(fill).extent("mid")
    slack_end = (e + GA.ALIGN - 1) // GA.ALIGN * GA.ALIGN
    cases = [
        (e, 1, ("mid", "after", 0, 0, 1)),                            # end + 0
        (s - 1, 1, ("mid", "before", -1, -1, 1)),                     # start - 1
        (slack_end - 1, 1, ("mid", "after", slack_end - 1 - e, slack_end - 1 - e, 1)),   # the slack's last byte
        (e - 8, 16, ("mid", "after", 0, 7, 8)),                       # 16 bytes straddling the end: 8 outside
        (s - 3, 16, ("mid", "before", -3, -1, 3)),                    # straddling the start
    ]
    for offset, n, want in cases:
        a = _arena(fill)
        a.check()
        _stray(a, offset, n)
        assert _report(a) == want, (offset, n)
    a = _arena(fill)
    _stray(a, a.total - 1)                                            # the last byte of the trailing guard
    end = a.extent("last")[1]
    assert _report(a) == ("last", "after", a.total - 1 - end, a.total - 1 - end, 1)
    a = _arena(fill)
    _stray(a, 0)                                                      # the first byte of the leading guard
    assert _report(a) == ("first", "before", -a.extent("first")[0], -a.extent("first")[0], 1)
    a = _arena(fill)
    z = a.extent("empty")[0]
    _stray(a, z)                                                      # a zero-length region owns no byte
    assert _report(a)[0] == "empty" and _report(a)[2:] == (0, 0, 1)


def test_first_last_and_count_of_a_scattered_write():
    a = _arena()
    e = a.extent("first")[1]
    for k in (5, 9, 300):
        _stray(a, e + k)
    assert _report(a) == ("first", "after", 5, 300, 3)


def test_writes_inside_regions_are_not_reported():
    for fill in GA.FILLS:
        a = _arena(fill)
        for name in a.names():
            s, e = a.extent(name)
            a.buf[s:e] = 0x11
        a.check()


def test_restoring_the_byte_passes_again():
    a = _arena()
    e = a.extent("mid")[1]
    _stray(a, e)
    with pytest.raises(GA.GuardError):
        a.check()
    _stray(a, e)
    a.check()


def test_snapshot_and_unchanged():
    a = _arena()
    a.snapshot("last")
    assert a.unchanged("last") and a.snapshots() == ["last"]
    s, _ = a.extent("last")
    a.buf[s + 4] ^= 1
    assert not a.unchanged("last")
    a.check()                                                         # (inside a region: no guard's business)


def test_plain_has_the_arena_interface():
    p = GA.Plain("cpu")
    t = p.tensor("x", (2, 3), torch.int32, np.arange(6, dtype=np.int32).reshape(2, 3))
    assert t.tolist() == [[0, 1, 2], [3, 4, 5]] and p.region("w", 0).numel() == 0
    p.snapshot("x")
    assert p.unchanged("x")
    t[0, 0] = 9
    assert not p.unchanged("x")
    p.check()


def test_run_guarded_on_cpu_tensors():
    """The three-run harness on a CPU 'kernel': a well-behaved one passes; one
    that stores past its output, one whose result depends on the bytes behind
    its input, and one that writes its input are each caught."""
    x = np.arange(10, dtype=np.float32)

    def kernel(mem, overrun=0, overread=False, clobber=False):
        a = mem.tensor("x", (10,), torch.float32, x)
        mem.snapshot("x")
        out = mem.tensor("y", (10,), torch.float32)
        out.copy_(a * 2)
        if isinstance(mem, GA.Arena):
            s, e = mem.extent("y")
            if overrun:
                mem.buf[e:e + overrun] = 0
            if overread:
                out[9] += float(mem.buf[mem.extent("x")[1]])
        if clobber:
            a[3] = -1.0
        return {"y": out}

    res = GA.run_guarded(kernel, "cpu", capacity=1 << 18)
    assert np.array_equal(res["y"], x * 2)
    with pytest.raises(GA.GuardError):
        GA.run_guarded(lambda m: kernel(m, overrun=4), "cpu", capacity=1 << 18)
    with pytest.raises(AssertionError, match="differs|depends"):
        GA.run_guarded(lambda m: kernel(m, overread=True), "cpu", capacity=1 << 18)
    with pytest.raises(AssertionError, match="read-only"):
        GA.run_guarded(lambda m: kernel(m, clobber=True), "cpu", capacity=1 << 18)


def test_device_self_test_runs_on_the_cpu():
    GA.device_self_test("cpu")


# ------------------------------------------------- the GPU half's case tables
def test_engine_cases_reach_the_size_functions(lib):
    """Every engine case gets a size from ggnn_adjacency_bytes,
    ggnn_weight_pack_bytes and ggnn_workspace_bytes (training and inference),
    its dims pass ggnn_check_dims (PropagationEngine.dims checks them), and
    its regions fit the arena."""
    import engine_edge_cases as EC
    from ggnn_amd import _lib
    names = {g.c.name for g in GC.ENGINE_CASES}
    want = {c.name for c in EC.TIER_CASES + EC.EXTRA_CASES + EC.EMPTY_CASES + EC.PAIR_CASES} - {"fused_maxt"}
    assert want | set(GC.LOCAL) == names and set(EC.DENSE_CHANNEL_CASES) <= names
    assert sum(g.batch_pack for g in GC.ENGINE_CASES) == sum(c.ek < 1.0 for c in EC.PAIR_CASES) > 0
    assert {g.precision for g in GC.ENGINE_CASES} == {"fp32", "fp16", "bf16"}
    for g in GC.ENGINE_CASES:
        c = g.c
        eng = GC.make_engine(g, device="cpu")
        plan, keys = GC.engine_plan(eng, g)
        sizes = dict(plan)
        assert list(sizes) == ["adjacency", "pack", "ws.train", "ws.inf"] and all(n > 0 for n in sizes.values()), g.id
        assert sizes["ws.train"] > sizes["ws.inf"], g.id             # the training workspace keeps the saves
        d = eng.dims(c.b, c.v, c.T, **{k: v for k, v in GC.dropout_of(c).items()})
        assert lib.ggnn_check_dims(ctypes.byref(d)) == 0, g.id
        assert bool(d.flags & _lib.GGNN_SPARSE_PAIRS) == eng.sparse == GC.uses_edges(c), g.id
        assert GA.capacity_for([n for _, n in plan] + GC.engine_typed_bytes(g)) <= GC.CAPACITY, g.id
        if g.batch_pack:        # the pack made for the staged batch is sized with the batch's dims
            assert c.ek < 1.0
    # the local rows are what their names say
    x = GC.engine_inputs("pair_full")
    c = GC.LOCAL["pair_full"]
    rows = {(gi,) + tuple(e) for gi in range(c.b) for e in x["edges"][x["offsets"][gi]:x["offsets"][gi + 1]].tolist()}
    assert x["edges"].shape[0] == c.b * c.v == len(rows)             # at capacity, no repeats
    assert [(c.b, c.v, c.h, c.C) for c in GC.LOCAL.values()][:3] == GC.RAGGED_HIDDEN
    assert all(GC.LOCAL["ragged_h%d" % h].ek < 1.0 and h % 4 for _, _, h, _ in GC.RAGGED_HIDDEN)
    assert GC.LOCAL["v150_dense"].v == GC.LOCAL["v150_pairs"].v == 150 > 128


def test_gemm_cases():
    assert {(M, N, K) for M, N, K, _, _ in GC.GEMM_CASES} == set(GC.GEMM_SHAPES)      # k_gemm takes every shape
    assert {k for _, _, _, k, _ in GC.GEMM_CASES} == set(GC.GEMM_KERNELS)
    for kern in (2, 3, 4, 5):
        shapes = {(M, N, K) for M, N, K, k, _ in GC.GEMM_CASES if k == kern}
        assert shapes == {(132, 260, 40), (28, 400, 88), (33, 148, 1000), (96, 32, 264)}, kern
    assert all(4 * (M * K + K * N + M * N) + 4 * 65536 < (8 << 20) for M, N, K in GC.GEMM_SHAPES)


def test_decode_cases_reach_the_size_functions(lib):
    """Every decode case gets its workspace size from the call's own
    ggnn_*_workspace_bytes: > 0 on the batch that crosses the LDS tier (the
    graphs of n = L + 1 and v use it, those of n <= L do not), 0 (a zero-length
    region; tree_loss: its n_eff slot alone) on the tiny one; ggnn_check_dims
    accepts the dims; the passes have work on the large graphs."""
    from ggnn_amd import _lib, evaluation as E
    for call, batch, sr in GC.DECODE_CASES:
        p, n, y, scores, pred, gold, counts = GC.decode_batch(call, batch)
        b, v, o = p.shape
        d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
        assert lib.ggnn_check_dims(ctypes.byref(d)) == 0
        ws = dict(GC.decode_workspaces(lib, call, b, v))
        L = GC.decode_lds_maxn(call)
        if batch == "tiers":
            assert v == L + 3 <= _lib.TREE_MAXV and n.tolist() == [1, 2, L, L + 1, v]
            assert (ws["ws"] > 0) == (call != "tree_decode"), call
            if call in ("tree_decode", "projective_decode"):
                assert not any(E.is_tree(pred[g, :, 0], int(n[g]), bool(sr)) for g in range(2, b))
        else:
            assert (b, v) == (1, 2) and ws["ws"] == (256 if call.startswith("tree_loss") else 0), call
        if call.startswith("tree_sample"):
            assert ws["ws"] == int(call[-1]) * ws["ws.marginals"]     # the sampler's grows with num_samples
        assert sum(ws.values()) + 6 * p.nbytes + 20 * 65536 <= (16 << 20)
    assert {int(c[-1]) for c in GC.DECODE_CALLS if c.startswith("tree_sample")} == {1, 3}
    assert {int(c[-1]) for c in GC.DECODE_CALLS if c.startswith("tree_loss")} == {0, 1}


def test_heads_cases_reach_the_size_functions(lib):
    from ggnn_amd import _lib
    assert any(b == 1 and any(o % 2 for o in os_) for b, v, h, os_ in GC.HEADS_SHAPES)
    for b, v, h, os_ in GC.HEADS_SHAPES:
        d = _lib.dims(b, v, h, 1, 1, True, "fp32")
        assert lib.ggnn_check_dims(ctypes.byref(d)) == 0
        n = GC.heads_workspace_bytes(lib, b, v, h, os_)
        ot = sum((o + 3) & ~3 for o in os_)
        assert n >= 4 * (2 * b * v * ot + 3 * 2 * h * ot)           # logits, dZ and the three weight-shaped parts
        typed = [4 * b * v * h] * 6 + [4, 4, 4 * len(os_), 4 * len(os_)]
        for o in os_:
            typed += [4 * b * v * o] * 3 + [4 * 2 * h * o, 4 * o] * 3
        assert GA.capacity_for([n] + typed) <= GC.CAPACITY, (b, v, h, os_)
    assert any(b == 1 for b, _, _, _ in GC.DECODE_HEAD_SHAPES) and all(v <= o for _, v, o, _ in GC.DECODE_HEAD_SHAPES)
    from test_gpu_embed_edges import LAYOUTS
    assert any(b == 1 for _, b, _, _, _ in GC.EMBED_CASES)
    for layout in {c[0] for c in GC.EMBED_CASES}:
        L = LAYOUTS[layout]
        n = GC.embed_workspace_bytes(lib, layout)
        assert n >= sum(8 * L["tables"][ti][0] * L["tables"][ti][1] for ti in L["segs"])   # the fixed-point copies
        for _, b, v, _, _ in [c for c in GC.EMBED_CASES if c[0] == layout]:
            nseg, width = len(L["segs"]), L["tables"][L["segs"][-1]][1]
            typed = ([4 * b * v * L["H"]] * 3 + [4 * b * v * (nseg + 1), 4 * nseg, 4 * (b * v + 3) * (width + 1)]
                     + [4 * r * w for r, w in L["tables"]] * 2)
            assert GA.capacity_for([n] + typed) <= GC.CAPACITY, (layout, b, v)
    assert all(n % 4 for n in GC.ADAM_FLAT) and 12 * 4 * sum(GC.ADAM_FLAT) <= (16 << 20)
