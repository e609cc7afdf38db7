"""The life of a captured step (ggnn_amd/graphs.py, model._graph_step) against
the eager step: distinct batches through one graph, stale edge rows and empty
edge lists, back-to-back replays, the edge capacity, eviction and recapture,
train and eval graphs of one shape, checkpoints into live graphs, the host
scalars a capture bakes, the reduction branch, and the float64 oracle on a
replay.

The oracle of every case but the last is the eager twin (graph_cases.py): the
same model with hip_graphs off, fed the same batches, compared with
torch.equal after every step.  All training feeds have the four dropouts on.
"""
import numpy as np
import pytest

from decode_cases import _synthetic_model, _torch
from graph_cases import (BATCH, V_A, assert_same_outputs, assert_same_state, lifecycle_feeds, lifecycle_raw, model_pair,
                         n_edges, outputs, train_both)

pytestmark = pytest.mark.gpu

BOTH_PATHS = pytest.mark.parametrize("hidden", [64, 128])   # the general path / the specialised kernels


def _stats(m, *keys):
    return tuple(m.graph_stats[k] for k in keys)


# ------------------------------------------------------------------ case 1
@BOTH_PATHS
def test_distinct_batches_through_one_graph(hidden):
    """Four different batches of one shape: eager, capture, two replays, the
    batch with the most edges followed by the one with the fewest."""
    _torch()
    ea, gr = model_pair(hidden)
    F = lifecycle_feeds(ea)
    assert n_edges(F.A4[1]) > n_edges(F.A4[0]) > n_edges(F.A4[2]) and n_edges(F.A4[3]) > n_edges(F.A4[2])
    for k, f in enumerate(F.A4):
        train_both(ea, gr, f, k)
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (1, 1, 3, 0), gr.graph_stats


# ------------------------------------------------------------------ case 2
def test_stale_edge_rows_and_empty_edge_lists():
    """StepLayout.fill writes only the batch's own rows, so after the batch
    with the most edges the device buffer keeps its rows: replays with no
    edges at all, with one graph's edges gone, and the full batch again read
    only the rows the offsets delimit."""
    _torch()
    ea, gr = model_pair()
    F = lifecycle_feeds(ea)
    a = F.a_max
    none = dict(a, adjacency_edges=[[] for _ in a["adjacency_edges"]])
    one = dict(a, adjacency_edges=[[] if i == 2 else g for i, g in enumerate(a["adjacency_edges"])])
    for k, f in enumerate([F.a_min, a, none, one, a]):
        train_both(ea, gr, f, k)
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (1, 1, 4, 0), gr.graph_stats


# ------------------------------------------------------------------ case 3
@BOTH_PATHS
def test_back_to_back_steps_and_output_aliasing(hidden):
    """Six different batches without a synchronisation between them (the two
    pinned staging buffers and the one device input buffer in flight), and
    the aliasing contract of train_step: what a replay returns is the graph's
    static output, overwritten by the next replay of the shape."""
    torch = _torch()
    ea, gr = model_pair(hidden)
    F = lifecycle_feeds(ea)
    six = F.A[:6]
    ref = [outputs(ea, ea.train_step(dict(f))) for f in six]
    torch.cuda.synchronize()
    handles, clones, later = [], [], []
    for f in six:
        loss = gr.train_step(dict(f))
        if handles:          # the previous step's un-cloned handles, as they read after this step
            later.append([h.detach().clone() for h in handles[-1]])
        handles.append([loss, gr.ops["computed_values"], gr.ops["computed_values_edges"]])
        clones.append(outputs(gr, loss))
    torch.cuda.synchronize()
    for k in range(6):
        assert_same_outputs(ref[k], clones[k], k)
    assert_same_state(ea, gr, "after six")
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (1, 1, 5, 0), gr.graph_stats
    # steps 1..5 are replays of one graph: step k's handle holds step k + 1's values
    for k in range(1, 5):
        assert_same_outputs(clones[k + 1], later[k], ("alias", k))
        for h0, h1 in zip(handles[k], handles[k + 1]):
            assert h0.data_ptr() == h1.data_ptr()
        assert not torch.equal(clones[k][1], clones[k + 1][1])


# ------------------------------------------------------------------ case 4
def _padded(feed, total):
    """``feed`` with graph 0's edge list padded to ``total`` edges in the
    batch by copies of its own first edge: the same adjacency."""
    g = [list(x) for x in feed["adjacency_edges"]]
    g[0] = g[0] + [g[0][0]] * (total - n_edges(feed))
    out = dict(feed, adjacency_edges=g)
    assert n_edges(out) == total
    return out


def test_edge_capacity_boundary():
    """b * v edges run captured, b * v + 1 fall back to the eager step (seeds
    and the Adam step drawn once); both equal the eager twin, and the
    un-padded batch on a second pair of models."""
    _torch()
    ea, gr = model_pair()
    ea3, gr3 = model_pair()
    F = lifecycle_feeds(ea)
    x, cap = F.A[2], BATCH * V_A
    padded = [F.A[0], F.A[1], _padded(x, cap), _padded(x, cap + 1), F.A[3]]
    plain = [F.A[0], F.A[1], x, x, F.A[3]]
    expect = [(1, 0, 0, 0), (1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 2, 1), (1, 1, 3, 1)]
    for k, (fp, f) in enumerate(zip(padded, plain)):
        o = train_both(ea, gr, fp, k)
        assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == expect[k], (k, gr.graph_stats)
        o3 = train_both(ea3, gr3, f, (k, "plain"))
        assert_same_outputs(o3, o, (k, "padded against plain"))
        assert_same_state(ea3, ea, (k, "padded against plain"))
        assert gr.optimizer.t == k + 1
        if k == 3:
            # the eager step's engine counts an over-long list without its
            # repeats, so the padded batch runs the path of the plain one
            assert ea._engine("main").sparse and gr._engine("main").sparse
    assert gr3.graph_stats["eager"] == 0


# ------------------------------------------------------------------ case 5
def _step_bytes(hidden, F):
    """CapturedStep.nbytes() of the two shapes on a warm-up model, after the
    first (eager) run and after the capture."""
    torch = _torch()
    m = _synthetic_model(True, hidden)
    out = {}
    for name, fs in (("A", F.A), ("B", F.B)):
        m.train_step(dict(fs[0]))
        first = next(reversed(m._graphs.values())).nbytes()
        m.train_step(dict(fs[1]))
        cs = next(reversed(m._graphs.values()))
        assert cs.graph is not None
        out[name] = (first, cs.nbytes())
    torch.cuda.synchronize()
    assert m.graph_stats["evicted"] == 0
    return out


def _one_step_budget(hidden, F):
    """A cache budget (bytes) that holds either shape's captured step, and
    not one of them beside the other's step of any age: the larger step plus
    half of the smaller step's size before its capture.  (Not the larger step
    to the byte: pool_bytes is memory_allocated across the capture, which
    also sees the previous step's outputs freed, in blocks whose sizes follow
    the allocator's state, so nbytes() of one shape differs by some 512-byte
    blocks from model to model; 1024 B were seen.)"""
    sz = _step_bytes(hidden, F)
    budget = max(sz["A"][1], sz["B"][1]) + min(sz["A"][0], sz["B"][0]) // 2
    assert sz["A"][1] + sz["B"][0] > budget + 2 ** 16 and sz["B"][1] + sz["A"][0] > budget + 2 ** 16, sz
    assert budget > max(sz["A"][1], sz["B"][1]) + 2 ** 16
    return budget, sz


@BOTH_PATHS
def test_eviction_and_recapture(hidden):
    """A cache that holds one step: A A A B B B A A A B B B releases and
    recaptures a step at every change of shape, every step equal to the eager
    one; then five more cycles, over which the device memory in use may not
    grow (CapturedStep.release returns the graph's private pool)."""
    torch = _torch()
    F = lifecycle_feeds()
    budget, sz = _one_step_budget(hidden, F)
    ea, gr = model_pair(hidden, hip_graph_cache_mb=budget / 2 ** 20)
    A, B = F.A, F.B
    seq = [A[0], A[1], A[2], B[0], B[1], B[0], A[3], A[4], A[5], B[1], B[0], B[1]]
    for k, f in enumerate(seq):
        train_both(ea, gr, f, k)
        assert gr.graph_stats["cache_bytes"] <= budget, (k, gr.graph_stats, budget)
        assert sum(cs.nbytes() for cs in gr._graphs.values()) <= budget, k
        assert len(gr._graphs) == 1
    # every change of shape evicts the other shape's step after the new one's
    # first (eager) run; the second batch captures again
    st = gr.graph_stats
    assert (st["uncaptured"], st["captured"], st["replayed"], st["evicted"], st["eager"]) == (4, 4, 8, 3, 0), st
    # the evicted graphs' pools are returned: the same cycle again and again
    mem = []
    for c in range(5):
        for f in [A[c], A[c + 1], A[0], B[c % 2], B[1 - c % 2], B[0]]:
            gr.train_step(dict(f))
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
        assert gr.graph_stats["cache_bytes"] <= budget
    print("hidden %d: step bytes %s, budget %d, memory_allocated after each cycle %s" % (hidden, sz, budget, mem))
    assert mem[-1] - mem[1] <= max(sz["A"][1], sz["B"][1]), mem
    assert gr.graph_stats["evicted"] == 3 + 10 and gr.graph_stats["captured"] == 4 + 10, gr.graph_stats


def test_run_epoch_fetches_an_evicted_steps_outputs(monkeypatch):
    """run_epoch keeps one batch in flight: the fetch of a batch's
    probabilities is still pending when the next batch, of another shape,
    evicts the step that produced them."""
    _torch()
    from ggnn_amd.graphs import CapturedStep
    released = []                   # per eviction: whether the step had a graph
    release = CapturedStep.release

    def counted(self):
        released.append(self.graph is not None)
        release(self)
    monkeypatch.setattr(CapturedStep, "release", counted)
    F = lifecycle_feeds()
    budget, _ = _one_step_budget(64, F)
    ea, gr = model_pair(hip_graph_cache_mb=budget / 2 ** 20)
    data = []
    for m in (ea, gr):          # (one copy per model: run_epoch shuffles its buckets in place)
        np.random.seed(0)
        data.append(m.process_raw_graphs(lifecycle_raw(), True))
    for epoch in range(2):
        res = []
        for m, d in zip((ea, gr), data):
            np.random.seed(epoch + 1)
            res.append(m.run_epoch("epoch", d, True))
        ra, rb = res
        assert ra[0] == rb[0] and ra[4] == rb[4] and ra[9] == rb[9]
        for i in (8, 14):       # computed_values, computed_values_edges, batch by batch
            assert len(ra[i]) == len(rb[i]) == ra[4]
            for k, (xa, xb) in enumerate(zip(ra[i], rb[i])):
                assert np.array_equal(xa, xb), (epoch, i, k)
    st = gr.graph_stats
    assert st["captured"] > 0 and st["evicted"] == len(released) and st["eager"] == 0, st
    assert any(released), released              # a captured step was evicted, its fetch in flight
    assert st["cache_bytes"] <= budget
    assert_same_state(ea, gr, "after two epochs")


# ------------------------------------------------------------------ case 6
def test_train_and_eval_interleaved_at_one_shape():
    """An eval replay packs the weights inside its graph: it must see what
    the training replay before it wrote."""
    torch = _torch()
    ea, gr = model_pair()
    F = lifecycle_feeds(ea)
    a0, a1, a2 = F.A[:3]
    for rep in range(3):        # from the second pass on, both graphs are replays
        train_both(ea, gr, a0, (rep, 0))
        sa = ea.evaluate_batch(dict(a1), on_device=True)
        la = ea.ops["loss"].detach().clone()
        sb = gr.evaluate_batch(dict(a1), on_device=True)
        assert torch.equal(la, gr.ops["loss"].detach()), (rep, float(la), float(gr.ops["loss"]))
        assert sa == sb, (rep, sa, sb)
        train_both(ea, gr, a1, (rep, 1))
        pa, pb = ea.predict_batch(dict(a2)), gr.predict_batch(dict(a2))
        for key in ("heads", "labels", "n_nodes"):
            assert np.array_equal(pa[key], pb[key]), (rep, key)
        assert (pa["heads"] >= 0).any()
        train_both(ea, gr, a2, (rep, 2))
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (2, 2, 13, 0), gr.graph_stats


# ------------------------------------------------------------------ case 7
def test_checkpoint_into_live_graphs(tmp_path):
    """restore_progress copies in place into the variables and Adam slots a
    live graph holds by address, and the restored step count reaches the
    replay through StepInputs.step; make_optimizer drops every captured step."""
    torch = _torch()
    ea, gr = model_pair()
    A = lifecycle_feeds(ea).A
    path = str(tmp_path / "live.pickle")
    for k in range(3):
        train_both(ea, gr, A[k], k)
    gr.save_progress(path, 3, 1)
    saved = [t.detach().clone() for t in gr.trainable_variables() + gr.optimizer.m + gr.optimizer.v]
    for k in (3, 4):
        train_both(ea, gr, A[k], k)
    assert not torch.equal(saved[0], gr.trainable_variables()[0].detach())
    for m in (gr, ea):
        assert m.restore_progress(path) == (3, 1)
        assert m.optimizer.t == 3
        for s, t in zip(saved, m.trainable_variables() + m.optimizer.m + m.optimizer.v):
            assert torch.equal(s, t.detach())
    for k in range(3):
        train_both(ea, gr, A[5 - k], ("restored", k))
        assert gr.optimizer.t == ea.optimizer.t == 3 + k + 1
    # the graph captured before the checkpoint served every step since
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (1, 1, 7, 0), gr.graph_stats
    for m in (ea, gr):
        m.make_optimizer()
    assert len(gr._graphs) == 0
    expect = [(2, 1, 7), (2, 2, 8), (2, 2, 9)]
    for k in range(3):
        train_both(ea, gr, A[k], ("new optimizer", k))
        assert gr.optimizer.t == k + 1
        assert _stats(gr, "uncaptured", "captured", "replayed") == expect[k], (k, gr.graph_stats)


# ------------------------------------------------------------------ case 8
def _halve_lr(m):
    m.optimizer.lr *= 0.5


def _set_clip(m):
    m.optimizer.clip = 0.25


def _more_timesteps(m):
    m.params["num_timesteps"] = 3


@pytest.mark.parametrize("change", [_halve_lr, _set_clip, _more_timesteps], ids=lambda f: f.__name__.strip("_"))
def test_host_scalars_changed_after_a_capture(change):
    """optimizer.lr / clip go by value into the captured Adam launch and
    num_timesteps into the propagation's: after a change the captured model
    must not replay the old values (they are part of the step's key)."""
    torch = _torch()
    ea, gr = model_pair()
    ct = _synthetic_model(False)             # a control that is never changed
    A = lifecycle_feeds(ea).A
    for k in range(3):                       # eager, capture, replay
        train_both(ea, gr, A[k], k)
        ct.train_step(dict(A[k]))
    for m in (ea, gr):
        change(m)
    for k in range(3, 6):
        train_both(ea, gr, A[k], ("changed", k))
        ct.train_step(dict(A[k]))
        # (the change is no no-op: the control's variables move differently)
        assert any(not torch.equal(x.detach(), y.detach())
                   for x, y in zip(ct.trainable_variables(), ea.trainable_variables())), k
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (2, 2, 4, 0), gr.graph_stats


def test_optimizer_params_are_read_by_make_optimizer_only():
    """params['clamp_gradient_norm'] and ['learning_rate'] are read when the
    optimizer is made: changing them alone changes nothing, on either path."""
    _torch()
    ea, gr = model_pair()
    ct = _synthetic_model(False)                 # the control: never changed
    A = lifecycle_feeds(ea).A
    for k in range(3):
        train_both(ea, gr, A[k], k)
        ct.train_step(dict(A[k]))
    for m in (ea, gr):
        m.params["clamp_gradient_norm"] = 0.25
        m.params["learning_rate"] = 0.0015
    for k in range(3, 6):
        train_both(ea, gr, A[k], ("changed", k))
        ct.train_step(dict(A[k]))
        assert_same_state(ct, gr, ("control", k))
    assert _stats(gr, "uncaptured", "captured", "replayed", "eager") == (1, 1, 5, 0), gr.graph_stats


# ------------------------------------------------------------------ case 9
def test_reduction_branch_on_one_gpu():
    """train_step(all_reduce=f, grad_scale=0.5) with a plain callable f that
    doubles the step's flat buffer in place: the captured step ends before
    Adam, and the reduction and Adam follow eagerly.  Scaling by 2 and 0.5 is
    exact in fp32, so the step equals a plain one on a third model.

    f scales the tables' squared lookup norms by 4, not 2: they are squares,
    and clip_by_norm of a doubled gradient reads a squared norm four times as
    large.  With those slots only doubled, 0.5 ** 2 * 2 = half the squared
    norm reaches the clip, and a table whose lookup norm exceeds the clip norm
    is clipped by sqrt(2) less than in the plain step (here the squared norms
    are 12.1, 3.1 and 9.4 against a clip norm of 1): the two steps then differ
    by design, as a union of two equal batches does from one batch under the
    reference's IndexedSlices norm."""
    torch = _torch()
    ea, gr = model_pair()
    plain = _synthetic_model(True)
    fl = plain.train_buffer()
    lo, n_sq = fl.sq.storage_offset(), fl.sq.numel()     # (the layout is the same on the three models)

    def double(t):
        t.mul_(2)
        t[lo:lo + n_sq].mul_(2)
        return t

    back = torch.full_like(fl.flat, 0.5)
    back[lo:lo + n_sq] = 0.25
    A = lifecycle_feeds(ea).A
    for k in range(3):                           # the plain key: eager, capture, replay
        train_both(ea, gr, A[k], k)
        plain.train_step(dict(A[k]))
    assert _stats(gr, "uncaptured", "captured", "replayed") == (1, 1, 2)
    expect = [(2, 1, 2), (2, 2, 3), (2, 2, 4)]   # another key: eager, capture, replay
    for k in range(3, 6):
        loss2 = train_both(ea, gr, A[k], ("reduced", k), all_reduce=double, grad_scale=0.5)[0]
        assert _stats(gr, "uncaptured", "captured", "replayed") == expect[k - 3], (k, gr.graph_stats)
        loss = plain.train_step(dict(A[k])).detach().clone()
        torch.cuda.synchronize()
        assert float(fl.sq.max()) > plain.optimizer.clip ** 2      # the tables are clipped: the norms matter
        assert torch.equal(loss2, 2 * loss), (k, float(loss2), float(loss))
        assert torch.equal(gr.train_buffer().flat * back, fl.flat), k
        for i, (x, y) in enumerate(zip(gr.trainable_variables() + gr.optimizer.m + gr.optimizer.v,
                                       plain.trainable_variables() + plain.optimizer.m + plain.optimizer.v)):
            assert torch.equal(x.detach(), y.detach()), (k, i)
        assert gr.optimizer.t == plain.optimizer.t == k + 1
    assert gr.graph_stats["eager"] == 0 and len(gr._graphs) == 2


# ----------------------------------------------------------------- case 10
@BOTH_PATHS
def test_replay_matches_the_float64_oracle(hidden):
    """The third batch of a shape, a replay with every dropout on: the loss,
    every gradient and the lookup norms against oracle/ggnn_oracle.py at the
    eager step's tolerance (test_gpu_heads.TOL).  Adam is covered by the
    equality with the eager step."""
    _torch()
    from test_gpu_heads import _check_train_step
    gr = _synthetic_model(True, hidden)
    A = lifecycle_feeds(gr).A
    gr.train_step(dict(A[0]))
    gr.train_step(dict(A[1]))
    before = gr.graph_stats["replayed"]
    _check_train_step(gr, dict(A[2]), adam=False)
    assert gr.graph_stats["replayed"] == before + 1 and gr.graph_stats["eager"] == 0
