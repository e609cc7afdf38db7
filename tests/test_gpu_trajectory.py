"""Every step of a short, mixed-shape training run of the drop-in model
against the float64 oracle (tests/trajectory_cases.py).

The schedule A0 B0 A1 B1 tail A2 EVAL(A3) B2 A0 CKPT tail A3 takes both full
shapes through uncaptured -> captured -> replayed with the other shape's steps
between the replays, an evaluate_batch and a checkpoint round trip into a
freshly built model between them.  After every entry the state is read back
and held to the oracle, teacher-forced: the gradients to oracle_step at the
variables the device had before the step, Adam to O.adam_step from the
device's own before-state with the device's own gradients and lookup norms
and the harness's own step count.  tests/test_trajectory_inputs.py shows, on
the host, ten faults these comparators reject and the earlier checks pass.

Run with -s for the table of worst errors per case.
"""
import numpy as np
import pytest

import trajectory_cases as TC
from decode_cases import _synthetic_model, _torch
from graph_cases import lifecycle_feeds
from trajectory_cases import CKPT, EVAL, LOC, POS, TRAIN, WORD, StepRecord

pytestmark = pytest.mark.gpu

_CACHE = {}


def _entries():
    """The schedule, built once per module (batching reads no weight)."""
    if "entries" not in _CACHE:
        _CACHE["entries"] = TC.schedule(lifecycle_feeds())
    return _CACHE["entries"]


def _snapshot(m):
    """(dict(vars, m, v), optimizer.t) as host copies; a model that has not
    stepped yet has no optimizer: zero slots, t = 0."""
    st = dict(vars=[p.detach().cpu().numpy().copy() for p in m.trainable_variables()])
    opt = m.optimizer
    for k in ("m", "v"):
        st[k] = ([np.zeros_like(x) for x in st["vars"]] if opt is None
                 else [x.detach().cpu().numpy().copy() for x in getattr(opt, k)])
    return st, (0 if opt is None else int(opt.t))


def _draws(m):
    return dict(embed=dict(m.last_embed), path=dict(m.last_dropout), heads=dict(m.last_heads))


def _train_entry(torch, m, i, e):
    before, t0 = _snapshot(m)
    loss = m.train_step(dict(e.feed))
    torch.cuda.synchronize()
    # host copies at once: the loss and, on a captured step, everything the
    # next replay of the shape writes (train_step's aliasing contract)
    params = m.trainable_variables()
    rec = StepRecord(i, TRAIN, e.name, e.feed, before=before, t_before=t0, loss=float(loss.detach()),
                     grads=[p.grad.detach().cpu().numpy().copy() for p in params],
                     sq=[np.float32(m.lookup_sqnorm[id(params[k])].cpu().numpy()[0]) for k in (LOC, POS, WORD)],
                     drop=_draws(m), graph_stats=dict(m.graph_stats))
    rec.after, rec.t_after = _snapshot(m)
    return rec


def _eval_entry(torch, m, i, e):
    before, t0 = _snapshot(m)
    flat = m.train_buffer().flat
    flat0 = flat.cpu().numpy().copy()
    scores = m.evaluate_batch(dict(e.feed))
    torch.cuda.synchronize()
    rec = StepRecord(i, EVAL, e.name, e.feed, before=before, t_before=t0, drop=_draws(m), scores=tuple(scores),
                     probs=[m.ops[k].detach().cpu().numpy().copy() for k in ("computed_values", "computed_values_edges")],
                     flat_before=flat0, flat_after=flat.cpu().numpy().copy(), graph_stats=dict(m.graph_stats))
    rec.after, rec.t_after = _snapshot(m)
    return rec


def _ckpt_entry(m, i, e, n_train, path, build):
    """save_progress, then restore_progress into a freshly built model, which
    takes over.  The fresh model is built with another constructor seed: one
    built with the same seed would draw the run's first Philox seeds again
    (its variables are all overwritten by the restore either way)."""
    before, t0 = _snapshot(m)
    m.save_progress(path, n_train, 0)
    m2 = build(seed=1)
    assert m2.optimizer is None
    assert m2.restore_progress(path) == (n_train, 0)
    rec = StepRecord(i, CKPT, e.name, None, before=before, t_before=t0, graph_stats=dict(m.graph_stats))
    rec.after, rec.t_after = _snapshot(m2)
    return rec, m2


def _run(entries, build, path, title):
    torch = _torch()
    m = build()
    h = TC.Harness(TC.spec_of(m))
    models, records = [m], []
    for i, e in enumerate(entries):
        if e.kind == TRAIN:
            rec = _train_entry(torch, m, i, e)
        elif e.kind == EVAL:
            rec = _eval_entry(torch, m, i, e)
        else:
            rec, m = _ckpt_entry(m, i, e, h.n_train, path, build)
            models.append(m)
        h.check(rec)
        records.append(rec)
    print("\n" + h.table(title))
    return models, records, h


# what each entry of the schedule adds to graph_stats with hip_graphs on: a
# shape's first batch runs uncaptured, its second is captured and replayed,
# later ones replay; the model restored at CKPT starts over
_U, _C, _R, _NONE = {"uncaptured": 1}, {"captured": 1, "replayed": 1}, {"replayed": 1}, {}
GRAPH_PATH = [_U, _U, _C, _C, _U, _R, _NONE, _R, _R, _NONE, _U, _U]


@pytest.mark.parametrize("hip_graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("hidden", [64, 128])     # the general path / the specialised kernels, fused forward
def test_trajectory_matches_the_oracle(hidden, hip_graphs, tmp_path):
    entries = _entries()
    build = lambda seed=0: _synthetic_model(hip_graphs, hidden, seed=seed)
    models, records, h = _run(entries, build, str(tmp_path / "trajectory.pickle"),
                              "hidden %d, hip_graphs %s" % (hidden, hip_graphs))
    assert h.n_train == 10 and len(models) == 2
    keys = ("uncaptured", "captured", "replayed", "eager", "evicted")
    prev = dict.fromkeys(keys, 0)
    for rec, e, want in zip(records, entries, GRAPH_PATH):
        if e.kind == CKPT:
            prev = dict.fromkeys(keys, 0)        # (the restored model's counters)
            continue
        got = {k: rec.graph_stats[k] - prev[k] for k in keys if rec.graph_stats[k] != prev[k]}
        if hip_graphs:
            assert got == want, (rec.index, e.name, got)
        else:
            assert got == ({"eager": 1} if e.kind == TRAIN else {}), (rec.index, e.name, got)
        prev = {k: rec.graph_stats[k] for k in keys}
    if hip_graphs:
        st = models[0].graph_stats
        assert (st["uncaptured"], st["captured"], st["replayed"], st["eager"]) == (3, 2, 5, 0), st
        st = models[1].graph_stats
        assert (st["uncaptured"], st["captured"], st["replayed"], st["eager"]) == (2, 0, 0, 0), st


def test_trajectory_dense_feed(tmp_path):
    """The first five training entries with compact_adjacency off: the feed
    carries the dense adjacency_matrix, which never runs as a captured step
    (model._graph_ok): train_step's eager body on the engine's dense staging
    (set_adjacency), at hidden 128."""
    from ggnn_amd.batching import graph_to_adj_mat_bd
    build = lambda seed=0: _synthetic_model(True, 128, seed=seed, compact_adjacency=False)
    E = 6                                   # num_edge_types of decode_cases._synthetic_model
    dense = lambda f: dict(f, adjacency_matrix=np.stack([graph_to_adj_mat_bd(g, f["num_vertices"], E)
                                                         for g in f["adjacency_edges"]]))
    entries = [TC.Entry(e.kind, e.name, dense(e.feed)) for e in _entries()[:5]]
    assert all(e.kind == TRAIN for e in entries)
    models, records, h = _run(entries, build, str(tmp_path / "unused.pickle"), "hidden 128, dense feed")
    st = models[0].graph_stats
    assert h.n_train == 5 and (st["eager"], st["uncaptured"], st["captured"], st["replayed"]) == (5, 0, 0, 0), st
