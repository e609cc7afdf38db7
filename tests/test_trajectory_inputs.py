"""CPU preconditions of tests/test_gpu_trajectory.py, with the float64 oracle
alone (tests/trajectory_cases.py): the harness can fail.

First the fixture conditions hold and the clean records of oracle_trajectory
pass every comparator.  Then ten faults a training step could have from its
second step on, each applied to the records of that trajectory as a device
with the fault would have left them (self-consistent where the fault is: a
wrong gradient is also the gradient Adam applied).  Each must be rejected by
the comparator named in MUTATIONS at the first entry it applies to, with the
comparator's measure at least 10 x its bar, and each must pass what the suite
checked before: _check_train_step's Adam bounds on the first step, and a loss
that goes down.

The loss check.  test_model_trains_on_dev_batches asserts losses[-1] < 0.9
losses[0] over eight dropout-free steps on ONE batch; ten steps over batches
of three shapes with every dropout on have no such pair (the free-running
losses are 173.1 on A0 and 164.8 when A0 returns eight steps later, B and the
tail lie elsewhere), so what is reproduced is the run_epoch tests' losses[-1]
< losses[0], on the batch the schedule visits twice.  A record carries the
loss of the forward BEFORE its update, and the faults sit in the update or
behind a later entry's forward: the check sees the same numbers with and
without them, which is the point.

Run with -s for the table of measured ratios.
"""
import numpy as np
import pytest

import trajectory_cases as TC
from decode_cases import _synthetic_model
from graph_cases import lifecycle_feeds
from trajectory_cases import CKPT, EVAL, LOC, TRAIN, WORD

_CACHE = {}


def _trajectory():
    if not _CACHE:
        m = _synthetic_model(False, 64, device="cpu")
        entries = TC.schedule(lifecycle_feeds(m))
        _CACHE["spec"], _CACHE["records"] = TC.spec_of(m), list(TC.oracle_trajectory(entries, m))
    return _CACHE["spec"], [r.copy() for r in _CACHE["records"]]


def _run(spec, records, skip=()):
    h = TC.Harness(spec, skip)
    for r in records:
        h.check(r, getattr(r, "oracle", None))
    return h


def _n_train(records, i):
    """The harness's count at entry i: training entries up to and including it."""
    return sum(r.kind == TRAIN for r in records[:i + 1])


# ------------------------------------------------------------ the clean run
def test_fixture_conditions_hold():
    spec, records = _trajectory()
    assert [r.kind for r in records].count(TRAIN) == 10 and records[6].kind == EVAL and records[9].kind == CKPT
    assert spec.clip == 1.0 and spec.lr == 0.003
    TC.check_fixture(spec, records)
    f = TC.clip_factors(spec, records)
    print("\nclip factors over the ten training steps (min .. max)")
    for i, name in enumerate(TC.NAMES):
        print("%-18s %.3f .. %.3f" % (name, min(f[i]), max(f[i])))


def test_clean_trajectory_passes_every_comparator():
    spec, records = _trajectory()
    h = _run(spec, records)
    assert h.n_train == 10 and len(h.seen_seeds) == 33
    print("\n" + h.table("clean oracle records (fp32 storage)"))
    # what is stored in fp32 is within rounding of the float64 step
    assert h.worst["parameter"][0] <= 1.2e-7 and h.worst["m"][0] <= 1e-7 and h.worst["v"][0] <= 1e-7
    # and the comparators recompute the oracle themselves when not handed it
    g = TC.check_gradients(records[2], spec)
    assert max(g["grads"]) <= 1e-7


# ------------------------------------------------------------ today's checks
def _todays_checks(spec, records):
    """What the suite held a training run to before: the step-1 Adam bounds
    of test_gpu_heads._check_train_step (its formula, on the first record),
    and a loss that goes down (module docstring)."""
    r = records[0]
    lr, clip = spec.lr, spec.clip
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    sqn = TC._sqnorms(r.oracle["sq"])
    for i, (p0, g) in enumerate(zip(r.before["vars"], r.oracle["grads"])):
        n = np.sqrt(sqn[i]) if sqn[i] is not None else np.sqrt(np.sum(g * g))
        gc = g * clip / max(n, clip)
        mm, vv = 0.1 * gc, 0.001 * gc * gc
        ref = p0.astype(np.float64) - lr_t * mm / (np.sqrt(vv) + 1e-8)
        sig = np.abs(gc) > 1e-3 * max(np.abs(gc).max(), 1e-30)
        assert np.abs(r.after["vars"][i] - ref)[sig].max(initial=0.0) <= lr * 1e-2, i
        assert np.abs(r.after["vars"][i] - ref).max() <= 2.01 * lr, i
    same = [x for x in records if x.kind == TRAIN and x.name.rstrip("'") == records[0].name]
    assert len(same) == 2 and same[-1].loss < same[0].loss


# ---------------------------------------------------------------- the faults
def _a_untouched_rows_skipped(spec, rs):
    seen = set()
    for r in rs:
        if r.kind != TRAIN:
            continue
        now = set(TC.lookups(r.feed, WORD).tolist())
        stale = np.asarray(sorted(seen - now), np.int64)
        for s in ("vars", "m", "v"):
            r.after[s][WORD][stale] = r.before[s][WORD][stale]
        seen |= now


def _b_step_count_of_the_capture(spec, rs):
    # shape A is captured at entry 2 (t = 3), shape B at entry 3 (t = 4)
    for i, t in ((5, 3), (7, 4), (8, 3)):
        TC.rebuild_after(spec, rs[i], t)


def _c_eval_advances_the_step_count(spec, rs):
    rs[6].t_after += 1
    for i in range(7, len(rs)):
        rs[i].t_before += 1
        rs[i].t_after += 1
        if rs[i].kind == TRAIN:
            TC.rebuild_after(spec, rs[i], _n_train(rs, i) + 1)


def _d_seed_repeated(spec, rs):
    r = rs[1]
    r.drop["path"]["seed"] = rs[0].drop["path"]["seed"]
    o = TC.oracle_step(spec, [x.astype(np.float64) for x in r.before["vars"]], r.feed, r.drop)
    r.loss, r.grads, r.sq = float(np.float32(o["loss"])), TC._f32(o["grads"]), TC._f32(o["sq"])
    r.oracle = None                     # (check_gradients recomputes it from the record)
    TC.rebuild_after(spec, r, 2)


def _e_gradient_accumulated(spec, rs):
    rs[2].grads[0] = rs[2].grads[0] + rs[0].grads[0]      # edge_weights: A1's plus A0's
    TC.rebuild_after(spec, rs[2], 3)


def _f_word_clipped_by_last_norm(spec, rs):
    sq = [rs[1].sq[0], rs[1].sq[1], rs[0].sq[2]]
    TC.rebuild_after(spec, rs[1], 2, sq=sq)


def _g_loc_clipped_by_one_segment(spec, rs):
    r = rs[0]
    TC.rebuild_after(spec, r, 1, sq=[np.float32(r.oracle["sq_raw"][0]), r.sq[1], r.sq[2]])


def _h_loc_gradient_of_one_segment(spec, rs):
    r = rs[1]
    r.grads[LOC] = r.oracle["dts"][0].astype(np.float32)
    TC.rebuild_after(spec, r, 2)


def _i_checkpoint_zeroes_the_slots(spec, rs):
    zero = lambda st: dict(vars=st["vars"], m=[np.zeros_like(x) for x in st["m"]], v=[np.zeros_like(x) for x in st["v"]])
    rs[9].after = zero(rs[9].after)
    rs[10].before = zero(rs[10].before)
    TC.rebuild_after(spec, rs[10], 9)


def _j_eval_writes_the_gradient_buffer(spec, rs):
    rs[6].flat_after = rs[6].flat_after.copy()
    rs[6].flat_after[:64] = 0.0


# name -> (fault, [(comparators skipped, rejecting comparator, entry)]): the first
# row is the first rejection, a further row the next one with that comparator off
MUTATIONS = {
    "a": (_a_untouched_rows_skipped, [((), "check_update", 1), (("check_update",), "check_untouched_rows", 1)]),
    "b": (_b_step_count_of_the_capture, [((), "check_update", 5)]),
    "c": (_c_eval_advances_the_step_count, [((), "check_step_count", 6),
                                            (("check_step_count", "check_eval_is_pure"), "check_update", 7)]),
    "d": (_d_seed_repeated, [((), "check_seeds", 1)]),
    "e": (_e_gradient_accumulated, [((), "check_gradients", 2)]),
    "f": (_f_word_clipped_by_last_norm, [((), "check_update", 1)]),
    "g": (_g_loc_clipped_by_one_segment, [((), "check_update", 0)]),
    "h": (_h_loc_gradient_of_one_segment, [((), "check_gradients", 1)]),
    "i": (_i_checkpoint_zeroes_the_slots, [((), "check_update", 10)]),
    "j": (_j_eval_writes_the_gradient_buffer, [((), "check_eval_is_pure", 6)]),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_rejected_and_was_invisible(name):
    spec, records = _trajectory()
    fault, expect = MUTATIONS[name]
    fault(spec, records)
    _todays_checks(spec, records)            # what the suite could see: nothing
    for skip, comparator, step in expect:
        with pytest.raises(TC.Rejected) as e:
            _run(spec, records, skip)
        r = e.value
        ratio = r.measure / r.bar if r.bar else float("inf")
        print("\n%s: %-22s entry %2d (%s)  %-18s measure %.3e  bar %.1e  ratio %.3g"
              % (name, r.comparator, r.step, records[r.step].name, r.tensor if isinstance(r.tensor, str)
                 else TC.NAMES[r.tensor], r.measure, r.bar, ratio))
        assert (r.comparator, r.step) == (comparator, step), str(r)
        assert r.measure >= 10 * r.bar and r.measure > 0, str(r)
    if name == "d":
        # the repeated seed's step is self-consistent: only check_seeds sees it
        _run(spec, records, ("check_seeds",))
