"""Every step of a short training run against the float64 oracle
(test_gpu_trajectory.py on the GPU, test_trajectory_inputs.py on the host):
the schedule, the oracle of one whole training step, the record of one
schedule entry and the comparators over a record.  Imports no GPU.

The model and the batches are the lifecycle cases' (decode_cases.
_synthetic_model, graph_cases.lifecycle_feeds): full batches of 5 x 24 nodes
(shape A) and 5 x 40 (shape B), a tail batch, all four dropouts on.

The comparison is teacher-forced.  Each step's gradients are held to the
oracle evaluated at the variables the device had BEFORE the step, and Adam is
held to O.adam_step applied to the device's own before-state with the device's
own fp32 gradients and lookup norms: after Adam's sign-like first step a free
fp32 run and a float64 run legitimately separate, and gradient rounding would
be amplified through 1 / sqrt(v).  What is left is the glue: which gradient
reaches which tensor, which norm clips it, the step count, the slots, the
seeds.  ``oracle_trajectory`` (a free-running float64 trainer that stores fp32,
as a device would) only feeds the host half and the choice of the clip norm.

The clip norm stays the default clamp_gradient_norm = 1.0.  Over the ten
training steps of the free-running trajectory (hidden 64) the norms that
clip_by_norm reads are: edge_weights 3.4 .. 7.5, edge_biases 2.8 .. 4.7, the
GRU kernels 1.2 .. 3.0 and 4.3 .. 9.9, gates_bias 0.32 .. 0.76 (never
clipped), the word table's lookup norm 2.9 .. 7.0, loc 3.4 .. 8.0, pos 1.6 ..
3.6, the head weights 5.7 .. 12.4 and 5.2 .. 12.0: every tensor but gates_bias
is clipped in every step, and the clip factor 1 / norm of each changes by far
more than 10 % between the shapes (A against B against the one-graph tail),
which is what makes a norm taken from the wrong step or the wrong segments
visible.  A clip norm inside one tensor's range (clipped here, not there)
was not needed for any mutation of test_trajectory_inputs.py.
``check_fixture`` asserts the conditions on the oracle's values, so a change
of the fixture cannot lose them silently.

The repeated word.  The treebank's batches repeat few words, and the word
table's IndexedSlices norm (one row per lookup) then differs from the dense
norm of the same gradient by under 1 % in some steps.  ``with_repeats`` gives
nodes 1 .. 10 of every graph of a batch one word: the two norms then differ by
2.2 % .. 18 % in every step (their sign is not fixed: the rows of one word add
up coherently or not), and every step still leaves 20 and more word rows
looked up earlier and not now.
"""
import collections

import numpy as np

import ggnn_oracle as O

from graph_cases import KEEPS

TOL = 1e-3                     # test_gpu_heads.TOL: loss (relative) and gradients (_nmax)
SQ_TOL = 1e-4                  # _check_train_step's bar on the lookup norms
P_TOL, SLOT_TOL = 1e-6, 1e-5   # test_gpu_optim: parameters (absolute), m and v (of the largest entry)
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))   # the betas as the C ABI carries them
REPEAT = 10                    # with_repeats: nodes 1 .. 10 of every graph of a batch share one word
LOC, POS, WORD = 6, 7, 8       # the tables in trainable_variables() order
PATH, HEADS = range(0, 6), range(9, 13)
TABLE_COLS = {LOC: (0, 3), POS: (1,), WORD: (2,)}
NAMES = ("edge_weights", "edge_biases", "gates_kernel", "gates_bias", "candidate_kernel", "candidate_bias",
         "loc_embeddings", "pos_embeddings", "word_embeddings", "head_W", "head_b", "edge_W", "edge_b")
TRAIN, EVAL, CKPT = "train", "eval", "ckpt"
EVAL_KEEPS = {k: 1.0 for k in KEEPS}       # a validation feed: every dropout off

Entry = collections.namedtuple("Entry", "kind name feed")
Spec = collections.namedtuple("Spec", "hidden T num_edge_types o oe lr clip")


class Rejected(AssertionError):
    """A comparator's verdict: which one, at which schedule entry, on which
    tensor, the measured value and the bar it missed."""

    def __init__(self, comparator, step, tensor, measure, bar, what=""):
        self.comparator, self.step, self.tensor, self.measure, self.bar = comparator, step, tensor, measure, bar
        name = NAMES[tensor] if isinstance(tensor, int) else tensor
        super().__init__("%s: step %d, %s: %s %.3e > %.1e" % (comparator, step, name, what, measure, bar))


def _nmax(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def spec_of(m) -> Spec:
    return Spec(m.params["hidden_size"], m.params["num_timesteps"], m.num_edge_types, m.params["output_size"],
                m.output_size_edges, m.params["learning_rate"], m.params["clamp_gradient_norm"])


def with_repeats(feed, k=REPEAT):
    """A copy of ``feed`` in which nodes 1 .. k of every graph carry the word
    of the first graph's node 1: that id's row of the word table's gradient is
    the sum of up to b * k lookups' rows, so the table's IndexedSlices norm and
    its dense norm differ (check_fixture: by more than 1 % in every step)."""
    wi = np.array(feed["word_inputs"], copy=True)
    wi[:, 1:k + 1, 2] = wi[0, 1, 2]
    return dict(feed, word_inputs=wi)


def schedule(F):
    """A0 B0 A1 B1 tail A2 EVAL(A3) B2 A0 CKPT tail A3.  Each full shape runs
    at least three times and never twice in a row: first batch uncaptured,
    second captured, later ones replays with another shape's steps between
    them; the evaluation and the checkpoint sit between replays."""
    A, B, tail = [with_repeats(f) for f in F.A], [with_repeats(f) for f in F.B], with_repeats(F.tail)
    s = [Entry(TRAIN, "A0", A[0]), Entry(TRAIN, "B0", B[0]), Entry(TRAIN, "A1", A[1]), Entry(TRAIN, "B1", B[1]),
         Entry(TRAIN, "tail", tail), Entry(TRAIN, "A2", A[2]), Entry(EVAL, "EVAL(A3)", dict(A[3], **EVAL_KEEPS)),
         Entry(TRAIN, "B2", B[2 % len(B)]), Entry(TRAIN, "A0'", A[0]), Entry(CKPT, "CKPT", None),
         Entry(TRAIN, "tail'", tail), Entry(TRAIN, "A3", A[3])]
    shape = lambda e: (e.feed["num_graphs"], e.feed["num_vertices"])
    train = [e for e in s if e.kind == TRAIN]
    for full in (shape(s[0]), shape(s[1])):
        assert sum(shape(e) == full for e in train) >= 3
    assert all(shape(x) != shape(y) for x, y in zip(train, train[1:]))
    assert 10 <= len(s) <= 12
    return s


# ------------------------------------------------------------------ the oracle
def _dense_adjacency(feed, num_edge_types):
    if feed.get("adjacency_matrix") is None:
        from ggnn_amd.batching import graph_to_adj_mat_bd
        return np.stack([graph_to_adj_mat_bd(g, feed["num_vertices"], num_edge_types)
                         for g in feed["adjacency_edges"]])
    return np.asarray(feed["adjacency_matrix"], np.float64)


def _oracle_forward(spec, P, feed, drop):
    """The forward half of the step: P: the 13 float64 variables in
    trainable_variables() order; drop: dict(embed, path, heads) as the model
    records them (last_embed, last_dropout, last_heads)."""
    wi = np.asarray(feed["word_inputs"]).astype(np.int64)
    segs = [(P[LOC], 0), (P[POS], 1), (P[WORD], 2), (P[LOC], 3)]
    e, dr, hd = drop["embed"], drop["path"], drop["heads"]
    h0 = O.embed_forward(segs, wi, spec.hidden, e["keep"], e["seed"])
    w64 = dict(zip(NAMES[:6], P[:6]))
    A = _dense_adjacency(feed, spec.num_edge_types)
    hT, caches = O.forward(A, h0, w64, spec.T,
                           dropout=dict(edge_keep=dr["edge_keep"], state_keep=dr["state_keep"], seed=dr["seed"]))
    b, v = feed["num_graphs"], feed["num_vertices"]
    heads = [dict(W=P[9], b=P[10], labels=np.asarray(feed["target_values_head"], np.float64).reshape(b, v, spec.o)),
             dict(W=P[11], b=P[12], labels=np.asarray(feed["target_values_edges"], np.float64).reshape(b, v, spec.oe))]
    probs, losses = O.heads_forward(hT, h0, heads, hd["keep"], hd["seed"], hd["target_num"])
    return dict(wi=wi, segs=segs, h0=h0, w64=w64, A=A, hT=hT, caches=caches, heads=heads, probs=probs, losses=losses)


def oracle_step(spec, P, feed, drop):
    """One whole btb training step in float64, composed as the model composes
    it (and as test_gpu_heads._check_train_step always has): the loss, the 13
    gradients in trainable_variables() order, the three IndexedSlices norms
    (loc: both its segments), plus the pieces some checks read (gp: the
    path's own gradients, dts / sq_raw: per front-end segment)."""
    f = _oracle_forward(spec, P, feed, drop)
    e, hd = drop["embed"], drop["heads"]
    dWs, dbs, dhT, dh0_heads = O.heads_backward(f["hT"], f["h0"], f["heads"], f["probs"], hd["keep"], hd["seed"],
                                                hd["target_num"])
    gp = O.backward(f["A"], dhT, f["caches"], f["w64"])
    dts, sq = O.embed_backward(f["segs"], f["wi"], spec.hidden, dh0_heads + gp["h0"], e["keep"], e["seed"])
    grads = [gp[k] for k in NAMES[:6]] + [dts[0] + dts[3], dts[1], dts[2], dWs[0], dbs[0], dWs[1], dbs[1]]
    return dict(loss=float(sum(f["losses"])), grads=grads, sq=[sq[0] + sq[3], sq[1], sq[2]], gp=gp, dts=dts,
                sq_raw=sq, probs=f["probs"])


def oracle_probs(spec, P, feed, drop):
    return _oracle_forward(spec, P, feed, drop)["probs"]


def _sqnorms(sq):
    return [None] * 6 + [float(x) for x in sq] + [None] * 4


def adam_reference(spec, start, grads, sq, t):
    """O.adam_step in float64 from ``start`` (vars, m, v) with the given
    gradients and lookup norms at step t.  Returns (vars, m, v)."""
    p, m, v = ([np.asarray(x, np.float64).copy() for x in start[k]] for k in ("vars", "m", "v"))
    O.adam_step(p, [np.asarray(g, np.float64) for g in grads], m, v, t, lr=spec.lr, beta1=B1, beta2=B2,
                clip_norm=spec.clip, sqnorms=_sqnorms(sq))
    return dict(vars=p, m=m, v=v)


# ------------------------------------------------------------------ the record
class StepRecord:
    """One schedule entry as read back from the device (numpy / host values).

    index, kind, name, feed; before / after: dict(vars, m, v) of 13 fp32
    arrays each; t_before / t_after: optimizer.t; graph_stats.
    Training: loss, grads (13 fp32), sq (the three lookup norms, fp32), drop
    (embed / path / heads draws: keeps, seeds, target_num).
    Evaluation: drop, probs (both heads'), scores, flat_before / flat_after
    (the flat gradient buffer)."""

    def __init__(self, index, kind, name, feed, **fields):
        self.index, self.kind, self.name, self.feed = index, kind, name, feed
        self.loss = self.grads = self.sq = self.drop = self.probs = self.scores = None
        self.flat_before = self.flat_after = None
        self.graph_stats = {}
        self.__dict__.update(fields)

    @property
    def seeds(self):
        return (self.drop["embed"]["seed"], self.drop["path"]["seed"], self.drop["heads"]["seed"])

    def copy(self):
        r = StepRecord(self.index, self.kind, self.name, self.feed)
        r.__dict__.update(self.__dict__)
        for k in ("before", "after"):
            setattr(r, k, {s: [a.copy() for a in x] for s, x in getattr(self, k).items()})
        r.grads = None if self.grads is None else [g.copy() for g in self.grads]
        r.drop = None if self.drop is None else {k: dict(d) for k, d in self.drop.items()}
        return r


def _f32(xs):
    return [np.asarray(x).astype(np.float32) for x in xs]


def lookups(feed, table):
    """The ids of ``table`` a batch looks up (padded nodes included, as the
    front-end gathers them)."""
    wi = np.asarray(feed["word_inputs"]).astype(np.int64)
    return np.unique(np.concatenate([wi[..., c].reshape(-1) for c in TABLE_COLS[table]]))


def rebuild_after(spec, rec, t, grads=None, sq=None, start=None):
    """rec.after recomputed as a device would store it: Adam from ``start``
    (default: rec.before) with the given gradients / norms (default: the
    record's), rounded to fp32."""
    ref = adam_reference(spec, start or rec.before, grads or rec.grads, rec.sq if sq is None else sq, t)
    rec.after = {k: _f32(x) for k, x in ref.items()}


def draw_seeds(m, feed, target_num=None):
    """The three draws of a step in the model's order (front-end, path,
    heads) with the keeps the step reads from the feed."""
    se, sp, sh = m._seed(), m._seed(), m._seed()
    if target_num is None:
        target_num = float(np.asarray(feed["target_mask"], np.float64)[0].sum() + O.SMALL_NUMBER)
    return dict(embed=dict(keep=float(feed["emb_dropout_keep_prob"]), seed=se),
                path=dict(edge_keep=float(feed["edge_weight_dropout_keep_prob"]),
                          state_keep=float(feed["graph_state_keep_prob"]), seed=sp),
                heads=dict(keep=float(feed["out_layer_dropout_keep_prob"]), seed=sh, target_num=target_num))


def host_scores(spec, feed, probs):
    """evaluation's host scoring of both heads' probabilities (as
    model._score_arrays feeds it)."""
    from ggnn_amd.evaluation import batch_las_uas
    b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
    r = lambda key, w: np.asarray(feed[key], np.float32).reshape(b, v * w)
    return batch_las_uas(r("target_values_head", spec.o), np.asarray(probs[0], np.float32).reshape(b, v * spec.o), v,
                         r("node_mask", spec.o), r("target_values_edges", spec.oe),
                         np.asarray(probs[1], np.float32).reshape(b, v * spec.oe), r("node_mask_edges", spec.oe),
                         spec.o, spec.oe)


def oracle_trajectory(entries, m):
    """The schedule through a free-running float64 trainer (oracle_step +
    O.adam_step) that stores its state in fp32 as a device would, with the
    seeds drawn by the (CPU) model ``m`` in the model's order.  Yields
    StepRecords whose device fields are the oracle's values rounded to fp32;
    rec.oracle keeps the float64 step (evaluated at rec.before)."""
    spec = spec_of(m)
    state = dict(vars=_f32(p.detach().cpu().numpy() for p in m.trainable_variables()))
    state["m"] = [np.zeros_like(x) for x in state["vars"]]
    state["v"] = [np.zeros_like(x) for x in state["vars"]]
    t, flat = 0, np.zeros(4, np.float32)
    for i, e in enumerate(entries):
        rec = StepRecord(i, e.kind, e.name, e.feed, before=state, after=state, t_before=t, t_after=t)
        if e.kind == TRAIN:
            rec.drop = draw_seeds(m, e.feed)
            rec.oracle = o = oracle_step(spec, [x.astype(np.float64) for x in state["vars"]], e.feed, rec.drop)
            rec.loss, rec.grads, rec.sq = float(np.float32(o["loss"])), _f32(o["grads"]), _f32(o["sq"])
            t += 1
            rebuild_after(spec, rec, t)
            rec.t_after, state = t, rec.after
            flat = np.concatenate([g.reshape(-1) for g in rec.grads] + [np.asarray(rec.sq, np.float32)])
        elif e.kind == EVAL:
            rec.drop = draw_seeds(m, e.feed)
            rec.probs = _f32(oracle_probs(spec, [x.astype(np.float64) for x in state["vars"]], e.feed, rec.drop))
            rec.scores = host_scores(spec, e.feed, rec.probs)
            rec.flat_before = rec.flat_after = flat
        yield rec


# ------------------------------------------------------------------ comparators
def _raise_worst(comparator, step, misses):
    """misses: (tensor, measure, bar, what) of every quantity; raises for the
    one furthest above its bar, if any is."""
    bad = [x for x in misses if not x[1] <= x[2]]
    if bad:
        t, measure, bar, what = max(bad, key=lambda x: x[1] / x[2] if x[1] == x[1] else np.inf)
        raise Rejected(comparator, step, t, measure, bar, what)


def check_gradients(rec, spec, ref=None):
    """The loss, every gradient and the lookup norms against oracle_step at
    the record's before-variables (``ref``: that step, if already computed).
    Returns the measures."""
    if ref is None:
        ref = oracle_step(spec, [x.astype(np.float64) for x in rec.before["vars"]], rec.feed, rec.drop)
    out = {"loss": abs(rec.loss - ref["loss"]) / abs(ref["loss"]),
           "grads": [_nmax(g, r) for g, r in zip(rec.grads, ref["grads"])],
           "sq": [abs(float(got) - r) / r for got, r in zip(rec.sq, ref["sq"])]}
    _raise_worst("check_gradients", rec.index,
                 [("loss", out["loss"], TOL, "relative error")]
                 + [(i, x, TOL, "gradient _nmax") for i, x in enumerate(out["grads"])]
                 + [(LOC + k, x, SQ_TOL, "lookup norm, relative") for k, x in enumerate(out["sq"])])
    return out


def check_update(rec, spec, start, n_train):
    """The teacher-forced Adam: O.adam_step from ``start`` (the record's
    before-state; behind a checkpoint round trip, the state saved) with the step's own fp32 gradients
    and lookup norms and t = n_train, the harness's count.  Returns the
    measures and the reference."""
    for i, p in enumerate(start["vars"]):
        # the condition of the absolute bar: max|p| <= 1 at initialisation
        # (check_fixture); gates_bias starts at exactly 1 and Adam moves it by
        # about lr a step (1.025 after ten), where fp32 spacing is 1.2e-7
        if not np.abs(p).max() <= 1.0 + 4 * spec.lr * n_train:
            raise Rejected("check_update", rec.index, i, float(np.abs(p).max()), 1.0, "max|p| before the step")
    ref = adam_reference(spec, start, rec.grads, rec.sq, n_train)
    n = len(ref["vars"])
    out = {"vars": [float(np.abs(rec.after["vars"][i] - ref["vars"][i]).max()) for i in range(n)],
           "m": [_nmax(rec.after["m"][i], ref["m"][i]) for i in range(n)],
           "v": [_nmax(rec.after["v"][i], ref["v"][i]) for i in range(n)]}
    _raise_worst("check_update", rec.index,
                 [(i, x, P_TOL, "variable, absolute error") for i, x in enumerate(out["vars"])]
                 + [(i, x, SLOT_TOL, "slot m, of its largest entry") for i, x in enumerate(out["m"])]
                 + [(i, x, SLOT_TOL, "slot v, of its largest entry") for i, x in enumerate(out["v"])])
    return out, ref


def check_untouched_rows(rec, spec, start, n_train, seen, ref=None):
    """Rows of a table that this step does not look up.  Seen in an earlier
    step (``seen``: table -> ids): gradient exactly 0, yet Adam moves them (the
    slots decay): at least one by more than 100 x the parameter bar in the
    reference, and every such row moved on the device.  Never seen: p, m and v
    bit-unchanged.  Returns table -> (stale rows, largest reference update)."""
    if ref is None:
        ref = adam_reference(spec, start, rec.grads, rec.sq, n_train)
    out = {}
    for tb in (LOC, POS, WORD):
        rows = rec.before["vars"][tb].shape[0]
        now = lookups(rec.feed, tb)
        stale = np.setdiff1d(np.asarray(sorted(seen[tb]), np.int64), now)
        never = np.setdiff1d(np.arange(rows), np.union1d(now, np.asarray(sorted(seen[tb]), np.int64)))
        g = rec.grads[tb]
        nz = int(np.count_nonzero(g[stale])) + int(np.count_nonzero(g[never]))
        if nz:
            raise Rejected("check_untouched_rows", rec.index, tb, nz, 0, "non-zero gradient entries in rows not looked up")
        for s in ("vars", "m", "v"):
            d = int(np.count_nonzero(rec.after[s][tb][never] != rec.before[s][tb][never]))
            if d:
                raise Rejected("check_untouched_rows", rec.index, tb, d, 0, "%s entries changed in rows never looked up" % s)
        if not stale.size:
            continue
        move = np.abs(ref["vars"][tb][stale] - np.asarray(start["vars"][tb], np.float64)[stale]).max(axis=1)
        out[tb] = (int(stale.size), float(move.max()))
        if not move.max() > 100 * P_TOL:
            raise Rejected("check_untouched_rows", rec.index, tb, 100 * P_TOL, float(move.max()),
                           "the fixture: no stale row's reference update is above")
        big = stale[move > 100 * P_TOL]
        still = np.all(rec.after["vars"][tb][big] == rec.before["vars"][tb][big], axis=1)
        if still.any():
            raise Rejected("check_untouched_rows", rec.index, tb, float(move[move > 100 * P_TOL][still].max()), P_TOL,
                           "%d stale rows did not move; reference update" % int(still.sum()))
    return out


def check_seeds(rec, earlier):
    """The three seeds of a step differ from each other and from every seed of
    every earlier entry (``earlier``: a set)."""
    s = rec.seeds
    rep = len(s) - len(set(s)) + len(set(s) & earlier)
    if rep:
        raise Rejected("check_seeds", rec.index, "seeds", rep, 0, "repeated seeds")


def check_step_count(rec, n_train):
    if rec.t_after != n_train:
        raise Rejected("check_step_count", rec.index, "optimizer.t", abs(rec.t_after - n_train), 0,
                       "optimizer.t = %d, %d training steps so far: off by" % (rec.t_after, n_train))


def check_eval_is_pure(rec, spec):
    """evaluate_batch between two training steps: variables, slots, t and the
    flat gradient buffer bit-equal; the scores are evaluation's host scoring
    of the probabilities; the probabilities match the oracle forward with
    every keep at 1, as a validation feed has them.  Returns the two _nmax."""
    for s in ("vars", "m", "v"):
        for i, (a, b) in enumerate(zip(rec.before[s], rec.after[s])):
            d = int(np.count_nonzero(a != b))
            if d:
                raise Rejected("check_eval_is_pure", rec.index, i, d, 0, "%s entries changed" % s)
    if rec.t_after != rec.t_before:
        raise Rejected("check_eval_is_pure", rec.index, "optimizer.t", abs(rec.t_after - rec.t_before), 0,
                       "step count moved by")
    d = int(np.count_nonzero(rec.flat_before != rec.flat_after)) + abs(rec.flat_before.size - rec.flat_after.size)
    if d:
        raise Rejected("check_eval_is_pure", rec.index, "gradient buffer", d, 0, "entries changed")
    dr = rec.drop
    keeps = (dr["embed"]["keep"], dr["path"]["edge_keep"], dr["path"]["state_keep"], dr["heads"]["keep"])
    assert keeps == (1.0, 1.0, 1.0, 1.0), keeps
    want = host_scores(spec, rec.feed, rec.probs)
    if tuple(rec.scores) != tuple(want):
        raise Rejected("check_eval_is_pure", rec.index, "scores", max(abs(a - b) for a, b in zip(rec.scores, want)), 0,
                       "scores against the host scoring")
    ref = oracle_probs(spec, [x.astype(np.float64) for x in rec.before["vars"]], rec.feed, dr)
    out = []
    for k, (p, r) in enumerate(zip(rec.probs, ref)):
        out.append(_nmax(np.asarray(p).reshape(r.shape), r))
        if not out[-1] <= TOL:
            raise Rejected("check_eval_is_pure", rec.index, "probabilities %d" % k, out[-1], TOL, "_nmax")
    return out


class Harness:
    """Runs every comparator over the records of a schedule, in order, and
    keeps what they need from entry to entry: its own count of the training
    steps, the seeds and lookups seen so far, and across a checkpoint round
    trip the state that went into it: the step behind it is referred to that
    state, so a restore that loses something shows in that step's update.  ``skip``: comparators left out (to show a second one
    reject).  ``worst``: the largest measure per quantity and its step."""

    def __init__(self, spec, skip=()):
        self.spec, self.skip = spec, set(skip)
        self.n_train, self.seen_seeds, self.carry = 0, set(), None
        self.seen = {tb: set() for tb in TABLE_COLS}
        self.worst = {}

    def _note(self, key, value, step):
        if value > self.worst.get(key, (-1.0, None))[0]:
            self.worst[key] = (value, step)

    def check(self, rec, ref=None):
        spec, on = self.spec, lambda name: name not in self.skip
        # the state the update is referred to: the record's own before-state,
        # and behind a checkpoint round trip the state that went into it
        start = self.carry if self.carry is not None else rec.before
        self.carry = rec.before if rec.kind == CKPT else None
        if rec.kind == TRAIN:
            self.n_train += 1
        if on("check_step_count"):
            check_step_count(rec, self.n_train)
        if rec.kind == CKPT:
            return
        if on("check_seeds"):
            check_seeds(rec, self.seen_seeds)
        self.seen_seeds |= set(rec.seeds)
        if rec.kind == EVAL:
            if on("check_eval_is_pure"):
                for k, x in enumerate(check_eval_is_pure(rec, spec)):
                    self._note("eval probabilities %d" % k, x, rec.index)
            return
        if on("check_gradients"):
            g = check_gradients(rec, spec, ref)
            self._note("loss", g["loss"], rec.index)
            for i, x in enumerate(g["grads"]):
                self._note("grad " + NAMES[i], x, rec.index)
            for k, x in enumerate(g["sq"]):
                self._note("lookup norm " + NAMES[LOC + k], x, rec.index)
        aref = None
        if on("check_update"):
            u, aref = check_update(rec, spec, start, self.n_train)
            for s, label in (("vars", "parameter"), ("m", "m"), ("v", "v")):
                i = int(np.argmax(u[s]))
                self._note(label, u[s][i], (rec.index, NAMES[i]))
        if on("check_untouched_rows"):
            check_untouched_rows(rec, spec, start, self.n_train, self.seen, aref)
        for tb in TABLE_COLS:
            self.seen[tb] |= set(lookups(rec.feed, tb).tolist())

    def table(self, title):
        rows = ["%-32s %10s  %s" % (title, "worst", "at step")]
        for k in sorted(self.worst):
            rows.append("%-32s %10.2e  %s" % (k, self.worst[k][0], self.worst[k][1]))
        return "\n".join(rows)


# ------------------------------------------------------------ fixture conditions
def clip_factors(spec, records):
    """tensor -> the clip factor clip / max(norm, clip) of every training
    step, from the oracle's float64 gradients and lookup norms."""
    out = {i: [] for i in range(13)}
    for r in records:
        if r.kind != TRAIN:
            continue
        sq = _sqnorms(r.oracle["sq"])
        for i, g in enumerate(r.oracle["grads"]):
            n = np.sqrt(sq[i] if sq[i] is not None else np.sum(g * g))
            out[i].append(spec.clip / max(n, spec.clip))
    return out


def check_fixture(spec, records):
    """The conditions the comparators' sharpness rests on, from the feeds and
    the oracle's values (records of oracle_trajectory)."""
    train = [r for r in records if r.kind == TRAIN]
    seen = set()
    for k, r in enumerate(train):
        now = set(lookups(r.feed, WORD).tolist())
        if k:
            assert len(seen - now) >= 20, (r.name, len(seen - now))
        seen |= now
        ids = np.asarray(r.feed["word_inputs"])[..., 2].reshape(-1)
        assert np.unique(ids).size < ids.size, r.name
        g, sq = r.oracle["grads"][WORD], r.oracle["sq"][2]
        dense = np.sqrt(np.sum(g * g))
        assert abs(np.sqrt(sq) - dense) > 0.01 * dense, (r.name, np.sqrt(sq), dense)
    f = clip_factors(spec, records)
    varies = lambda i: min(f[i]) < 1.0 and (max(f[i]) == 1.0 or max(f[i]) > 1.1 * min(f[i]))
    assert any(varies(i) for i in PATH), {NAMES[i]: f[i] for i in PATH}
    assert any(varies(i) for i in HEADS), {NAMES[i]: f[i] for i in HEADS}
    assert varies(WORD), f[WORD]
    for p in records[0].before["vars"]:
        assert np.abs(p).max() <= 1.0
