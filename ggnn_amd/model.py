"""Drop-in ``DenseGGNNChemModel`` for the propagation hot path.

Mirrors the part of the reference class (chem_tensorflow_dense.py:147-437 and
chem_tensorflow.py:70-136) that the hot path reads, with the same names:

* ``params['hidden_size', 'num_timesteps', 'use_edge_bias', ...]``
  (``default_params``, chem_tensorflow.py:77-112, chem_tensorflow_dense.py:152-161)
* ``num_edge_types`` (C = 2 * num_edge_types adjacency channels, :192-206)
* ``weights['edge_weights', 'edge_biases', 'edge_weights_fixed',
  'edge_biases_fixed', 'node_gru']`` (``prepare_specific_graph_model``, :163-241)
* ``placeholders`` -- here a feed dict keyed by name; ``feed()`` stages a
  minibatch produced by ``make_minibatch_iterator`` (the reference's
  ``sess.run(feed_dict=...)``, chem_tensorflow.py:595)
* ``compute_final_node_representations(initial_node_representations,
  fixed_ts=None)`` -> [b, v, h] (:312-340), differentiable: its backward is the
  engine's HIP backward (the reference's TF autodiff, chem_tensorflow.py:496)
* ``process_raw_graphs`` / ``make_minibatch_iterator`` (``BtbBatching``)
* ``save_progress`` / ``restore_progress`` in the reference's pickle format
  (chem_tensorflow.py:796-855; ``checkpoint.py``) and the host LAS/UAS scoring
  ``get_las_uas`` / ``evaluate_batch`` (chem_tensorflow_dense.py:1160-1215,
  1304-1319; ``evaluation.py``)
* the callers either side of the path:
  ``get_initial_node_representation`` (embedding front-end, :264-306),
  ``gated_regression`` + the btb loss (:439-516, chem_tensorflow.py:326-421)
  via ``build_loss()``, and ``train_step()`` (loss -> backward -> clip + Adam,
  chem_tensorflow.py:483-506) -- all on the HIP library (``heads.py``).

* not in the reference: ``predict_batch`` / ``parse`` (the predicted tree of a
  batch / of raw sentences), ``score_epoch`` and ``evaluate_batch(on_device=
  True)`` (the scores from per-graph counts): ``decoding.DecodingMixin``, the
  decode and the tree passes after it on the device (``tree=``, ``confidence=``)
* not in the reference: ``params['structured_loss']`` ("nonprojective" /
  "projective"): the head's loss as the negative log-likelihood of the gold
  tree (``ggnn_tree_loss`` after the heads' forward, in every step body;
  ``ops['tree_loss_used']``: the graphs of the last step it applied to);
  "nonprojective-margin" / "projective-margin": the structured hinge loss over
  cost-augmented decoding in its place (``ggnn_margin_loss``), with
  ``params['structured_loss_margin']`` (default 1.0) the cost of a wrong head
  (``ops['margin_loss_hamming']``: the wrong heads of the last step's
  cost-augmented trees, per graph)

The arithmetic runs in libggnn.so; torch tensors only hold device memory and
carry the autograd graph around the call.

How the class is laid out: one step body without autograd (``_forward`` on a
``_StepFeed``; ``_forward_backward`` adds the backward half), which
``train_step`` runs eagerly and ``_graph_step`` records as a captured step;
one dropout-free forward behind every evaluation entry but the host branch of
``evaluate_batch`` (``_eval_forward``: captured if possible, else
``build_loss``); one epoch loop (``_epoch``) under ``run_epoch`` and
``score_epoch``, whose per-batch results come back through
``upload.PinnedFetch``.  All state is declared in
``prepare_specific_graph_model``; the objects that load libggnn.so are made on
first use by ``_embedder`` / ``_output_heads`` / ``_decode_heads`` / ``_engine``.
"""
from __future__ import annotations

import random
import time
from collections import OrderedDict

import numpy as np
import torch

from . import checkpoint as _ckpt
from . import dist as _dist
from . import evaluation as _eval
from .batching import BtbBatching, ThreadedIterator
from .decoding import DecodingMixin, _as_np, _tree_mode
from .dist import FlatTrainBuffer
from .engine import PropagationEngine
from .graphs import CapturedStep, PinnedRing, StepLayout, edge_arrays
from .heads import SMALL_NUMBER, EmbedFunction, EmbeddingFrontEnd, HeadsFunction, OutputHeads, word_inputs_tensor
from .optim import ClipAdam
from .upload import PinnedFetch, Uploader

GRU_KEYS = ("gates_kernel", "gates_bias", "candidate_kernel", "candidate_bias")
# the path's weights in the order the engine's dicts and _Propagate take them
PATH_KEYS = ("edge_weights", "edge_biases") + GRU_KEYS


def mlp_init(shape, rng):
    """utils.py MLP.init_weights: sqrt(6/(in+out)) * (2*rand - 1)."""
    return (np.sqrt(6.0 / (shape[-2] + shape[-1])) * (2 * rng.rand(*shape).astype(np.float32) - 1)).astype(np.float32)


def glorot_init(shape, rng=None):
    """U(+-sqrt(6/(fan_in+fan_out))) on the last two dims (utils.py:11-14)."""
    rng = np.random if rng is None else rng
    lim = np.sqrt(6.0 / (shape[-2] + shape[-1]))
    return rng.uniform(low=-lim, high=lim, size=shape).astype(np.float32)


class _StepFeed:
    """One step's inputs as the library calls take them: device tensors
    (word_inputs, labels), the seeds as values or as device addresses
    (seed_device, GGNN_SEED_DEVICE), target_num as a number or a device
    scalar, the engine and heads that run the step and how the engine stages
    the batch's adjacency."""

    def __init__(self, wi, seeds, seed_values, seed_device, labels, target_num, engine, heads, stage, b, v,
                 target_num_value=None, n_nodes=None):
        self.wi, self.seeds, self.seed_values, self.seed_device = wi, seeds, seed_values, seed_device
        self.labels, self.target_num, self.engine, self.heads, self.stage = labels, target_num, engine, heads, stage
        self.b, self.v = b, v
        self.target_num_value = target_num if target_num_value is None else target_num_value
        self.n_nodes = n_nodes    # int32 [b] on the device (params['structured_loss']), else None


class _Propagate(torch.autograd.Function):
    """h_T = GGNN_T(h0; W, beta, GRU) through the HIP engine."""

    @staticmethod
    def forward(ctx, h0, engine, T, edge_keep, state_keep, seed, *path_weights):
        """path_weights: the six tensors of PATH_KEYS (edge_biases may be None)."""
        weights = {k: None if w is None else w.contiguous() for k, w in zip(PATH_KEYS, path_weights)}
        pack = engine.pack_weights(weights, T=T, edge_keep=edge_keep, seed=seed, batch=True)
        # (autograd runs Function.forward with grad mode off: ask the ctx)
        training = any(ctx.needs_input_grad)
        out = engine.forward(h0.contiguous(), pack, T, training=training, state_keep=state_keep)
        ctx.engine = engine
        ctx.generation = engine.generation
        beta = weights["edge_biases"]
        ctx.beta_shape = None if beta is None else tuple(path_weights[1].shape)
        ctx.pack = pack
        return out

    @staticmethod
    def backward(ctx, g_out):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("the engine ran another forward since this output was produced; "
                               "call backward before re-using the same call site")
        g = eng.backward(g_out.contiguous())
        if ctx.beta_shape is None:
            g["edge_biases"] = None
        elif g["edge_biases"] is not None:
            g["edge_biases"] = g["edge_biases"].view(ctx.beta_shape)
        return (g["h0"], None, None, None, None, None) + tuple(g[k] for k in PATH_KEYS)


class DenseGGNNChemModel(DecodingMixin, BtbBatching):
    """Hot-path subset of the reference's DenseGGNNChemModel (btb task)."""

    def __init__(self, args=None, params=None, num_edge_types=None, output_size_edges=12, pos_size=46,
                 bucket_max_nodes=120, device=None, seed=None, precision="fp32", vocab_size=1000, max_nodes=None,
                 embedding_sizes=None, rank=0, world_size=1, group=None):
        """rank, world_size, group: data-parallel training (one process per GPU,
        ``torch.distributed`` initialised by the caller, e.g. dist.init_from_env):
        run_epoch then draws this rank's share of every global step's batches
        and train_step sums the flat gradient buffer over the group (RCCL)."""
        self.args = dict(args or {"--pr": "btb"})
        self.rank, self.world_size, self.group = int(rank), int(world_size), group
        if not 0 <= self.rank < self.world_size:
            raise ValueError("rank %d outside world_size %d" % (self.rank, self.world_size))
        self.params = self.default_params()
        if params:
            self.params.update(params)
        kinds = tuple(_eval.TREE_LOSS_FAMILIES) + tuple(_eval.MARGIN_LOSS_KINDS)
        if self.params.get("structured_loss") not in (None,) + kinds:
            raise ValueError("params['structured_loss'] must be None or one of %s, got %r"
                             % (", ".join(repr(k) for k in kinds), self.params["structured_loss"]))
        try:
            _eval.margin_cost(self.params.get("structured_loss_margin", 1.0))
        except ValueError:
            raise ValueError("params['structured_loss_margin'] must be a number in 0..%g, got %r"
                             % (_eval.MARGIN_COST_MAX, self.params["structured_loss_margin"])) from None
        if self.params.get("structured_loss_single_root", True) not in (True, False):
            raise ValueError("params['structured_loss_single_root'] must be True or False, got %r"
                             % (self.params["structured_loss_single_root"],))
        if num_edge_types is None:
            raise ValueError("num_edge_types is required (len(dep_list)+1 in the reference, "
                             "chem_tensorflow.py:198)")
        self.num_edge_types = int(num_edge_types)
        self.output_size_edges = int(output_size_edges)
        self.pos_size = int(pos_size)
        self.bucket_max_nodes = int(bucket_max_nodes)
        # front-end sizes (chem_tensorflow.py:184-189; vocab/max_nodes come from
        # the treebank lists there).  The reference's concat is 80+50+100+80 =
        # 310 wide, so hidden_size < 310 needs smaller embeddings:
        # embedding_sizes = dict(loc=, pos=, word=, edge=)
        es = dict(loc=80, pos=50, word=100, edge=50)
        es.update(embedding_sizes or {})
        self.loc_embedding_size, self.pos_embedding_size = int(es["loc"]), int(es["pos"])
        self.word_embedding_size, self.edge_embedding_size = int(es["word"]), int(es["edge"])
        self.vocab_size = int(vocab_size)
        self.max_nodes = int(max_nodes if max_nodes is not None else self.bucket_max_nodes)
        self.precision = precision
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.placeholders = {}
        self.weights = {}
        self.ops = {}
        self._engines = {}
        self._up_labels, self._up_labels_e = Uploader(), Uploader()
        # the reference seeds Python's and numpy's global RNGs here
        # (chem_tensorflow.py:174-175): minibatch_schedule shuffles with the
        # global numpy RNG, so ranks of a data-parallel job that construct their
        # models alike run the same schedule (run_epoch checks that they do)
        random.seed(self.params["random_seed"])
        np.random.seed(self.params["random_seed"])
        rs = self.params["random_seed"] if seed is None else seed
        self._rng = np.random.RandomState(rs)
        self.prepare_specific_graph_model()

    # ------------------------------------------------------------- params
    def default_params(self):
        """chem_tensorflow.py:77-112 (btb) + chem_tensorflow_dense.py:152-161."""
        return {
            "batch_size": 20, "num_epochs": 200, "patience": 15, "learning_rate": 0.003,
            "clamp_gradient_norm": 1.0, "out_layer_dropout_keep_prob": 0.85, "emb_dropout_keep_prob": 0.55,
            "hidden_size": 400, "num_timesteps": 4, "use_graph": True, "tie_fwd_bkwd": True,
            "task_ids": [0], "random_seed": 0, "output_size": 150,
            "graph_state_dropout_keep_prob": 0.9, "task_sample_ratios": {}, "use_edge_bias": True,
            "edge_weight_dropout_keep_prob": 1,
            "compact_adjacency": False,   # not in the reference: edge-list feed (ggnn_set_adjacency_edges)
            "hip_graphs": True,           # not in the reference: captured steps for edge-list feeds (graphs.py)
            "hip_graph_cache_mb": 16384,  # not in the reference: device memory the captured steps may hold
            # not in the reference: the head's loss as the negative log-likelihood of the gold TREE
            # (None: the per-word cross-entropy; "nonprojective" / "projective": ggnn_tree_loss;
            # "nonprojective-margin" / "projective-margin": the structured hinge, ggnn_margin_loss,
            # with structured_loss_margin the cost of a wrong head)
            "structured_loss": None,
            "structured_loss_single_root": True,
            "structured_loss_margin": 1.0,
        }

    @property
    def num_channels(self) -> int:
        return 2 * self.num_edge_types

    # ------------------------------------------------------------ weights
    def prepare_specific_graph_model(self) -> None:
        """Create the path's variables with the reference's initialisers
        (chem_tensorflow_dense.py:202-212, GRUCell defaults :238)."""
        h, C = self.params["hidden_size"], self.num_channels
        dev = self.device
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev, requires_grad=True)
        self.weights["edge_weights"] = t(glorot_init([C, h, h], self._rng))
        self.weights["edge_weights_fixed"] = t(glorot_init([C, h, h], self._rng))
        if self.params["use_edge_bias"]:
            self.weights["edge_biases"] = t(np.zeros([C, 1, h], np.float32))
            self.weights["edge_biases_fixed"] = t(np.zeros([C, 1, h], np.float32))
        self.weights["node_gru"] = {
            "gates_kernel": t(glorot_init([2 * h, 2 * h], self._rng)),
            "gates_bias": t(np.ones([2 * h], np.float32)),
            "candidate_kernel": t(glorot_init([2 * h, h], self._rng)),
            "candidate_bias": t(np.zeros([h], np.float32)),
        }
        # front-end tables (chem_tensorflow_dense.py:214-235; tf.get_variable's
        # default initializer is glorot-uniform)
        self.weights["loc_embeddings"] = t(glorot_init([self.max_nodes, self.loc_embedding_size], self._rng))
        self.weights["head_loc_embeddings"] = t(glorot_init([self.max_nodes, self.loc_embedding_size], self._rng))
        self.weights["pos_embeddings"] = t(glorot_init([self.pos_size, self.pos_embedding_size], self._rng))
        self.weights["word_embeddings"] = t(glorot_init([self.vocab_size, self.word_embedding_size], self._rng))
        self.weights["edge_embeddings"] = t(glorot_init([self.num_edge_types + 1, self.edge_embedding_size],
                                                        self._rng))
        # out layers (chem_tensorflow.py:332-341): MLP(in, out, []) = one W, b;
        # the regression_transform MLPs are built but unused by btb (:466)
        o, oe = self.params["output_size"], self.output_size_edges
        for task_id in self.params["task_ids"]:
            for name, shape in (("regression_gate_task%i", [2 * h, o]), ("regression_gate_task_edges%i", [2 * h, oe]),
                                ("regression_transform_task%i", [h, o]),
                                ("regression_transform_task_edges%i", [h, oe])):
                self.weights[name % task_id] = {"weights": [t(mlp_init(shape, self._rng))],
                                                "biases": [t(np.zeros([shape[1]], np.float32))]}
        # the library's front-end, the eager path's heads and the decoder load
        # libggnn.so: created on first use (_embedder, _output_heads, _decode_heads)
        self._front_end = None
        self._heads = None
        self._decoder = None
        self._up_nodes = Uploader()
        self._up_loss_nodes = Uploader()   # the structured loss's node counts (the eager paths)
        self._last_labels = None  # the last forward's labels on the device: the decode's gold inputs
        # the last forward's dropout draws, by stage (keep probabilities, seed, ...)
        self.last_embed = self.last_dropout = self.last_heads = None
        # the epoch loops' device -> host fetches: run_epoch's (loss, both
        # heads' probabilities) and score_epoch's (loss, decode counts)
        self._fetch_probs, self._fetch_counts = PinnedFetch(), PinnedFetch()
        self.decode_stats = {"graphs": 0, "fallback_graphs": 0, "d2h_bytes": 0, "repaired_graphs": 0,
                             "infeasible_graphs": 0}
        self._flat = None
        self._rows = None          # the word segment's lookup rows / ids (sparse data-parallel reduction)
        # hipGraph-captured steps by batch shape (graphs.py), least recently
        # used first; bounded by params['hip_graph_cache_mb'] (_evict_graphs)
        self._graphs = OrderedDict()
        self._ring = PinnedRing()
        # batches by path: captured-step replays, first batches of a shape
        # (eager, on the step's device inputs), the plain eager path
        self.graph_stats = {"captured": 0, "replayed": 0, "uncaptured": 0, "eager": 0, "evicted": 0, "cache_bytes": 0}
        self.lookup_sqnorm = {}
        self.optimizer = None

    def _seed(self) -> int:
        """A fresh 64-bit Philox seed from the model's RandomState (a new mask
        per step, like TF's stateful RNG).  Rank r of a data-parallel job XORs
        a rank constant in, so the ranks' masks are independent (rank 0, and a
        single process, keep the plain draw)."""
        s = int(self._rng.randint(0, 2 ** 31 - 1)) << 32 | int(self._rng.randint(0, 2 ** 31 - 1))
        return s ^ ((self.rank * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)

    def _embedder(self) -> EmbeddingFrontEnd:
        if self._front_end is None:
            self._front_end = EmbeddingFrontEnd(self.params["hidden_size"])
        return self._front_end

    def _output_heads(self) -> OutputHeads:
        """The eager path's heads (a captured step has its own workspace)."""
        if self._heads is None:
            self._heads = OutputHeads(self.params["hidden_size"])
        return self._heads

    def _decode_heads(self) -> OutputHeads:
        if self._decoder is None:
            self._decoder = OutputHeads(self.params["hidden_size"])
        return self._decoder

    def _path_weights(self, fixed=False) -> dict:
        """The path's six weights (PATH_KEYS) as the dict the engine takes;
        ``fixed``: the ``*_fixed`` edge weights / biases."""
        W, sfx = self.weights, "_fixed" if fixed else ""
        wts = {"edge_weights": W["edge_weights" + sfx],
               "edge_biases": W["edge_biases" + sfx] if self.params["use_edge_bias"] else None}
        wts.update((k, W["node_gru"][k]) for k in GRU_KEYS)
        return wts

    def parameters(self):
        ps = [self.weights["edge_weights"], self.weights["edge_weights_fixed"]]
        if self.params["use_edge_bias"]:
            ps += [self.weights["edge_biases"], self.weights["edge_biases_fixed"]]
        ps += [self.weights["node_gru"][k] for k in GRU_KEYS]
        return ps

    def trainable_variables(self):
        """The variables the btb loss reaches (TF passes None gradients for the
        rest: the *_fixed twins, head_loc/edge embeddings, regression_transform)."""
        ps = [self.weights["edge_weights"]]
        if self.params["use_edge_bias"]:
            ps.append(self.weights["edge_biases"])
        ps += [self.weights["node_gru"][k] for k in GRU_KEYS]
        ps += [self.weights[k] for k in ("loc_embeddings", "pos_embeddings", "word_embeddings")]
        for task_id in self.params["task_ids"]:
            for name in ("regression_gate_task%i", "regression_gate_task_edges%i"):
                mlp = self.weights[name % task_id]
                ps += [mlp["weights"][0], mlp["biases"][0]]
        return ps

    # -------------------------------------------------------------- feeds
    def feed(self, feed_dict: dict) -> None:
        """Stage one minibatch (a dict from ``make_minibatch_iterator`` or any
        dict with ``adjacency_matrix``, ``num_vertices``, ``num_graphs``)."""
        adj = feed_dict.get("adjacency_matrix")
        self.placeholders = dict(feed_dict)
        if adj is None:
            # compact feed: edge lists only (params['compact_adjacency'])
            if feed_dict.get("adjacency_edges") is None:
                raise ValueError("feed needs adjacency_matrix or adjacency_edges")
            self.placeholders["adjacency_matrix"] = None
            return
        if not isinstance(adj, torch.Tensor):
            adj = torch.from_numpy(np.ascontiguousarray(np.asarray(adj, dtype=np.float32)))
        adj = adj.to(device=self.device, dtype=torch.float32).contiguous()
        self.placeholders["adjacency_matrix"] = adj
        b, C, v, _ = adj.shape
        if C != self.num_channels:
            raise ValueError("adjacency has %d channels, model expects 2*num_edge_types = %d" % (C, self.num_channels))
        if int(feed_dict.get("num_vertices", v)) != v or int(feed_dict.get("num_graphs", b)) != b:
            raise ValueError("num_vertices/num_graphs disagree with adjacency shape %s" % (tuple(adj.shape),))

    def _engine(self, site):
        key = (self.params["hidden_size"], self.num_channels, bool(self.params["use_edge_bias"]), site)
        eng = self._engines.get(key)
        if eng is None:
            eng = self._engines[key] = self._new_engine()      # one per call site
        return eng

    def _new_engine(self) -> PropagationEngine:
        return PropagationEngine(self.params["hidden_size"], self.num_channels, bool(self.params["use_edge_bias"]),
                                 device=self.device, precision=self.precision)

    # ------------------------------------------------------------ hot path
    def compute_final_node_representations(self, initial_node_representations, fixed_ts=None):
        """[b, v, h] -> [b, v, h] after T = num_timesteps (or fixed_ts) GGNN
        steps (chem_tensorflow_dense.py:312-340).  ``fixed_ts`` selects the
        ``*_fixed`` edge weights/biases, as compute_timestep_fast does (:396-412)."""
        if "adjacency_matrix" not in self.placeholders and "adjacency_edges" not in self.placeholders:
            raise RuntimeError("feed() a minibatch before compute_final_node_representations()")
        # --old (compute_timestep_normal, :350-389) is the same contraction in
        # another summation order with element-wise independent edge-weight
        # dropout, so the engine serves it too (tests: oracle ordering="old");
        # the identity task is out of scope
        if self.args.get("--pr", "btb") != "btb":
            raise NotImplementedError("only --pr btb is supported by the engine")
        T = self.params["num_timesteps"] if fixed_ts is None else int(fixed_ts)
        # compute_timestep_fast picks the *_fixed twins when fixed_ts is given
        # (:396-412); compute_timestep_normal (--old, :350-389) always uses the
        # main edge_weights / edge_biases
        fixed = fixed_ts is not None and not self.args.get("--old")
        h0 = initial_node_representations
        if not isinstance(h0, torch.Tensor):
            h0 = torch.from_numpy(np.ascontiguousarray(np.asarray(h0, dtype=np.float32)))
        h0 = h0.to(device=self.device, dtype=torch.float32)
        eng = self._engine("main" if fixed_ts is None else "fixed")
        self._stage_adjacency(eng)
        # dropout as fed (chem_tensorflow_dense.py:860-861 training, :938-940 eval);
        # a fresh Philox seed per call = fresh masks per step, like TF's stateful RNG
        edge_keep, state_keep = self._path_keeps()
        seed = self._seed()
        out = _Propagate.apply(h0, eng, T, edge_keep, state_keep, seed, *self._path_weights(fixed).values())
        self.last_dropout = dict(edge_keep=edge_keep, state_keep=state_keep, seed=seed)
        self.ops["final_node_representations" if fixed_ts is None else "second_node_representations"] = out
        return out

    def _stage_adjacency(self, eng) -> None:
        if self.placeholders["adjacency_matrix"] is not None:
            eng.set_adjacency(self.placeholders["adjacency_matrix"])
        else:
            eng.set_adjacency_edges(self.placeholders["adjacency_edges"], int(self.placeholders["num_vertices"]),
                                    self.num_edge_types)

    def _path_keeps(self):
        """(edge_weight_dropout_keep_prob, graph_state_keep_prob) as fed."""
        return (float(self.placeholders.get("edge_weight_dropout_keep_prob", 1.0)),
                float(self.placeholders.get("graph_state_keep_prob", 1.0)))

    # ------------------------------------------------- §8f rank 1: callers
    def _front_end_segments(self):
        """(tables, word_inputs columns) of the btb front-end in concat order."""
        W = self.weights
        return (W["loc_embeddings"], W["pos_embeddings"], W["word_embeddings"], W["loc_embeddings"]), (0, 1, 2, 3)

    def get_initial_node_representation(self):
        """btb front-end (chem_tensorflow_dense.py:264-306): lookups of
        word_inputs columns 0 (loc), 1 (pos), 2 (word), 3 (head loc, the loc
        table again), each dropped out with emb_dropout_keep_prob, concatenated
        and zero-padded to hidden_size.  Columns 4, 5 (head POS, edge) are
        looked up by the reference but unused; they are not gathered here."""
        if "word_inputs" not in self.placeholders:
            raise RuntimeError("feed() a minibatch with word_inputs first")
        self._check_front_end_width()
        tables, cols = self._front_end_segments()
        wi = word_inputs_tensor(self.placeholders["word_inputs"], self.device,
                                {c: tb.shape[0] for tb, c in zip(tables, cols)})
        keep = float(self.placeholders.get("emb_dropout_keep_prob", 1.0))
        seed = self._seed()
        h0 = EmbedFunction.apply(self._embedder(), self, wi, keep, seed, cols, *tables)
        self.last_embed = dict(keep=keep, seed=seed)
        self.ops["initial_node_representations"] = h0
        return h0

    def build_loss(self, task_id=0):
        """make_model for btb (chem_tensorflow.py:326-421): h0 -> h_T -> both
        gated_regression heads on [h_T, h0] -> loss = heads CE + edges CE, each
        over task_target_num = sum(target_mask[task]) + SMALL_NUMBER."""
        h0 = self.get_initial_node_representation()
        hT = self.compute_final_node_representations(h0)
        b, v, _ = hT.shape
        o, oe = self.params["output_size"], self.output_size_edges
        labels = self._head_labels(b, v)
        target_num = float(self._target_count(task_id) + SMALL_NUMBER)
        keep = self._out_keep()
        seed = self._seed()
        (gw, gb), (gew, geb) = self._heads_list(task_id)
        n = self._loss_n_nodes(self.placeholders)
        tree_loss = self._tree_loss_arg(None if n is None else self._up_loss_nodes(n, self.device))
        oh = self._output_heads()
        loss, probs, probs_e = HeadsFunction.apply(oh, labels, keep, seed, target_num, tree_loss, hT, h0,
                                                   gw, gb, gew, geb)
        self.ops["tree_loss_used"] = oh.tree_used
        self.ops["margin_loss_hamming"] = oh.margin_hamming
        self.ops["loss"] = loss
        self.ops["computed_values"] = probs.reshape(b, v * o)
        self.ops["computed_values_edges"] = probs_e.reshape(b, v * oe)
        self.last_heads = dict(keep=keep, seed=seed, target_num=target_num)
        return loss

    def _head_labels(self, b, v):
        """The two heads' targets [b, v, o] / [b, v, e_o] on the device
        (placeholders target_values_head / _edges, chem_tensorflow.py:372-376)."""
        o, oe = self.params["output_size"], self.output_size_edges
        if v > o:
            raise ValueError("num_vertices %d > output_size %d" % (v, o))
        y_h = self._up_labels(np.asarray(self.placeholders["target_values_head"], np.float32).reshape(b, v, o),
                              self.device)
        y_e = self._up_labels_e(np.asarray(self.placeholders["target_values_edges"], np.float32).reshape(b, v, oe),
                                self.device)
        self._last_labels = [y_h, y_e]     # (the decode's gold inputs: _decode_forward)
        return [y_h, y_e]

    def _target_count(self, task_id=0) -> float:
        """sum(target_mask[task]) of the staged batch (chem_tensorflow.py:358-360)."""
        tmask = np.asarray(self.placeholders["target_mask"], np.float64)
        return float(tmask[self.params["task_ids"].index(task_id)].sum())

    def _structured(self):
        """params['structured_loss'] as (family, single_root) of ggnn_tree_loss,
        as (family, single_root, cost) of ggnn_margin_loss, or None (off)."""
        kind = self.params.get("structured_loss")
        if kind is None:
            return None
        single_root = bool(self.params.get("structured_loss_single_root", True))
        if kind in _eval.MARGIN_LOSS_KINDS:
            return (_eval.MARGIN_LOSS_KINDS[kind], single_root,
                    _eval.margin_cost(self.params.get("structured_loss_margin", 1.0)))
        return _eval.TREE_LOSS_FAMILIES[kind], single_root

    def _loss_n_nodes(self, ph):
        """The node counts the structured loss runs on: _feed_n_nodes, and 0 for
        every graph of a feed whose masks are not in closed form (the local
        loss for that batch); None with params['structured_loss'] off."""
        if self._structured() is None:
            return None
        n = self._feed_n_nodes(ph)
        return np.zeros(int(ph["num_graphs"]), np.int32) if n is None else n.astype(np.int32)

    def _tree_loss_arg(self, n_nodes):
        """OutputHeads.forward's tree_loss= for device node counts (None: off)."""
        st = self._structured()
        return None if st is None or n_nodes is None else st[:2] + (n_nodes,) + st[2:]

    def _out_keep(self) -> float:
        return float(self.placeholders.get("out_layer_dropout_keep_prob", self.params["out_layer_dropout_keep_prob"]))

    def _heads_list(self, task_id=0):
        g = self.weights["regression_gate_task%i" % task_id]
        ge = self.weights["regression_gate_task_edges%i" % task_id]
        return [(g["weights"][0], g["biases"][0]), (ge["weights"][0], ge["biases"][0])]

    def train_buffer(self) -> FlatTrainBuffer:
        """The flat gradient / lookup-norm / loss buffer of train_step.  The
        output heads' gradients and the losses come first (one bucket, final
        before the propagation backward); with world_size > 1 and
        params['sparse_embedding_reduce'] the word table's gradient sits past
        the dense part: it is reduced as IndexedSlices (_sparse_reduce)."""
        if self._flat is None:
            params = self.trainable_variables()
            ids = {id(p): i for i, p in enumerate(params)}
            first = [ids[id(t)] for tid in self.params["task_ids"] for hw in self._heads_list(tid) for t in hw]
            sparse = [ids[id(self.weights["word_embeddings"])]] if self._sparse_reduce_on() else []
            self._flat = FlatTrainBuffer(params, n_sq=4, n_loss=2, device=self.device, first=first, sparse=sparse)
        return self._flat

    def _sparse_reduce_on(self) -> bool:
        return self.world_size > 1 and bool(self.params.get("sparse_embedding_reduce", True))

    def _lookup_rows(self):
        """The word segment's per-lookup gradient rows and ids of this rank's
        batch (persistent buffers of capacity batch_size * bucket_max_nodes,
        the same on every rank: what the ranks all-gather)."""
        if self._rows is None:
            cap = int(self.params["batch_size"]) * int(self.bucket_max_nodes)
            w = self.weights["word_embeddings"].shape[1]
            self._rows = (torch.zeros((cap, w), dtype=torch.float32, device=self.device),
                          torch.full((cap,), -1, dtype=torch.int32, device=self.device))
        return self._rows

    @staticmethod
    def _sparse_call(fl, reducer) -> bool:
        """Whether THIS step reduces the word table as IndexedSlices: the
        buffer has the sparse region and the reducer can gather (a
        dist.Reducer).  Without a reducer (a local step) or with a plain
        callable, the word table's gradient is written densely into its view
        of the buffer (and a plain callable all-reduces the whole buffer)."""
        return bool(fl.sparse) and reducer is not None and hasattr(reducer, "gather")

    def _reduce(self, fl, reducer, started=None) -> None:
        """The data-parallel reduction of one step's flat buffer: the dense
        part as (heads + losses) and the rest -- the first bucket possibly
        started already (``started``: its handle) -- and, with the sparse
        reduction on (_sparse_call), the word table as the union of every
        rank's lookups: the ranks' (rows, ids) all-gathered, accumulated in
        fixed point (exact, so the same bits on every rank).  A plain
        callable reducer sums the whole buffer in one blocking call (the word
        table dense, as the step wrote it)."""
        sparse = self._sparse_call(fl, reducer)
        if not hasattr(reducer, "start"):          # a plain callable: one blocking all-reduce
            reducer(fl.flat)
        else:
            b0, b1 = fl.buckets
            h0 = started if started is not None else reducer.start(b0)
            reducer(b1)
            reducer.wait(h0)
        if sparse:
            rows, ids = self._lookup_rows()
            g_rows, g_ids = reducer.gather(rows), reducer.gather(ids)
            word = self.weights["word_embeddings"]
            tables = self._front_end_segments()[0]
            slot = next(i for i, t in enumerate(tables) if t is word)
            self._embedder().union_backward(word, fl.grads[fl.sparse[0]], g_rows.view(-1, word.shape[1]),
                                            g_ids.view(-1), fl.sq[slot:slot + 1])

    def train_step(self, feed_dict=None, grad_scale=1.0, all_reduce=None, target_count=None, task_id=0):
        """One training step (chem_tensorflow.py:483-506 + run_epoch's
        sess.run of train_step): front-end -> propagation -> heads -> loss,
        the backward of each, per-variable clip_by_norm, Adam.  Returns the
        loss (a device scalar).

        Every gradient lands in ONE flat fp32 buffer (``train_buffer()``: all
        trainable variables, the embedding tables' IndexedSlices norms and the
        per-head losses), written in place by the library's backward calls.

        Data parallel (``all_reduce``: a callable summing a tensor over the
        ranks; run_epoch passes it when world_size > 1): the loss of a global
        step is the reference's btb loss (chem_tensorflow.py:358-360,399-403)
        over the UNION of the ranks' batches, i.e. every rank normalises its
        cross-entropy by the global ``target_count`` (sum of target_mask over
        all ranks' graphs; the feed's ``global_target_count`` from the sharded
        iterator) + SMALL_NUMBER.  Then the per-rank gradients, lookup norms
        (sum of squared rows of the concatenated IndexedSlices) and losses
        simply add: one all-reduce of the flat buffer, and clip + Adam on the
        sums with grad_scale 1.  With dropout off this equals one process
        stepping the concatenated batch.  A feed with num_graphs == 0 (a rank
        without a batch in the last global step) contributes zeros.

        Aliasing: on a captured step (_graph_step) without an all-reduce the
        returned loss, ``ops["loss"]`` and ``ops["computed_values"]`` /
        ``["computed_values_edges"]`` are the graph's static outputs, so the
        next replay of the same shape overwrites them in place (stream
        ordered).  Clone or fetch what must outlive the next step, as run_epoch
        does (tests/test_gpu_graph_lifecycle.py pins this)."""
        if feed_dict is not None and int(feed_dict.get("num_graphs", 1)) == 0:
            return self._empty_train_step(all_reduce, grad_scale)
        if feed_dict is not None and self._graph_ok(feed_dict):
            loss = self._graph_step(feed_dict, True, task_id, target_count, all_reduce, grad_scale)
            if loss is not None:
                return loss
        self.graph_stats["eager"] += 1
        if feed_dict is not None:
            self.feed(feed_dict)
        if target_count is None:
            target_count = self.placeholders.get("global_target_count")
        fl = self.train_buffer()
        params = self.trainable_variables()
        started = []
        self._forward_backward(fl, params, None if target_count is None else float(target_count), task_id,
                               reducer=all_reduce, started=started)
        if all_reduce is not None:
            self._reduce(fl, all_reduce, started[0] if started else None)
        self._apply_gradients(fl, params, grad_scale)
        return fl.loss.sum()

    def _empty_train_step(self, all_reduce, grad_scale):
        fl = self.train_buffer()
        fl.zero_()
        if self._sparse_call(fl, all_reduce):   # no lookups of this rank in the union
            self._lookup_rows()[0].zero_()
            self._lookup_rows()[1].fill_(-1)
        if all_reduce is not None:
            self._reduce(fl, all_reduce)
        self._apply_gradients(fl, self.trainable_variables(), grad_scale)
        return fl.loss.sum()

    # ------------------------------------------- hipGraph capture (graphs.py)
    def _graph_ok(self, feed) -> bool:
        """Whether a feed can run as a captured step: a compact (edge-list)
        batch on the GPU, params['hip_graphs'] on."""
        return (bool(self.params.get("hip_graphs", True)) and self.device.type == "cuda"
                and feed.get("adjacency_matrix") is None and feed.get("adjacency_edges") is not None
                and "word_inputs" in feed and int(feed.get("num_graphs", 0)) > 0
                and self.args.get("--pr", "btb") == "btb")

    def _graph_step(self, feed, training, task_id=0, target_count=None, all_reduce=None, grad_scale=1.0):
        """One batch through its shape's captured step: stage the batch's
        inputs (one H2D copy), then replay the shape's graph.  Training: the
        train_step body (+ clip + Adam inside the graph when there is no
        all-reduce; otherwise the all-reduce and Adam follow eagerly).
        Evaluation: the build_loss forward.  Returns the loss (device
        scalar), or None when the batch does not fit a captured step (more
        edges than the b * v capacity).  A shape's first batch runs the body
        eagerly; its second is captured and replayed; later ones replay."""
        self.feed(feed)
        self._check_front_end_width()
        ph = self.placeholders
        b, v = int(ph["num_graphs"]), int(ph["num_vertices"])
        o, oe = self.params["output_size"], self.output_size_edges
        if v > o:
            raise ValueError("num_vertices %d > output_size %d" % (v, o))
        tables, cols = self._front_end_segments()
        wi = np.asarray(ph["word_inputs"]).astype(np.int64)
        for tb, c in zip(tables, cols):
            x = wi[..., c]
            if x.size and (x.min() < 0 or x.max() >= tb.shape[0]):
                raise IndexError("word_inputs[..., %d] holds index %d outside [0, %d)"
                                 % (c, int(x.max() if x.max() >= tb.shape[0] else x.min()), tb.shape[0]))
        edges, offs = edge_arrays(ph["adjacency_edges"], v, self.num_edge_types)
        if edges.shape[0] > b * v:
            return None
        if target_count is None:
            target_count = ph.get("global_target_count") if training else None
        count = self._target_count(task_id) if target_count is None else float(target_count)
        target_num = float(count + SMALL_NUMBER)
        keeps = (float(ph.get("emb_dropout_keep_prob", 1.0)),) + self._path_keeps() + (self._out_keep(),)
        adam = training and all_reduce is None
        # (grad_scale is baked into the captured Adam launch: part of the key)
        # (the word table's layout, dense or IndexedSlices, is captured too)
        sparse = bool(training) and self._sparse_call(self.train_buffer(), all_reduce)
        if training:
            fl = self.train_buffer()
            params = self.trainable_variables()
            if self.optimizer is None:
                self.make_optimizer()
        # (the host scalars a launch takes by value are part of the key too:
        # the number of timesteps, and Adam's rates and clip norm when Adam is
        # in the graph; a change captures a fresh step, the old one ages out)
        opt = self.optimizer
        baked = (int(self.params["num_timesteps"]),) + ((opt.lr, opt.b1, opt.b2, opt.eps, opt.clip) if adam else ())
        # (the structured loss's family and root mode are launch arguments too)
        key = (bool(training), adam, b, v, wi.shape[-1], keeps, task_id, float(grad_scale) if adam else 1.0, sparse,
               baked, self._structured())
        cs = self._graphs.get(key)
        if cs is None:
            cs = self._graphs[key] = CapturedStep(StepLayout(b, v, wi.shape[-1], o, oe), self._new_engine(),
                                                  OutputHeads(self.params["hidden_size"]), self.device)
        self._graphs.move_to_end(key)
        seeds = [self._seed() for _ in range(3)]
        step = 0
        if adam:
            self.optimizer.t += 1
            step = self.optimizer.t
        # stage the batch: pinned host buffer -> the step's device inputs
        L = cs.layout
        i, host = self._ring.acquire(L.nbytes)
        L.fill(host.numpy(), seeds, step, target_num, wi.astype(np.int32), edges, offs,
               np.asarray(ph["target_values_head"], np.float32), np.asarray(ph["target_values_edges"], np.float32),
               n_nodes=self._loss_n_nodes(ph))
        stream = torch.cuda.current_stream(self.device)
        cs.inputs.buf[:L.nbytes].copy_(host, non_blocking=True)
        self._ring.release(i, stream)
        inp = cs.inputs
        sf = _StepFeed(inp.wi, tuple(inp.seed_address(k) for k in range(3)), tuple(seeds), True, [inp.yh, inp.ye],
                       inp.target_num, cs.engine, cs.heads,
                       lambda eng: eng.set_adjacency_edges((inp.edges, inp.offs), v, self.num_edge_types), b, v,
                       target_num_value=target_num, n_nodes=inp.n_nodes)

        def body():
            if training:
                # (the reducer only decides the word table's layout here: the
                # collectives run after the replay, RCCL is not captured)
                probs = self._forward_backward(fl, params, None, task_id, sf, reducer=None if adam else all_reduce)
                if adam:
                    self._apply_gradients(fl, params, grad_scale, step_dev=inp.step)
                loss = fl.loss.sum()
            else:
                _, _, probs, loss = self._forward(sf, task_id, training=False)
                loss = loss.sum()
            return {"loss": loss, "probs": probs, "used": cs.heads.tree_used, "hamming": cs.heads.margin_hamming}

        if cs.graph is None and cs.runs == 0:
            # a shape's first batch runs eagerly (on the same device inputs):
            # one-off shapes never pay for a capture
            out = body()
            self.graph_stats["uncaptured"] += 1
        else:
            if cs.graph is None:             # its second batch: capture, then replay
                g = torch.cuda.CUDAGraph()
                before = torch.cuda.memory_allocated(self.device)
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    cs.out = body()          # recorded, not executed
                cs.graph = g
                # the activations the captured body allocated live in the
                # graph's private pool for as long as the graph does
                cs.pool_bytes = max(torch.cuda.memory_allocated(self.device) - before, 0)
                self.graph_stats["captured"] += 1
                self._evict_graphs(keep=key)
            cs.graph.replay()
            out = cs.out
            self.graph_stats["replayed"] += 1
            # (a replay runs none of the body's Python: this batch's draws, as
            # _forward records them)
            self.last_embed = dict(keep=keeps[0], seed=seeds[0])
            self.last_dropout = dict(edge_keep=keeps[1], state_keep=keeps[2], seed=seeds[1])
            self.last_heads = dict(keep=keeps[3], seed=seeds[2], target_num=target_num)
        cs.runs += 1
        if cs.runs == 1:
            self._evict_graphs(keep=key)
        probs = out["probs"]
        self.ops["computed_values"] = probs[0].reshape(b, v * o)
        self.ops["computed_values_edges"] = probs[1].reshape(b, v * oe)
        self.ops["tree_loss_used"] = out["used"]
        self.ops["margin_loss_hamming"] = out["hamming"]
        self._last_labels = [inp.yh, inp.ye]
        loss = out["loss"]
        if training and not adam:
            self._reduce(fl, all_reduce)
            self._apply_gradients(fl, params, grad_scale)
            # the union-batch loss: the graph's loss sum was taken before the
            # all-reduce (this rank's share), the eager path's after it
            loss = fl.loss.sum()
        self.ops["loss"] = loss
        return loss

    def _evict_graphs(self, keep=None) -> None:
        """Drop the least recently used captured steps (their graph, engine
        workspaces, heads workspace and input buffer) while the cache holds
        more than params['hip_graph_cache_mb'] of device memory.  Bucketed
        treebanks have a full and a tail batch shape per bucket, for training
        and evaluation; unbounded, their workspaces (~0.9 GB at hidden 400,
        b = 20, v = 120) grew to tens of GB per process."""
        budget = float(self.params.get("hip_graph_cache_mb", 16384)) * 2 ** 20
        total = sum(cs.nbytes() for cs in self._graphs.values())
        while total > budget and len(self._graphs) > 1:
            k = next(iter(self._graphs))
            if k == keep:
                self._graphs.move_to_end(k)
                k = next(iter(self._graphs))
            cs = self._graphs.pop(k)
            total -= cs.nbytes()
            cs.release()
            self.graph_stats["evicted"] += 1
        self.graph_stats["cache_bytes"] = int(total)

    def _forward(self, sf, task_id, training, loss_out=None):
        """The forward of one step on a _StepFeed, without autograd: front-end
        (chem_tensorflow_dense.py:264-306) -> T-step propagation (:312-340) ->
        heads + btb loss (:439-516, chem_tensorflow.py:326-421).  ``training``
        keeps what the engine's backward reads; ``loss_out``: where the heads
        write the two losses.  Returns (h0, hT, probs, the two heads' losses)."""
        segs = list(zip(*self._front_end_segments()))
        keep_e = float(self.placeholders.get("emb_dropout_keep_prob", 1.0))
        h0 = self._embedder().forward(segs, sf.wi, keep_e, sf.seeds[0], seed_device=sf.seed_device)
        self.last_embed = dict(keep=keep_e, seed=sf.seed_values[0])
        T = self.params["num_timesteps"]
        eng = sf.engine
        sf.stage(eng)
        edge_keep, state_keep = self._path_keeps()
        pack = eng.pack_weights(self._path_weights(), T=T, edge_keep=edge_keep, seed=sf.seeds[1],
                                seed_device=sf.seed_device, batch=True)
        hT = eng.forward(h0, pack, T, training=training, state_keep=state_keep)
        self.last_dropout = dict(edge_keep=edge_keep, state_keep=state_keep, seed=sf.seed_values[1])
        keep_o = self._out_keep()
        probs, loss = sf.heads.forward(hT, h0, self._heads_list(task_id), sf.labels, keep_o, sf.seeds[2],
                                       sf.target_num, loss_out=loss_out, seed_device=sf.seed_device,
                                       tree_loss=self._tree_loss_arg(sf.n_nodes))
        self.ops["tree_loss_used"] = sf.heads.tree_used
        self.ops["margin_loss_hamming"] = sf.heads.margin_hamming
        self.last_heads = dict(keep=keep_o, seed=sf.seed_values[2], target_num=sf.target_num_value)
        return h0, hT, probs, loss

    def _apply_gradients(self, fl, params, grad_scale, step_dev=None):
        if self.optimizer is None:
            self.make_optimizer()
        tables = self._front_end_segments()[0]
        # the tables' squared lookup norms (first segment's slot per table)
        slot = {}
        for i, t in enumerate(tables):
            slot.setdefault(id(t), i)
        self.lookup_sqnorm = {k: fl.sq[i:i + 1] for k, i in slot.items()}
        sq = [self.lookup_sqnorm.get(id(p)) for p in params]
        for p, g in zip(params, fl.grads):
            p.grad = g
        self.optimizer.step(fl.grads, grad_scale=grad_scale, sqnorms=sq, step_dev=step_dev)

    def _eager_step_feed(self, task_id, target_count) -> "_StepFeed":
        """The staged batch's inputs as device tensors uploaded now, with
        fresh seed values (drawn in build_loss's order: front-end, path,
        heads) and the host target_num."""
        tables, cols = self._front_end_segments()
        wi = word_inputs_tensor(self.placeholders["word_inputs"], self.device,
                                {c: tb.shape[0] for tb, c in zip(tables, cols)})
        seeds = (self._seed(), self._seed(), self._seed())
        b, v = int(self.placeholders["num_graphs"]), int(self.placeholders["num_vertices"])
        labels = self._head_labels(b, v)
        count = self._target_count(task_id) if target_count is None else target_count
        n = self._loss_n_nodes(self.placeholders)
        return _StepFeed(wi, seeds, seeds, False, labels, float(count + SMALL_NUMBER), self._engine("main"),
                         self._output_heads(), self._stage_adjacency, b, v,
                         n_nodes=None if n is None else self._up_loss_nodes(n, self.device))

    def _check_front_end_width(self):
        width = self.loc_embedding_size * 2 + self.pos_embedding_size + self.word_embedding_size
        if width > self.params["hidden_size"]:
            raise ValueError("embedding concat width %d > hidden_size %d: the reference's tf.pad fails here "
                             "(SURVEY F7); pass smaller embedding_sizes" % (width, self.params["hidden_size"]))

    def _forward_backward(self, fl, params, target_count, task_id, sf=None, reducer=None, started=None):
        """The btb loss and every gradient of one staged batch, written into
        the flat buffer ``fl`` (no autograd: each backward of the library
        writes its outputs where the optimizer reads them).  ``sf``: the
        step's inputs (_StepFeed; default: uploaded from the placeholders).
        Returns the heads' probabilities."""
        if "word_inputs" not in self.placeholders:
            raise RuntimeError("feed() a minibatch with word_inputs first")
        if self.args.get("--pr", "btb") != "btb":
            raise NotImplementedError("only --pr btb is supported by the engine")
        self._check_front_end_width()
        if sf is None:
            sf = self._eager_step_feed(task_id, target_count)
        # the word table's reduction is decided per call: sparse
        # only when a gathering reducer follows; checked before any work or
        # collective is issued, so a rank cannot leave a step its peers wait in
        sparse = self._sparse_call(fl, reducer)
        if sparse:
            cap = self._lookup_rows()[0].shape[0]
            if sf.b * sf.v > cap:
                raise ValueError("batch of %d x %d nodes exceeds the word lookup-row capacity %d (batch_size x "
                                 "bucket_max_nodes)" % (sf.b, sf.v, cap))
        h0, hT, probs, _ = self._forward(sf, task_id, training=True, loss_out=fl.loss)
        b, v, _ = hT.shape
        o, oe = self.params["output_size"], self.output_size_edges
        self.ops["initial_node_representations"], self.ops["final_node_representations"] = h0, hT
        self.ops["computed_values"] = probs[0].reshape(b, v * o)
        self.ops["computed_values_edges"] = probs[1].reshape(b, v * oe)
        gv = {id(p): g for p, g in zip(params, fl.grads)}
        hl = self._heads_list(task_id)
        _, _, dhT, dh0_heads = sf.heads.backward(hT, h0, hl, sf.labels, probs, sf.target_num,
                                                  dws=[gv[id(w)] for w, _ in hl], dbs=[gv[id(bb)] for _, bb in hl])
        if reducer is not None and started is not None and hasattr(reducer, "start"):
            # the heads' gradients and the losses are final: their reduction
            # runs on the collective's stream while the propagation backward runs
            started.append(reducer.start(fl.buckets[0]))
        # the path's backward (TF autodiff, chem_tensorflow.py:496) into the weights' views of the buffer
        eg = {k: None if w is None else gv[id(w)] for k, w in self._path_weights().items()}
        eg["h0"] = torch.empty_like(h0)
        sf.engine.backward(dhT, eg)
        # the tables' gradients + IndexedSlices norms (h0 feeds the path and the heads)
        tables, cols = self._front_end_segments()
        segs, keep_e = list(zip(tables, cols)), self.last_embed["keep"]
        word = self.weights["word_embeddings"]
        dts = [None if (sparse and t is word) else gv[id(t)] for t in tables]
        self._embedder().backward(segs, sf.wi, eg["h0"], keep_e, sf.seeds[0], dh0_add=dh0_heads,
                                  dtables=dts, sq_out=fl.sq, seed_device=sf.seed_device)
        if sparse:
            # the word table as IndexedSlices (rows, ids): all-gathered by _reduce
            rows, ids = self._lookup_rows()
            slot = next(i for i, t in enumerate(tables) if t is word)
            self._embedder().lookup_rows(segs, slot, sf.wi, eg["h0"], keep_e, sf.seeds[0], rows, ids,
                                         dh0_add=dh0_heads, seed_device=sf.seed_device)
        return probs

    def make_optimizer(self) -> ClipAdam:
        """The reference's train step optimizer (chem_tensorflow.py:494-503) over
        ``trainable_variables()``: clip_by_norm(clamp_gradient_norm) + Adam."""
        self.optimizer = ClipAdam(self.trainable_variables(), learning_rate=self.params["learning_rate"],
                                  clamp_gradient_norm=self.params["clamp_gradient_norm"])
        self._graphs.clear()          # captured steps hold the old slots' addresses
        return self.optimizer

    # ------------------------------------------------- checkpoint / evaluation
    def save_progress(self, model_path: str, train_step: int, valid_step: int) -> None:
        """chem_tensorflow.py:796-809 (checkpoint.py)."""
        _ckpt.save_progress(self, model_path, train_step, valid_step)

    def restore_progress(self, model_path: str):
        """chem_tensorflow.py:816-855 (checkpoint.py); returns (train_step, valid_step)."""
        return _ckpt.restore_progress(self, model_path)

    get_las_uas = staticmethod(_eval.get_las_uas)  # chem_tensorflow_dense.py:1304-1319

    def evaluate_batch(self, feed_dict=None, on_device=False, tree=False, single_root=True):
        """(LAS, UAS, label accuracy) of one batch from the heads' probabilities
        (``humanize_batch_results_btb``, chem_tensorflow_dense.py:1160-1215):
        runs the forward + heads (no dropout) and scores on the host.
        on_device: the same three floats from the decode's per-graph counts
        (ggnn_heads_decode; only [b, 5] int32 leave the device).  tree (with
        on_device): the heads of every graph that is not a tree are replaced by
        the maximum spanning tree before the counts are read (ggnn_tree_decode,
        as predict_batch(tree=True) returns them); tree="projective": by the
        best projective tree when they are not a projective tree
        (ggnn_projective_decode); tree="projective-mbr": by the minimum Bayes
        risk projective tree, tree="mbr": by the minimum Bayes risk tree over
        all dependency trees (predict_batch).  Any other value of tree raises
        ValueError."""
        if _tree_mode(tree) and not on_device:
            raise ValueError("evaluate_batch: tree=True needs on_device=True")
        if on_device:
            r = self._decode_forward(feed_dict, True, tree, single_root)
            ph, b, v = r["ph"], r["b"], r["v"]
            o, oe = self.params["output_size"], self.output_size_edges

            def fallback(i):
                # an irregular graph: the reference's lists on its fetched probabilities
                row = lambda key, w: np.asarray(ph[key], np.float32).reshape(b, v * w)[i]
                cv = self.ops["computed_values"][i].detach().cpu().numpy()
                cv_e = self.ops["computed_values_edges"][i].detach().cpu().numpy()
                return _eval.graph_scores(row("target_values_head", o), cv, row("node_mask", o),
                                          row("target_values_edges", oe), cv_e, row("node_mask_edges", oe), v, o, oe)

            if r["counts"] is None:          # masks not of get_mask's closed form: the host scorer
                return self._score_batch()[:3]
            return _eval.scores_from_counts(_as_np(r["counts"]), fallback)
        if feed_dict is not None:
            self.feed(feed_dict)
        # the staged placeholders as fed, only the output layer's dropout off
        # (the other keeps are the caller's), never through a captured step
        saved = self.placeholders.get("out_layer_dropout_keep_prob")
        self.placeholders["out_layer_dropout_keep_prob"] = 1.0
        try:
            with torch.no_grad():
                self.build_loss()
        finally:
            if saved is None:
                self.placeholders.pop("out_layer_dropout_keep_prob", None)
            else:
                self.placeholders["out_layer_dropout_keep_prob"] = saved
        return self._score_batch()[:3]

    def _score_batch(self):
        """Host LAS/UAS of the staged batch from the last build_loss() (the
        heads' probabilities are the only device tensors fetched).  Returns
        (las, uas, label_acc, labels, probs, mask, labels_e, probs_e, mask_e)."""
        probs = self.ops["computed_values"].detach().cpu().numpy()
        probs_e = self.ops["computed_values_edges"].detach().cpu().numpy()
        return self._score_arrays(self.placeholders, probs, probs_e)

    def _score_arrays(self, ph, probs, probs_e):
        b = int(ph["num_graphs"])
        v = int(ph["num_vertices"])
        o, oe = self.params["output_size"], self.output_size_edges
        mask = np.asarray(ph["node_mask"], np.float32).reshape(b, v * o)
        mask_e = np.asarray(ph["node_mask_edges"], np.float32).reshape(b, v * oe)
        labels = np.asarray(ph["target_values_head"], np.float32).reshape(b, v * o)
        labels_e = np.asarray(ph["target_values_edges"], np.float32).reshape(b, v * oe)
        las, uas, uas_e = _eval.batch_las_uas(labels, probs, v, mask, labels_e, probs_e, mask_e, o, oe)
        return las, uas, uas_e, labels, probs, mask, labels_e, probs_e, mask_e

    def _epoch(self, data, is_training, step, consume, extra=None, announce=None):
        """One pass over ``data``: what run_epoch and score_epoch share.  The
        epoch's schedule (checked to agree across the ranks), this rank's share
        of it built in a background thread (ThreadedIterator, max_queue_size
        5), and one batch in flight: ``step(feed, all_reduce)`` queues a
        batch's device work and device -> host copies and returns a dict whose
        'event' (or None) follows them; ``consume(batch)`` -> (graphs, loss,
        LAS, UAS, label accuracy) of it runs after the NEXT batch's step, so
        the host's scoring overlaps the GPU instead of alternating with it
        (the reference's sess.run returns every fetch before the host
        continues, chem_tensorflow.py:594).  A rank without a batch in the
        last global step only joins a training step's all-reduce.
        ``extra()``: more sums of the epoch to add over the ranks; ``announce``:
        the epoch name to print progress under.  Returns (graphs, loss, LAS,
        UAS, label accuracy, batches, extra, elapsed): graph-weighted sums over
        all ranks, at least one graph, the slowest rank's seconds."""
        tot = [0, 0.0, 0.0, 0.0, 0.0, 0]

        def finish(p):
            if p["event"] is not None:
                p["event"].synchronize()
            b, batch_loss, las, uas, uas_e = consume(p)
            tot[0] += b
            for i, x in enumerate((batch_loss, las, uas, uas_e), 1):
                tot[i] += x * b
            if announce:
                print("Running %s, batch %i (has %i graphs). Loss so far: %.4f" % (
                    announce, tot[5], b, tot[1] / tot[0]), end="\r")
            tot[5] += 1

        start = time.time()
        pending = None
        world = self.world_size
        all_reduce = _dist.all_reduce_sum(self.group) if world > 1 else None
        if world > 1 and all_reduce is None:
            raise RuntimeError("world_size %d but torch.distributed is not initialised" % world)
        sched = self.minibatch_schedule(data, is_training)
        if world > 1:
            self._check_schedule_agrees(sched)
        it = self.make_minibatch_iterator(data, is_training, rank=self.rank, world_size=world, schedule=sched)
        for feed in ThreadedIterator(it, max_queue_size=5):
            if int(feed["num_graphs"]) == 0:     # no batch for this rank in the last global step
                if is_training:
                    self.train_step(feed, all_reduce=all_reduce)
                continue
            cur = step(feed, all_reduce)
            if pending is not None:
                finish(pending)
            pending = cur
        if pending is not None:
            finish(pending)
        elapsed = time.time() - start
        more = extra() if extra is not None else np.zeros(0)
        if world > 1:
            # one reduction of the epoch's sums over the ranks (off the step loop)
            dev = self.device if torch.distributed.get_backend(self.group) == "nccl" else torch.device("cpu")
            t = torch.tensor(tot + list(more), dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(t, group=self.group)
            mx = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(mx, op=torch.distributed.ReduceOp.MAX, group=self.group)
            t = t.cpu().numpy()
            tot, more, elapsed = [float(x) for x in t[:5]] + [int(t[5])], t[6:], float(mx.item())
        return (max(tot[0], 1), *tot[1:], more, elapsed)

    def _check_schedule_agrees(self, sched) -> None:
        """Data parallel: every rank must draw the same epoch schedule (the
        rank-sharded iterator assumes it; the shuffles use the global numpy
        RNG, seeded by the constructor as chem_tensorflow.py:174-175 does).
        One collective per epoch compares a 62-bit digest of (bucket, sentence
        ids) of every batch across the ranks; a mismatch raises instead of
        silently training some batches twice and others never."""
        import hashlib

        def key(d):
            # the sentence id; without one (a dataset that carries none), the
            # element's own content: words, head locations and edge labels
            i = d.get("id")
            if i is not None:
                return i
            return tuple(tuple(d.get(k) or ()) for k in ("words_index", "words_head", "edges_index"))
        hsh = hashlib.blake2b(digest_size=8)
        for bidx, els in sched:
            hsh.update(repr((bidx, [key(d) for d in els])).encode())
        dg = int.from_bytes(hsh.digest(), "little") >> 2
        dev = self.device if torch.distributed.get_backend(self.group) == "nccl" else torch.device("cpu")
        t = torch.tensor([dg, -dg], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=self.group)
        hi, lo = int(t[0].item()), -int(t[1].item())
        if hi != lo:
            raise RuntimeError("rank %d: the ranks drew different minibatch schedules (digest %d, range [%d, %d]); "
                               "seed np.random identically on every rank (params['random_seed'])"
                               % (self.rank, dg, lo, hi))

    # the reference's per-task "chemical accuracy" normalisers (chem_tensorflow.py:529-531)
    CHEMICAL_ACCURACIES = np.array([0.066513725, 0.012235489, 0.071939046, 0.033730778, 0.033486113, 0.004278493,
                                    0.001330901, 0.004165489, 0.004128926, 0.00409976, 0.004527465, 0.012292586,
                                    0.037467458])

    def run_epoch(self, epoch_name: str, data, is_training: bool, start_step: int = 0, verbose: bool = False):
        """One pass over ``data`` (the output of process_raw_graphs), as
        chem_tensorflow.py:528-667: minibatches built in a background thread
        (ThreadedIterator, max_queue_size 5), a training step (is_training) or a
        dropout-free forward per batch, host LAS/UAS from the heads'
        probabilities.  Returns the reference's tuple (loss, accuracies,
        error_ratios, instance_per_sec, steps, acc_las, acc_uas, all_labels,
        all_computed_values, all_num_vertices, all_masks, all_ids, all_adj_m,
        all_labels_e, all_computed_values_e, all_masks_e, acc_uas_e); for btb the
        task "accuracy" is the task loss (chem_tensorflow.py:411).

        Fetch diet: the reference's sess.run fetches 21 tensors per batch,
        among them the dense [b, 2E, v, v] adjacency, the final node states and
        the whole word-embedding table (:560-593); here only the loss and the
        two heads' probabilities leave the device.

        Data parallel (world_size > 1): each rank runs its share of every
        global step (make_minibatch_iterator(rank, world_size)); a training
        step all-reduces the flat gradient buffer once (train_step).  The loss,
        LAS/UAS sums and graph counts are summed over the ranks once at the
        end of the epoch, and instance_per_sec is all ranks' graphs over the
        slowest rank's epoch time; a training batch's loss is the global
        step's (union-batch) loss.  The per-batch lists (labels, computed
        values, ...) hold this rank's batches only."""
        accuracies = []
        lists = {k: [] for k in ("labels", "cv", "nv", "mask", "ids", "adj", "labels_e", "cv_e", "mask_e")}

        def step(feed, all_reduce):
            if is_training:
                feed["out_layer_dropout_keep_prob"] = self.params["out_layer_dropout_keep_prob"]
                loss = self.train_step(feed, all_reduce=all_reduce)
            else:
                loss = self._eval_forward(feed)
            # the fetch diet: the loss and the two heads' probabilities
            dev = [loss.detach(), self.ops["computed_values"].detach(), self.ops["computed_values_edges"].detach()]
            p = {"feed": feed, "ph": dict(self.placeholders), "event": None}
            if dev[0].device.type != "cuda":
                p["host"] = [t.cpu() for t in dev]
            else:
                p["host"], p["event"] = self._fetch_probs.fetch(dev)
            return p

        def consume(p):
            feed, (hl, hp, hpe) = p["feed"], p["host"]
            b, batch_loss = int(feed["num_graphs"]), float(hl.sum())
            # (copies: the pinned buffers are reused two batches later, and the
            # probabilities stay in the returned lists)
            las, uas, uas_e, labels, cv, mask, labels_e, cv_e, mask_e = self._score_arrays(
                p["ph"], hp.numpy().copy(), hpe.numpy().copy())
            accuracies.append(np.array([batch_loss] * len(self.params["task_ids"])) * b)
            for k, x in (("labels", labels), ("cv", cv), ("nv", int(feed["num_vertices"])), ("mask", mask),
                         ("ids", feed.get("sentences_id")), ("adj", feed.get("adjacency_matrix")),
                         ("labels_e", labels_e), ("cv_e", cv_e), ("mask_e", mask_e)):
                lists[k].append(x)
            return b, batch_loss, las, uas, uas_e

        task_sums = lambda: np.sum(accuracies, axis=0) if accuracies else np.zeros(len(self.params["task_ids"]))
        processed, loss, acc_las, acc_uas, acc_uas_e, steps, acc_sum, elapsed = self._epoch(
            data, is_training, step, consume, task_sums, epoch_name if verbose else None)
        accuracies = acc_sum / processed
        loss = loss / processed
        error_ratios = accuracies / self.CHEMICAL_ACCURACIES[self.params["task_ids"]]
        instance_per_sec = processed / elapsed
        return (loss, accuracies, error_ratios, instance_per_sec, steps, acc_las / processed, acc_uas / processed,
                lists["labels"], lists["cv"], lists["nv"], lists["mask"], lists["ids"], lists["adj"], lists["labels_e"],
                lists["cv_e"], lists["mask_e"], acc_uas_e / processed)
