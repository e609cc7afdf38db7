"""The callers either side of the propagation path, btb task.

* ``EmbeddingFrontEnd`` -- ``get_initial_node_representation``
  (chem_tensorflow_dense.py:264-306): embedding lookups of the ``word_inputs``
  columns, embedding dropout, concat, zero pad to ``hidden_size``.
* ``OutputHeads`` -- ``gated_regression`` for ``--pr btb``
  (chem_tensorflow_dense.py:439-516) with ``MLP(2h, o, [], keep)``
  (utils.py:40-84) and the btb cross-entropy (chem_tensorflow.py:349-403);
  not in the reference: ``tree_loss=`` turns head 0's loss into the negative
  log-likelihood of the gold tree (``ggnn_tree_loss``, ``csrc/k_tree_loss.h``)
  or, with a cost, into the structured hinge over cost-augmented decoding
  (``ggnn_margin_loss``, ``csrc/k_margin_loss.h``).

Both run in libggnn.so (``ggnn_embed_*``, ``ggnn_heads_*``; kernels in
``csrc/k_head.h``); torch tensors only hold device memory.  The autograd
Functions ``EmbedFunction`` / ``HeadsFunction`` let the drop-in model train with
``loss.backward()``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .upload import Uploader

from . import _lib
from .evaluation import TREE_LOG2_FLOOR, _count_in_range
from .evaluation import tree_score_shift  # noqa: F401  (tree_score_shift: re-exported)

SMALL_NUMBER = 1e-7   # utils.py


class EmbedSegment(ctypes.Structure):          # include/ggnn.h: ggnn_embed_segment
    _fields_ = [("table", ctypes.c_void_p), ("d_table", ctypes.c_void_p), ("rows", ctypes.c_int64),
                ("width", ctypes.c_int32), ("column", ctypes.c_int32)]


class OutputHead(ctypes.Structure):            # include/ggnn.h: ggnn_output_head
    _fields_ = [("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("o", ctypes.c_int32),
                ("labels", ctypes.c_void_p), ("probs", ctypes.c_void_p), ("d_weight", ctypes.c_void_p),
                ("d_bias", ctypes.c_void_p)]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, device):
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float32)))
    return t.to(device=device, dtype=torch.float32).contiguous()


_WI_UPLOAD = Uploader()


def word_inputs_tensor(word_inputs, device, table_rows=None) -> torch.Tensor:
    """The feed's ``word_inputs`` [b, v, ncols] (float64 in the reference's feed)
    as int32 on the device.  ``table_rows``: {column: rows} to validate (the
    reference's CPU ``embedding_lookup`` raises for an index out of range)."""
    wi = np.asarray(word_inputs)
    wi_i = wi.astype(np.int64)
    if table_rows:
        for col, rows in table_rows.items():
            c = wi_i[..., col]
            if c.size and (c.min() < 0 or c.max() >= rows):
                raise IndexError("word_inputs[..., %d] holds index %d outside [0, %d)"
                                 % (col, int(c.max() if c.max() >= rows else c.min()), rows))
    return _WI_UPLOAD(wi_i.astype(np.int32), device)


class EmbeddingFrontEnd:
    """segments: list of (table tensor [rows, width], word_inputs column), in
    concat order.  btb: [(loc_embeddings, 0), (pos_embeddings, 1),
    (word_embeddings, 2), (loc_embeddings, 3)] (:268-299)."""

    def __init__(self, hidden: int, deterministic: bool = True):
        """deterministic: the table gradients through ggnn_embed_backward_ws
        (fixed-point accumulation: the same bits run to run); False: the fp32
        atomics of ggnn_embed_backward."""
        self.hidden = int(hidden)
        self._lib = _lib.load()
        self.deterministic = bool(deterministic) and hasattr(self._lib, "ggnn_embed_backward_ws")
        self._ws = {}    # table set -> zero-filled workspace (each call leaves it zero-filled)

    def workspace(self, segments, device):
        """The deterministic backward's workspace for this table set: allocated
        (zero-filled) once and kept, so a captured step's pointer stays valid."""
        key = tuple((t.data_ptr(), tuple(t.shape)) for t, _ in segments)
        ws = self._ws.get(key)
        if ws is None:
            n = ctypes.c_size_t(0)
            _lib.check(self._lib.ggnn_embed_workspace_bytes(self._segs(segments), len(segments), ctypes.byref(n)),
                       "ggnn_embed_workspace_bytes")
            ws = torch.zeros(max(int(n.value), 1), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def _segs(self, segments, dtables=None):
        arr = (EmbedSegment * len(segments))()
        for i, (t, col) in enumerate(segments):
            dt = None if dtables is None or dtables[i] is None else dtables[i].data_ptr()
            arr[i] = EmbedSegment(t.data_ptr(), dt, t.shape[0], t.shape[1], int(col))
        return arr

    def lookup_rows(self, segments, seg, wi, dh0, keep, seed, rows, ids, dh0_add=None, seed_device=False):
        """Segment ``seg``'s gradient as IndexedSlices: rows [cap, width] (the
        per-lookup gradient rows, embedding dropout applied) and ids [cap]
        (int32, -1 past the batch) -- ggnn_embed_lookup_rows."""
        b, v, ncols = wi.shape
        d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32", seed_device=seed_device)
        _lib.check(self._lib.ggnn_embed_lookup_rows(ctypes.byref(d), self._segs(segments), len(segments), int(seg),
                                                    _ptr(wi), ncols, float(keep), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                    _ptr(dh0.contiguous()),
                                                    _ptr(None if dh0_add is None else dh0_add.contiguous()),
                                                    _ptr(rows), _ptr(ids), int(rows.shape[0]), _stream()),
                   "ggnn_embed_lookup_rows")

    def union_backward(self, table, dtable, rows, ids, sq_out):
        """The gradient of ``table`` from IndexedSlices (rows [n, width], ids
        [n]; -1 = none): dtable = the sum of the rows per id in 64-bit fixed
        point (exact, whatever order -- the same bits on every rank that holds
        the same slices), sq_out[0] = the sum of the squared rows
        (ggnn_embed_backward_ws over one segment, keep 1)."""
        n, w = rows.shape
        segs = [(table, 0)]
        d = _lib.dims(int(n), 1, int(w), 1, 1, True, "fp32")
        _lib.check(self._lib.ggnn_embed_backward_ws(ctypes.byref(d), self._segs(segs, [dtable]), 1,
                                                    _ptr(ids.contiguous()), 1, 1.0, 0, _ptr(rows.contiguous()),
                                                    None, _ptr(sq_out), _ptr(self.workspace(segs, rows.device)),
                                                    _stream()), "ggnn_embed_backward_ws")

    def forward(self, segments, wi: torch.Tensor, keep: float = 1.0, seed: int = 0, seed_device: bool = False,
                out=None) -> torch.Tensor:
        """seed_device: seed is the address of a device uint64 (GGNN_SEED_DEVICE)."""
        b, v, ncols = wi.shape
        h0 = out if out is not None else torch.empty(b, v, self.hidden, dtype=torch.float32, device=wi.device)
        d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32", seed_device=seed_device)
        _lib.check(self._lib.ggnn_embed_forward(ctypes.byref(d), self._segs(segments), len(segments), _ptr(wi), ncols,
                                                float(keep), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(h0), _stream()),
                   "ggnn_embed_forward")
        return h0

    def backward(self, segments, wi, dh0, keep=1.0, seed=0, dh0_add=None, dtables=None, sq_out=None,
                 seed_device=False):
        """Returns (per-segment dense table gradients, lookup sqnorm device
        vector [nseg]).  dtables: optional per-segment gradient buffers;
        segments that share a table may share one buffer (the kernel adds both
        segments' lookups into it, and the table's squared lookup norm goes to
        the first such segment's slot).  sq_out: optional [nseg] fp32 output
        (e.g. a view into a flat all-reduce buffer)."""
        b, v, ncols = wi.shape
        dts = dtables if dtables is not None else [torch.empty_like(t) for t, _ in segments]
        sq = sq_out if sq_out is not None else torch.empty(len(segments), dtype=torch.float32, device=wi.device)
        d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32", seed_device=seed_device)
        args = (ctypes.byref(d), self._segs(segments, dts), len(segments), _ptr(wi), ncols, float(keep),
                int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(dh0.contiguous()),
                _ptr(None if dh0_add is None else dh0_add.contiguous()), _ptr(sq))
        if self.deterministic:
            _lib.check(self._lib.ggnn_embed_backward_ws(*args, _ptr(self.workspace(segments, wi.device)), _stream()),
                       "ggnn_embed_backward_ws")
        else:
            _lib.check(self._lib.ggnn_embed_backward(*args, _stream()), "ggnn_embed_backward")
        return dts, sq


class OutputHeads:
    """heads: list of (W [2h, o], b [o]) tensors; labels per head [b, v, o]."""

    def __init__(self, hidden: int):
        self.hidden = int(hidden)
        self._lib = _lib.load()
        self._ws = None
        # pass name -> the binding's own workspace for ggnn_<name> (_pass): only
        # for graphs above the pass's *_LDS_MAXN nodes (tree_decode asks for none
        # today; tree_loss always: n_eff, then the family's marginals workspace)
        self._pass_ws = {}
        self._saved = None
        # the last forward's structured loss (tree_loss=): the marginals that
        # stand in head 0's probs place in the backward, and used int32 [b];
        # None after a forward without it
        self.tree_marg = self.tree_used = None
        # the last forward's max-margin loss (tree_loss= with a cost): T* int32
        # [b, v], max(0, l) float32 [b] and the Hamming distance int32 [b]; None
        # after a forward without it
        self.margin_heads = self.margin_value = self.margin_hamming = None

    def _table(self, heads, labels, probs, dws=None, dbs=None):
        arr = (OutputHead * len(heads))()
        for i, (W, bias) in enumerate(heads):
            arr[i] = OutputHead(W.data_ptr(), bias.data_ptr(), W.shape[1],
                                None if labels is None or labels[i] is None else labels[i].data_ptr(),
                                probs[i].data_ptr(), None if dws is None else dws[i].data_ptr(),
                                None if dbs is None else dbs[i].data_ptr())
        return arr

    def forward(self, hT, h0, heads, labels=None, keep=1.0, seed=0, target_num=1.0, loss_out=None, probs_out=None,
                seed_device=False, tree_loss=None):
        """Returns (probs list [b, v, o], loss tensor [nheads] or None).
        loss_out / probs_out: optional output buffers (loss [nheads] fp32).
        target_num: a number, or a device fp32 tensor of one element
        (ggnn_heads_forward_dev); seed_device: seed is the address of a
        device uint64 (GGNN_SEED_DEVICE).  tree_loss: None, or (family,
        single_root, n_nodes int32 [b] on the device): head 0's loss becomes
        the tree-structured one (``tree_loss`` below, after the heads' forward
        on the same stream: ln Z / target_num is added into loss[0]); the
        marginals and used [b] stay on the object (tree_marg, tree_used) and
        the next ``backward`` takes the marginals in head 0's probs place.
        With a fourth element, the margin cost, the max-margin loss runs in
        its place (``margin_loss`` below): tree_marg then holds onehot(T*), the
        gold block or the probabilities, and margin_heads, margin_value and
        margin_hamming stay on the object as well.
        The returned probs are the softmax either way."""
        if tree_loss is not None and labels is None:
            raise ValueError("tree_loss needs labels")
        b, v, h = hT.shape
        dev = hT.device
        probs = probs_out if probs_out is not None else [torch.empty(b, v, W.shape[1], dtype=torch.float32, device=dev)
                                                          for W, _ in heads]
        d = _lib.dims(b, v, h, 1, 1, True, "fp32", seed_device=seed_device)
        tab = self._table(heads, labels, probs)
        n = ctypes.c_size_t(0)
        _lib.check(self._lib.ggnn_heads_workspace_bytes(ctypes.byref(d), tab, len(heads), ctypes.byref(n)),
                   "ggnn_heads_workspace_bytes")
        if self._ws is None or self._ws.numel() < n.value:
            self._ws = torch.empty(max(int(n.value), 1), dtype=torch.uint8, device=dev)
        loss = None
        if labels is not None:
            loss = loss_out if loss_out is not None else torch.empty(len(heads), dtype=torch.float32, device=dev)
        if isinstance(target_num, torch.Tensor):
            _lib.check(self._lib.ggnn_heads_forward_dev(ctypes.byref(d), tab, len(heads), _ptr(hT.contiguous()),
                                                        _ptr(h0.contiguous()), float(keep),
                                                        int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(target_num), _ptr(loss),
                                                        _ptr(self._ws), _stream()),
                       "ggnn_heads_forward_dev")
        else:
            _lib.check(self._lib.ggnn_heads_forward(ctypes.byref(d), tab, len(heads), _ptr(hT.contiguous()),
                                                    _ptr(h0.contiguous()), float(keep), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                    float(target_num), _ptr(loss), _ptr(self._ws), _stream()),
                       "ggnn_heads_forward")
        self._saved = (b, v, h)
        self.tree_marg = self.tree_used = None
        self.margin_heads = self.margin_value = self.margin_hamming = None
        if tree_loss is not None and len(tree_loss) == 4:
            family, single_root, n_nodes, cost = tree_loss
            out = self.margin_loss(probs[0], labels[0], n_nodes, family, single_root, target_num, loss, cost)
            self.tree_marg, self.margin_heads, self.margin_value, self.margin_hamming, _, self.tree_used = out
        elif tree_loss is not None:
            family, single_root, n_nodes = tree_loss
            self.tree_marg, _, _, self.tree_used = self.tree_loss(probs[0], labels[0], n_nodes, family, single_root,
                                                                  target_num, loss)
        return probs, loss

    def tree_loss(self, probs_head, gold_head, n_nodes, family, single_root, target_num, loss, workspace=None):
        """The tree-structured loss term on the current stream (ggnn_tree_loss,
        include/ggnn.h): ``loss[0] += (sum over the used graphs of ln Z) /
        target_num``.  probs_head, gold_head: float32 [b, v, o]; n_nodes: int32
        [b]; family: 0 / "nonprojective" (all dependency trees) or 1 /
        "projective"; target_num: a number or a device fp32 tensor of one
        element; loss: a device fp32 tensor, element 0 added to.  Returns
        (marg float32 [b, v, o], logz float32 [b], status int32 [b], used
        int32 [b]): a used graph's marg holds the arc marginals (what the
        heads' backward takes in the probabilities' place), any other graph's
        a copy of probs_head.  workspace: a uint8 tensor to use instead of the
        binding's own."""
        family = {"nonprojective": 0, "projective": 1}.get(family, family)
        if family not in (0, 1):
            raise ValueError("family must be 0 / 'nonprojective' or 1 / 'projective'")
        b, v, o, dev, run = self._pass("tree_loss", probs_head, "probs_head", torch.float32, n_nodes, workspace, family)
        _check_tensor(gold_head, "gold_head", torch.float32)
        if gold_head.shape != probs_head.shape or gold_head.device != dev:
            raise ValueError("gold_head must have probs_head's shape and device")
        if loss.dtype != torch.float32 or loss.device != dev or loss.numel() < 1 or not loss.is_contiguous():
            raise ValueError("loss must be a contiguous float32 tensor on %s" % dev)
        marg = torch.empty_like(probs_head)
        logz = torch.empty(b, dtype=torch.float32, device=dev)
        status = torch.empty(b, dtype=torch.int32, device=dev)
        used = torch.empty(b, dtype=torch.int32, device=dev)
        on_dev = isinstance(target_num, torch.Tensor)
        run(_ptr(gold_head), _ptr(n_nodes), int(family), int(bool(single_root)),
            _ptr(target_num) if on_dev else float(target_num), _ptr(marg), _ptr(logz), _ptr(status), _ptr(used),
            _ptr(loss), entry="tree_loss_dev" if on_dev else "tree_loss")
        return marg, logz, status, used

    def margin_loss(self, probs_head, gold_head, n_nodes, family, single_root, target_num, loss, cost=1.0,
                    workspace=None):
        """The max-margin loss on the current stream (ggnn_margin_loss,
        include/ggnn.h): the structured hinge over cost-augmented decoding.
        Arguments and checks are ``tree_loss``'s; cost: the margin per wrong
        head, 0..64.  ``loss[0] += (sum over the used graphs of max(0, l) +
        sum_d ln p[d][y_d]) / target_num``: the hinge in the place of the
        cross-entropy the heads' forward has put there.  Returns (marg float32
        [b, v, o], heads int32 [b, v], value float32 [b], hamming int32 [b],
        status int32 [b], used int32 [b]): a used graph's marg holds
        onehot(T*) where its loss is positive and its gold block otherwise
        (what the heads' backward takes in the probabilities' place), any
        other graph's a copy of probs_head; heads is T* (-1 on node 0, the
        padding and the graphs that are not used)."""
        family = {"nonprojective": 0, "projective": 1}.get(family, family)
        if family not in (0, 1):
            raise ValueError("family must be 0 / 'nonprojective' or 1 / 'projective'")
        if isinstance(cost, (bool, str)) or cost is None or not 0.0 <= float(cost) <= 64.0:
            raise ValueError("cost must be a number in 0..64, got %r" % (cost,))
        _check_tensor(probs_head, "probs_head", torch.float32)
        b, v, o, dev, run = self._pass("margin_loss", probs_head, "probs_head", torch.float32, n_nodes, workspace,
                                       probs_head.shape[2], family)
        _check_tensor(gold_head, "gold_head", torch.float32)
        if gold_head.shape != probs_head.shape or gold_head.device != dev:
            raise ValueError("gold_head must have probs_head's shape and device")
        if loss.dtype != torch.float32 or loss.device != dev or loss.numel() < 1 or not loss.is_contiguous():
            raise ValueError("loss must be a contiguous float32 tensor on %s" % dev)
        marg = torch.empty_like(probs_head)
        heads = torch.empty(b, v, dtype=torch.int32, device=dev)
        value = torch.empty(b, dtype=torch.float32, device=dev)
        hamming, status, used = (torch.empty(b, dtype=torch.int32, device=dev) for _ in range(3))
        on_dev = isinstance(target_num, torch.Tensor)
        run(_ptr(gold_head), _ptr(n_nodes), int(family), int(bool(single_root)), float(cost),
            _ptr(target_num) if on_dev else float(target_num), _ptr(marg), _ptr(heads), _ptr(value), _ptr(hamming),
            _ptr(status), _ptr(used), _ptr(loss), entry="margin_loss_dev" if on_dev else "margin_loss")
        return marg, heads, value, hamming, status, used

    def backward(self, hT, h0, heads, labels, probs, target_num=1.0, d_loss=None, dws=None, dbs=None, dhT=None,
                 dh0=None):
        """Gradients of sum(loss) (times d_loss, a device scalar): dW, db per
        head and (dhT, dh0).  Uses the workspace of the last forward.  dws, dbs,
        dhT, dh0: optional output buffers (overwritten).  After a forward with
        tree_loss the marginals it kept stand in probs[0]'s place (dZ = marg -
        y on the used graphs); the caller's probs are not written."""
        b, v, h = hT.shape
        if self._saved != (b, v, h):
            raise RuntimeError("heads backward without a matching forward")
        if self.tree_marg is not None:
            probs = [self.tree_marg] + list(probs[1:])
        dws = dws if dws is not None else [torch.empty_like(W) for W, _ in heads]
        dbs = dbs if dbs is not None else [torch.empty_like(bb) for _, bb in heads]
        dhT = dhT if dhT is not None else torch.empty_like(hT)
        dh0 = dh0 if dh0 is not None else torch.empty_like(h0)
        d = _lib.dims(b, v, h, 1, 1, True, "fp32")
        tab = self._table(heads, labels, probs, dws, dbs)
        if isinstance(target_num, torch.Tensor):     # device target_num (ggnn_heads_backward_dev)
            _lib.check(self._lib.ggnn_heads_backward_dev(ctypes.byref(d), tab, len(heads), _ptr(hT.contiguous()),
                                                         _ptr(h0.contiguous()), _ptr(target_num), _ptr(d_loss),
                                                         _ptr(self._ws), _ptr(dhT), _ptr(dh0), _stream()),
                       "ggnn_heads_backward_dev")
        else:
            _lib.check(self._lib.ggnn_heads_backward(ctypes.byref(d), tab, len(heads), _ptr(hT.contiguous()),
                                                     _ptr(h0.contiguous()), float(target_num), _ptr(d_loss),
                                                     _ptr(self._ws), _ptr(dhT), _ptr(dh0), _stream()),
                       "ggnn_heads_backward")
        return dws, dbs, dhT, dh0

    def decode(self, probs, n_nodes, labels=None):
        """The predicted tree and the LAS / UAS counts of a batch on the device
        (ggnn_heads_decode).  probs: [head probabilities [b, v, o], label
        probabilities [b, v, oe]]; n_nodes: int32 [b] on the device; labels:
        the two heads' 0/1 targets (same shapes) or None.  Returns (pred
        [b, v, 2], gold [b, v, 2] or None, counts [b, 5]) as int32 device
        tensors: zero-based (head, label) columns, -1 = skipped; counts =
        (n_kept, las, uas, lab, regular) per graph."""
        p_h, p_l = (_decode_input(t, "probs") for t in probs)
        b, v, o = p_h.shape
        oe = p_l.shape[2]
        if p_l.shape[:2] != (b, v):
            raise ValueError("probs: head %s and label %s shapes disagree" % (tuple(p_h.shape), tuple(p_l.shape)))
        dev = p_h.device
        _check_n_nodes(n_nodes, b, dev)
        y_h = y_l = gold = None
        if labels is not None:
            y_h, y_l = (_decode_input(t, "labels") for t in labels)
            if y_h.shape != p_h.shape or y_l.shape != p_l.shape:
                raise ValueError("labels must have the probabilities' shapes")
            gold = torch.empty(b, v, 2, dtype=torch.int32, device=dev)
        pred = torch.empty(b, v, 2, dtype=torch.int32, device=dev)
        counts = torch.empty(b, _lib.DECODE_COUNTS, dtype=torch.int32, device=dev)
        d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32")
        _lib.check(self._lib.ggnn_heads_decode(ctypes.byref(d), _ptr(p_h), o, _ptr(p_l), oe, _ptr(y_h), _ptr(y_l),
                                               _ptr(n_nodes), _ptr(pred), _ptr(gold), _ptr(counts), _stream()),
                   "ggnn_heads_decode")
        return pred, gold, counts

    def _workspace(self, name, need, dev, workspace=None):
        """Pass ``name``'s workspace of ``need`` bytes: the binding's own
        buffer, grown on demand (None when the pass asks for none), or the
        caller's once it is checked."""
        if workspace is None:
            own = self._pass_ws.get(name)
            if need and (own is None or own.numel() < need or own.device != dev):
                own = self._pass_ws[name] = torch.empty(need, dtype=torch.uint8, device=dev)
            return own if need else None
        if workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
            raise ValueError("workspace must be a contiguous uint8 tensor on %s" % dev)
        if workspace.numel() < need:
            raise ValueError("workspace of %d bytes, %d needed" % (workspace.numel(), need))
        return workspace

    def _pass(self, name, x, x_name, dtype, n_nodes, workspace, *size_args):
        """What the passes with a workspace share, either side of a pass's own
        part.  Before it: the checks of the input ``x`` (``dtype`` [b, v, o]
        on the GPU, ``x_name`` in the messages), of the shape rule and of
        n_nodes.  Returns (b, v, o, device, run).  After it: ``run(*middle)``
        sizes the workspace (ggnn_<name>_workspace_bytes(b, v, *size_args);
        the binding's own buffer or the caller's ``workspace``) and calls
        ggnn_<name>(dims, x, o, *middle, workspace, its bytes, stream);
        ``entry``: another entry point with that signature and size."""
        _check_tensor(x, x_name, dtype)
        b, v, o = x.shape
        dev = x.device
        if v > o or v > _lib.TREE_MAXV:
            raise ValueError("%s needs v <= o and v <= %d (got v %d, o %d)" % (name, _lib.TREE_MAXV, v, o))
        _check_n_nodes(n_nodes, b, dev)

        def run(*middle, entry=name):
            need = int(getattr(self._lib, "ggnn_%s_workspace_bytes" % name)(b, v, *size_args))
            ws = self._workspace(name, need, dev, workspace)
            d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32")
            _lib.check(getattr(self._lib, "ggnn_" + entry)(ctypes.byref(d), _ptr(x), o, *middle, _ptr(ws),
                                                           0 if ws is None else ws.numel(), _stream()), "ggnn_" + entry)
        return b, v, o, dev, run

    def _tree_pass(self, name, scores, n_nodes, pred, gold, counts, single_root, workspace=None):
        """tree_decode / projective_decode: ggnn_<name> with its workspace."""
        b, v, o, dev, run = self._pass(name, scores, "scores", torch.int32, n_nodes, workspace)
        if (gold is None) != (counts is None):
            raise ValueError("gold and counts are given together")
        _check_int32(pred, "pred", (b, v, 2), dev)
        if gold is not None:
            _check_int32(gold, "gold", (b, v, 2), dev)
            _check_int32(counts, "counts", (b, _lib.DECODE_COUNTS), dev)
        status = torch.empty(b, dtype=torch.int32, device=dev)
        run(_ptr(n_nodes), int(bool(single_root)), _ptr(pred), _ptr(gold), _ptr(counts), _ptr(status))
        return status

    def tree_decode(self, scores, n_nodes, pred, gold=None, counts=None, single_root=True):
        """The tree post-pass on ``decode``'s pred, on the same stream
        (ggnn_tree_decode).  scores: int32 [b, v, o] (``tree_scores``);
        n_nodes: int32 [b]; pred: int32 [b, v, 2], updated in place; gold
        [b, v, 2] and counts [b, 5] (decode's) together or both None: a
        repaired graph's las / uas counts are recounted in place.  Returns
        status int32 [b]: 0 = pred's heads already were a tree, 1 = replaced
        by the maximum spanning tree of the scores, 2 = no tree exists (the
        graph is left as it was)."""
        return self._tree_pass("tree_decode", scores, n_nodes, pred, gold, counts, single_root)

    def projective_decode(self, scores, n_nodes, pred, gold=None, counts=None, single_root=True, workspace=None):
        """The projective post-pass on ``decode``'s pred, on the same stream
        (ggnn_projective_decode): tree_decode's arguments and checks.  Returns
        status int32 [b]: 0 = pred's heads already were a projective tree, 1 =
        replaced by the best projective tree of the scores (Eisner), 2 = no
        projective tree exists or the scores are out of range (the graph is
        left as it was).  workspace: a uint8 tensor to use instead of the
        binding's own (grown on demand; needed for v > PROJ_LDS_MAXN only)."""
        return self._tree_pass("projective_decode", scores, n_nodes, pred, gold, counts, single_root, workspace)

    def _marginals_pass(self, name, p, n_nodes, single_root, with_scores, workspace):
        """projective_marginals / tree_marginals: ggnn_<name> with its outputs
        and its workspace."""
        b, v, o, dev, run = self._pass(name, p, "probs_head", torch.float32, n_nodes, workspace)
        marg = torch.empty_like(p)
        logz = torch.empty(b, dtype=torch.float32, device=dev)
        scores = torch.empty(b, v, o, dtype=torch.int32, device=dev) if with_scores else None
        status = torch.empty(b, dtype=torch.int32, device=dev)
        run(_ptr(n_nodes), int(bool(single_root)), _ptr(marg), _ptr(logz), _ptr(scores), _ptr(status))
        return marg, logz, scores, status

    def projective_marginals(self, probs_head, n_nodes, single_root=True, with_scores=True, workspace=None):
        """The posterior marginal of every arc under the distribution over
        projective trees that the head probabilities define, on the current
        stream (ggnn_projective_marginals).  probs_head: float32 [b, v, o];
        n_nodes: int32 [b].  Returns (marg float32 [b, v, o], logz float32
        [b], scores int32 [b, v, o] = rint(marg * 2^20) / GGNN_TREE_FORBIDDEN
        (None without with_scores), status int32 [b]: 1 = written, 0 = n < 2,
        2 = no projective tree; for status != 1 marg is a copy of probs_head
        and scores are all forbidden).  workspace: a uint8 tensor to use
        instead of the binding's own (grown on demand; needed for v >
        MARG_LDS_MAXN only)."""
        return self._marginals_pass("projective_marginals", probs_head, n_nodes, single_root, with_scores, workspace)

    def tree_marginals(self, probs_head, n_nodes, single_root=True, with_scores=True, workspace=None):
        """The posterior marginal of every arc under the distribution over ALL
        dependency trees (crossing arcs included) that the head probabilities
        define, on the current stream (ggnn_tree_marginals: the matrix-tree
        theorem).  Arguments, checks and the returned (marg, logz, scores or
        None, status) are projective_marginals'; status 2 = no dependency
        tree exists; ``tree_decode`` on the scores gives the minimum Bayes
        risk tree.  workspace: a uint8 tensor to use instead of the binding's
        own (grown on demand; needed for v > LAPL_LDS_MAXN only)."""
        return self._marginals_pass("tree_marginals", probs_head, n_nodes, single_root, with_scores, workspace)

    def tree_sample(self, probs_head, n_nodes, num_samples, seed=0, single_root=True, marginals=None, workspace=None):
        """num_samples dependency trees per graph drawn from the distribution
        over ALL dependency trees that the head probabilities define, on the
        current stream (ggnn_tree_sample: conditional sampling on the
        matrix-tree inverse).  probs_head: float32 [b, v, o]; n_nodes: int32
        [b]; seed: a 64-bit integer (sample s of graph g depends on seed, g and
        s alone).  marginals: what ``tree_marginals`` returned for the same
        probs_head, n_nodes and single_root (run here when None).  Returns
        (heads int32 [b, K, v]: the head of word i, -1 on row 0, the rows >= n
        and where status != 1; log_prob float32 [b, K]: ln of the tree's
        probability, -inf where status != 1; status int32 [b, K]: 1 = drawn, 0
        = n < 2, 2 = no tree exists or a numerical dead end).  workspace: a
        uint8 tensor to use instead of the binding's own (grown on demand;
        needed for v > SAMPLE_LDS_MAXN only)."""
        p, K = probs_head, _count_in_range("num_samples", num_samples, _lib.SAMPLE_MAX)
        b, v, o, dev, run = self._pass("tree_sample", p, "probs_head", torch.float32, n_nodes, workspace, K)
        if marginals is None:
            marginals = self.tree_marginals(p, n_nodes, single_root, with_scores=False)
        marg, logz, _, m_status = marginals
        if (marg.shape != p.shape or marg.dtype != torch.float32 or marg.device != dev or not marg.is_contiguous()
                or logz.dtype != torch.float32 or logz.device != dev or logz.numel() != b or not logz.is_contiguous()):
            raise ValueError("marginals must be tree_marginals' outputs for probs_head")
        _check_int32(m_status, "marginals' status", (b,), dev)
        heads = torch.empty(b, K, v, dtype=torch.int32, device=dev)
        log_prob = torch.empty(b, K, dtype=torch.float32, device=dev)
        status = torch.empty(b, K, dtype=torch.int32, device=dev)
        run(_ptr(n_nodes), int(bool(single_root)), _ptr(marg), _ptr(logz), _ptr(m_status), K,
            int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(heads), _ptr(log_prob), _ptr(status))
        return heads, log_prob, status

    def projective_sample(self, probs_head, n_nodes, num_samples, seed=0, single_root=True, workspace=None):
        """num_samples projective dependency trees per graph drawn from the
        distribution over projective trees that the head probabilities define
        (``projective_marginals``' distribution), on the current stream
        (ggnn_projective_sample: one inside pass per graph, a top-down walk
        over its tables per sample; no marginals are needed).  probs_head:
        float32 [b, v, o]; n_nodes: int32 [b]; seed: a 64-bit integer (sample s
        of graph g depends on seed, g and s alone).  Returns (heads int32
        [b, K, v]: the head of word i, -1 on row 0, the rows >= n and where
        status != 1; log_prob float32 [b, K]: ln of the tree's probability,
        -inf where status != 1; status int32 [b, K]: 1 = drawn, 0 = n < 2, 2 =
        no projective tree exists or a numerical dead end; logz float32 [b]:
        ``projective_marginals``' ln Z).  workspace: a uint8 tensor to use
        instead of the binding's own (grown on demand; needed for v >
        PROJ_SAMPLE_LDS_MAXN only)."""
        K = _count_in_range("num_samples", num_samples, _lib.SAMPLE_MAX)
        b, v, o, dev, run = self._pass("projective_sample", probs_head, "probs_head", torch.float32, n_nodes,
                                       workspace, K)
        heads = torch.empty(b, K, v, dtype=torch.int32, device=dev)
        log_prob = torch.empty(b, K, dtype=torch.float32, device=dev)
        status = torch.empty(b, K, dtype=torch.int32, device=dev)
        logz = torch.empty(b, dtype=torch.float32, device=dev)
        run(_ptr(n_nodes), int(bool(single_root)), K, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(heads), _ptr(log_prob),
            _ptr(status), _ptr(logz))
        return heads, log_prob, status, logz

    def projective_kbest(self, scores, n_nodes, K, single_root=True, workspace=None):
        """The K best projective dependency trees of every graph, best first,
        on the current stream (ggnn_projective_kbest: Eisner's tables with a
        sorted list of up to K entries per item; rank 0 is
        ``projective_decode``'s tree).  scores: int32 [b, v, o]
        (``tree_scores``); n_nodes: int32 [b]; 1 <= K <= KBEST_MAX.  Returns
        (heads int32 [b, K, v]: the head of word i in the tree of rank k, -1 on
        node 0, the rows >= n and the ranks >= count; totals int32 [b, K]: the
        tree's sum of scores, TREE_FORBIDDEN on the ranks >= count; count int32
        [b]: the trees returned, min(K, number of projective trees); status
        int32 [b]: 1 = count >= 1, 0 = n < 2, 2 = no projective tree exists or
        the scores are out of range).  workspace: a uint8 tensor to use instead
        of the binding's own (grown on demand; needed for v >
        ggnn_projective_kbest_lds_maxn(K) only)."""
        return self._kbest_pass("projective_kbest", scores, n_nodes, K, single_root, workspace)

    def tree_kbest(self, scores, n_nodes, K, single_root=True, workspace=None):
        """The K best trees over ALL dependency trees (arcs may cross) of every
        graph, best first, on the current stream (ggnn_tree_kbest: Lawler's
        partitioning over ``tree_decode``'s solver, 2 K - 1 launches; rank 0 is
        ``tree_decode``'s tree).  Arguments, checks and the returned (heads,
        totals, count, status) are ``projective_kbest``'s; count =
        min(K, number of trees), status 2 = no tree exists or the scores are
        out of range.  workspace: a uint8 tensor to use instead of the
        binding's own (grown on demand, kept per pass:
        ggnn_tree_kbest_workspace_bytes(b, v, K) bytes)."""
        return self._kbest_pass("tree_kbest", scores, n_nodes, K, single_root, workspace)

    def _kbest_pass(self, name, scores, n_nodes, K, single_root, workspace):
        """projective_kbest / tree_kbest: ggnn_<name> with its outputs and its
        workspace."""
        K = _count_in_range("K", K, _lib.KBEST_MAX)
        b, v, o, dev, run = self._pass(name, scores, "scores", torch.int32, n_nodes, workspace, K)
        heads = torch.empty(b, K, v, dtype=torch.int32, device=dev)
        totals = torch.empty(b, K, dtype=torch.int32, device=dev)
        count = torch.empty(b, dtype=torch.int32, device=dev)
        status = torch.empty(b, dtype=torch.int32, device=dev)
        run(_ptr(n_nodes), int(bool(single_root)), K, _ptr(heads), _ptr(totals), _ptr(count), _ptr(status))
        return heads, totals, count, status

    def arc_confidence(self, marg, n_nodes, pred):
        """conf float32 [b, v]: marg[g, i, pred[g, i, 0]], 0 where there is no
        predicted head or the row is 0 or >= n (ggnn_arc_confidence).  marg:
        float32 [b, v, o]; n_nodes: int32 [b]; pred: int32 [b, v, 2]."""
        if marg.dim() != 3 or marg.dtype != torch.float32 or marg.device.type != "cuda" or not marg.is_contiguous():
            raise ValueError("marg must be a contiguous float32 [b, v, o] tensor on the GPU")
        b, v, o = marg.shape
        dev = marg.device
        if v > o:
            raise ValueError("arc_confidence needs v <= o (got v %d, o %d)" % (v, o))
        _check_n_nodes(n_nodes, b, dev)
        _check_int32(pred, "pred", (b, v, 2), dev)
        conf = torch.empty(b, v, dtype=torch.float32, device=dev)
        d = _lib.dims(b, v, self.hidden, 1, 1, True, "fp32")
        _lib.check(self._lib.ggnn_arc_confidence(ctypes.byref(d), _ptr(marg), o, _ptr(n_nodes), _ptr(pred),
                                                 _ptr(conf), _stream()), "ggnn_arc_confidence")
        return conf


def _check_n_nodes(n_nodes, b, dev):
    if n_nodes.dtype != torch.int32 or n_nodes.device != dev or n_nodes.numel() != b or not n_nodes.is_contiguous():
        raise ValueError("n_nodes must be a contiguous int32 tensor of %d elements on %s" % (b, dev))


def _check_tensor(t, name, dtype):
    """t: an int32 / float32 [b, v, o] tensor on the GPU, contiguous."""
    kind = "an int32" if dtype == torch.int32 else "a float32"
    if t.dim() != 3 or t.dtype != dtype or t.device.type != "cuda":
        raise ValueError("%s must be %s [b, v, o] tensor on the GPU" % (name, kind))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _check_int32(t, name, shape, dev):
    if t.dtype != torch.int32 or t.device != dev or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError("%s must be a contiguous int32 %s tensor on %s" % (name, list(shape), dev))


def tree_scores(probs_head, n_nodes, v):
    """Integer arc scores for ``OutputHeads.tree_decode`` on the tensor's
    device (plain torch, evaluation.tree_scores is the numpy form):
    probs_head float32 [b, v, o], n_nodes [b] -> int32 [b, v, o] with
    rint(log2(p) * 2^k) clamped below at -150 * 2^k, and GGNN_TREE_FORBIDDEN
    where p <= 0 or p is NaN / +-inf, the row or column is >= n, the row is 0
    or the arc is a self-loop."""
    p = probs_head
    if p.dim() != 3 or p.shape[1] != int(v):
        raise ValueError("probs_head [b, %d, o] expected, got %s" % (int(v), tuple(p.shape)))
    dev = p.device
    o = p.shape[2]
    n = torch.as_tensor(n_nodes, device=dev).to(torch.int64).reshape(-1, 1, 1)
    k = tree_score_shift(v)
    i = torch.arange(int(v), device=dev).reshape(1, -1, 1)
    j = torch.arange(o, device=dev).reshape(1, 1, -1)
    ok = torch.isfinite(p) & (p > 0) & (i < n) & (j < n) & (i != 0) & (i != j)
    q = torch.round(torch.log2(torch.where(ok, p, torch.ones_like(p)).to(torch.float64)) * float(2 ** k))
    q = torch.clamp(q, min=float(-TREE_LOG2_FLOOR * 2 ** k))
    return torch.where(ok, q, torch.full_like(q, float(_lib.TREE_FORBIDDEN))).to(torch.int32).contiguous()


def _decode_input(t, name):
    if t.dim() != 3 or t.dtype != torch.float32 or t.device.type != "cuda":
        raise ValueError("%s must be float32 [b, v, o] tensors on the GPU" % name)
    return t.contiguous()


class EmbedFunction(torch.autograd.Function):
    """h0 = front-end(tables); backward gives the dense table gradients and
    stashes the per-lookup squared norms on ``owner.lookup_sqnorm`` (for
    ClipAdam's IndexedSlices clip)."""

    @staticmethod
    def forward(ctx, fe, owner, wi, keep, seed, cols, *tables):
        segs = list(zip(tables, cols))
        ctx.fe, ctx.owner, ctx.wi, ctx.keep, ctx.seed, ctx.cols = fe, owner, wi, keep, seed, cols
        ctx.tables = tables
        return fe.forward(segs, wi, keep, seed)

    @staticmethod
    def backward(ctx, dh0):
        segs = list(zip(ctx.tables, ctx.cols))
        # segments sharing a table (btb: loc_embeddings for the location and
        # the head location) share one gradient buffer
        first = [next(j for j, u in enumerate(ctx.tables) if u is t) for t in ctx.tables]
        bufs = {}
        for i, t in enumerate(ctx.tables):
            if first[i] == i:
                bufs[i] = torch.empty_like(t)
        dts, sq = ctx.fe.backward(segs, ctx.wi, dh0, ctx.keep, ctx.seed, dtables=[bufs[f] for f in first])
        # (a table's squared lookup norm is in its first segment's slot)
        ctx.owner.lookup_sqnorm = {id(t): sq[first[i]:first[i] + 1] for i, t in enumerate(ctx.tables)}
        out = tuple(bufs[i] if first[i] == i else None for i in range(len(ctx.tables)))
        return (None, None, None, None, None, None) + out


class HeadsFunction(torch.autograd.Function):
    """loss = sum over heads of the btb cross-entropy (tree_loss, OutputHeads.
    forward's: head 0's is the tree-structured loss); also returns the probs
    (computed_values)."""

    @staticmethod
    def forward(ctx, oh, labels, keep, seed, target_num, tree_loss, hT, h0, *wb):
        heads = [(wb[2 * i], wb[2 * i + 1]) for i in range(len(wb) // 2)]
        probs, loss = oh.forward(hT, h0, heads, labels, keep, seed, target_num, tree_loss=tree_loss)
        ctx.oh, ctx.labels, ctx.target_num = oh, labels, target_num
        ctx.save_for_backward(hT, h0, *wb)
        ctx.probs = probs
        ctx.marg = oh.tree_marg
        ctx.mark_non_differentiable(*probs)
        return (loss.sum(),) + tuple(probs)

    @staticmethod
    def backward(ctx, d_loss, *unused):
        hT, h0, *wb = ctx.saved_tensors
        heads = [(wb[2 * i], wb[2 * i + 1]) for i in range(len(wb) // 2)]
        if ctx.oh.tree_marg is not ctx.marg:
            raise RuntimeError("the heads ran another forward since this loss was produced")
        dws, dbs, dhT, dh0 = ctx.oh.backward(hT, h0, heads, ctx.labels, ctx.probs, ctx.target_num,
                                             d_loss.reshape(1).contiguous())
        grads = []
        for dw, db in zip(dws, dbs):
            grads += [dw, db]
        return (None, None, None, None, None, None, dhT, dh0) + tuple(grads)
