"""Edge shapes of the output heads (k_head_wdrop, k_head_softmax, k_head_dz,
k_head_dw_out in csrc/k_head.h and the three products: logits, d[hT | h0], dW)
through ``OutputHeads`` against the float64 oracle, on the same inputs and the
same Philox seeds.  One checker (probs, per-head loss, dW, db, dhT, dh0; probs and loss errors are absolute,
the gradients' are max |x - ref| / max |ref|), one axis varied at a time around
a small base case:

* o = 1 .. 1024: every NI instantiation of k_head_softmax / k_head_dz (1, 2, 4,
  16), both sides of each boundary, o % 4 != 0, in calls of 1, 2 and 4 heads;
* H = 3, 50, 100, 400: one launch per half of [hT | h0] (H % 64 != 0), rows
  off a 16-byte boundary when H % 4 != 0;
* rows = b * v = 1 .. 16510: the dW split-K over node rows (Z > 1 chunks, a
  ragged last chunk, KC > 256), the second grid-stride trips of k_head_dz
  (rows > 4096) and k_head_softmax (rows > 16384);
* labels with all-zero rows (padded nodes; dhT and dh0 are exactly 0 there)
  and two-hot rows (sum(y) = 2 in p * sum(y) - y);
* biases of +-100 in a few columns: softmax without the max subtraction
  overflows; labels sit on those columns too (log p = z - lse on both sides);
* d_loss = 0.37 on the device, target_num = 0.75, 20 + 1e-7, 7680.5 (each moves
  the power of two dZ is carried at), keep = 0.5 with a seed >= 2^32;
* the inference call (labels=None): no loss, the training call's probs to the bit;
* the workspace: every case runs on a workspace filled with NaN bytes after a
  first forward, and a small shape after a large one equals a fresh
  OutputHeads bit for bit.

Bars: probs 1e-5 absolute, loss 1e-5 relative + 1e-6, gradients 1e-5 of
max |ref| (those of test_heads_forward_backward_parity).  At the sizes with
longer sums than the old tests reach (everything at H = 400; dW and db at rows
4097, 12289, 16510) the bar is the larger of that and 4 x the error of a plain
float32 numpy restatement of the same operation against the same oracle (the
split-f16 products carry 22 significand bits where fp32 carries 24).  Measured
on an MI355X (yardstick = the float32 restatement's error, kernel = the
kernels' error, same normalisation; the bar in force is max(1e-5, 4 x yardstick)):

    case                              quantity  yardstick  kernel
    H = 400, rows 33, o = (65, 7)     probs     8.2e-08    1.8e-07
                                      loss      7.7e-06    3.9e-06
                                      dW        2.8e-07    4.6e-07
                                      db        1.9e-07    1.8e-07
                                      dhT       2.4e-07    4.5e-07
                                      dh0       2.3e-07    4.3e-07
    the same with biases of +-100     probs     4.0e-06    3.5e-06
                                      loss      1.9e-04    7.2e-05
                                      dW        1.4e-07    1.5e-07
                                      db        9.6e-08    4.7e-08
                                      dhT       9.6e-08    3.9e-07
                                      dh0       9.9e-08    4.5e-07
    rows 4097, H = 12, o = (5, 3)     dW        1.5e-06    1.7e-07
                                      db        1.4e-06    1.4e-07
    rows 12289, H = 64, o = (5, 3)    dW        2.8e-07    2.3e-07
                                      db        1.6e-06    6.7e-08
    rows 16510, H = 12, o = (5, 3)    dW        2.9e-07    1.7e-07
                                      db        2.5e-06    1.1e-07

Everywhere else the kernels land between 1e-8 and 2.2e-6 against the 1e-5 bars
(4e-6 on probs under the +-100 biases, where a logit of 100 has a float32
spacing of 7.6e-6).
"""
import numpy as np
import pytest

import ggnn_oracle as O

pytestmark = pytest.mark.gpu

BIG_SEED = 0x5DEECE66D1234          # >= 2^32: the upper key word is in use
D_LOSS = float(np.float32(0.37))


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _nmax(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _inputs(b, v, h, os_, seed, spread):
    """hT, h0, heads (W Glorot, bias, labels) as float32 values.  Labels: the
    last row and ~20% of the others all zero in every head (padded nodes),
    ~25% of the labelled rows two-hot, the rest one-hot.  spread: biases of
    +-100 in up to four columns per head, some labels on those columns."""
    rng = np.random.default_rng(seed)
    rows = b * v
    hT = rng.uniform(-1, 1, (b, v, h)).astype(np.float32)
    h0 = rng.uniform(-0.5, 0.5, (b, v, h)).astype(np.float32)
    zero = rng.random(rows) < 0.2
    if rows > 1:
        zero[-1], zero[0] = True, False
    else:
        zero[:] = False
    heads = []
    for o in os_:
        W = (np.sqrt(6.0 / (2 * h + o)) * (2 * rng.random((2 * h, o)) - 1)).astype(np.float32)
        bias = (rng.normal(size=o) * 0.1).astype(np.float32)
        col = rng.integers(0, o, rows)
        if spread:
            hot = rng.permutation(o)[:min(o, 4)]
            bias[hot] = np.array([100.0, -100.0, 100.0, -100.0], np.float32)[:len(hot)]
            on_hot = rng.random(rows) < 0.3
            col = np.where(on_hot, hot[rng.integers(0, len(hot), rows)], col)
        y = np.zeros((rows, o), np.float32)
        y[np.arange(rows), col] = 1
        if o >= 2:
            two = rng.random(rows) < 0.25
            col2 = (col + 1 + rng.integers(0, o - 1, rows)) % o
            y[np.arange(rows)[two], col2[two]] = 1
        y[zero] = 0
        heads.append(dict(W=W, b=bias, labels=y.reshape(b, v, o)))
    return hT, h0, heads, zero


def _f32_restatement(hT, h0, heads, keep, seed, tn, d_loss):
    """The same operations in float32 numpy (the yardstick): returns probs,
    losses and a closure for the backward given probs."""
    f = np.float32
    x = np.concatenate([hT, h0], axis=-1).astype(f)
    b, v, K = x.shape
    x = x.reshape(b * v, K)
    probs, losses, parts = [], [], []
    for i, hd in enumerate(heads):
        s = np.ones(hd["W"].shape, f)
        if keep < 1.0:
            s = np.where(O.head_keep_mask(K, hd["W"].shape[1], i, keep, seed), f(1.0) / f(keep), f(0.0)).astype(f)
        Wd = hd["W"].astype(f) * s
        z = x @ Wd + hd["b"].astype(f)
        mx = z.max(axis=1, keepdims=True)
        lse = mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True, dtype=f))
        y = hd["labels"].reshape(b * v, -1).astype(f)
        probs.append(np.exp(z - lse).reshape(b, v, -1))
        losses.append(float(-(y * (z - lse)).sum(dtype=f) * (f(1.0) / f(tn))))
        parts.append((Wd, s, y))

    def backward(ps):
        g = f(d_loss) * (f(1.0) / f(tn))
        dx = np.zeros_like(x)
        dWs, dbs = [], []
        for (Wd, s, y), p in zip(parts, ps):
            p = np.asarray(p, f).reshape(b * v, -1)
            dz = g * (p * y.sum(axis=1, keepdims=True, dtype=f) - y)
            dWs.append((x.T @ dz) * s)
            dbs.append(dz.sum(axis=0, dtype=f))
            dx += dz @ Wd.T
        hd_ = K // 2
        return dWs, dbs, dx[:, :hd_].reshape(b, v, hd_), dx[:, hd_:].reshape(b, v, hd_)

    return probs, losses, backward


def _run(torch, oh, hT, h0, heads, keep, seed, tn, d_loss, poison=True):
    """Training forward (twice, the workspace filled with NaN bytes in between:
    nothing may be read that this call did not write), the inference call,
    backward.  Returns device results as numpy."""
    dev = torch.device("cuda", 0)
    hT_t, h0_t = torch.from_numpy(hT).to(dev), torch.from_numpy(h0).to(dev)
    heads_t = [(torch.from_numpy(hd["W"]).to(dev), torch.from_numpy(hd["b"]).to(dev)) for hd in heads]
    labels = [torch.from_numpy(hd["labels"]).to(dev) for hd in heads]
    probs, loss = oh.forward(hT_t, h0_t, heads_t, labels, keep, seed, tn)
    if poison:
        torch.cuda.synchronize()
        oh._ws.fill_(255)                        # every float of the workspace is a NaN now
        for p in probs:
            p.fill_(float("nan"))
        loss.fill_(float("nan"))
        probs, loss = oh.forward(hT_t, h0_t, heads_t, labels, keep, seed, tn, loss_out=loss, probs_out=probs)
    p_inf, l_inf = oh.forward(hT_t, h0_t, heads_t, None, keep, seed, tn)
    assert l_inf is None                         # the inference call returns no loss ...
    for a, c in zip(p_inf, probs):
        assert torch.equal(a, c)                 # ... and the training call's probs, bit for bit
    dl = None if d_loss is None else torch.tensor([d_loss], dtype=torch.float32, device=dev)
    dws, dbs, dhT, dh0 = oh.backward(hT_t, h0_t, heads_t, labels, probs, tn, d_loss=dl)
    torch.cuda.synchronize()
    n = lambda t: t.cpu().numpy()
    return dict(probs=[n(p) for p in probs], loss=n(loss), dW=[n(x) for x in dws], db=[n(x) for x in dbs],
                dhT=n(dhT), dh0=n(dh0))


def _check(b, v, h, os_, keep=0.85, seed=99, tn=None, d_loss=D_LOSS, spread=False, yard=()):
    """yard: the quantities whose bar is max(existing, 4 x float32 yardstick):
    () (the old tests' sizes), ("dW", "db") or "all"."""
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    tn = float(b) + O.SMALL_NUMBER if tn is None else tn
    hT, h0, heads, zero = _inputs(b, v, h, os_, seed=b * v * 1000 + h + len(os_), spread=spread)
    got = _run(torch, OutputHeads(h), hT, h0, heads, keep, seed, tn, d_loss)
    dl = 1.0 if d_loss is None else d_loss
    rp, rl = O.heads_forward(hT, h0, heads, keep, seed, tn)
    rw, rb, rhT, rh0 = O.heads_backward(hT, h0, heads, got["probs"], keep, seed, tn, d_loss=dl)
    # the float32 yardstick, against the same oracle under the same normalisation
    Y = {}
    if yard:
        fp, fl, fbwd = _f32_restatement(hT, h0, heads, keep, seed, tn, dl)
        fw, fb, fhT, fh0 = fbwd(fp)
        yw, yb, yhT, yh0 = O.heads_backward(hT, h0, heads, fp, keep, seed, tn, d_loss=dl)
        Y = dict(probs=max(float(np.abs(fp[i] - rp[i]).max()) for i in range(len(os_))),
                 loss=max(abs(fl[i] - rl[i]) for i in range(len(os_))),
                 dW=max(_nmax(fw[i], yw[i]) for i in range(len(os_))),
                 db=max(_nmax(fb[i], yb[i]) for i in range(len(os_))), dhT=_nmax(fhT, yhT), dh0=_nmax(fh0, yh0))
    use = (lambda q: yard == "all" or q in yard)
    bar = lambda q, base: max(base, 4.0 * Y[q]) if use(q) else base
    E = dict(probs=max(float(np.abs(got["probs"][i] - rp[i]).max()) for i in range(len(os_))),
             loss=max(abs(float(got["loss"][i]) - rl[i]) for i in range(len(os_))),
             dW=max(_nmax(got["dW"][i], rw[i]) for i in range(len(os_))),
             db=max(_nmax(got["db"][i], rb[i]) for i in range(len(os_))),
             dhT=_nmax(got["dhT"], rhT), dh0=_nmax(got["dh0"], rh0))
    print("\nHEADS b=%d v=%d H=%d o=%s keep=%g tn=%g spread=%d | kernel %s | yardstick %s" % (
        b, v, h, os_, keep, tn, spread, " ".join("%s=%.2e" % kv for kv in E.items()),
        " ".join("%s=%.2e" % (q, Y[q]) for q in Y if use(q)) or "-"))
    for i in range(len(os_)):
        assert np.abs(got["probs"][i] - rp[i]).max() <= bar("probs", 1e-5), i
        assert abs(float(got["loss"][i]) - rl[i]) <= bar("loss", 1e-5 * abs(rl[i]) + 1e-6), i
        assert _nmax(got["dW"][i], rw[i]) <= bar("dW", 1e-5), i
        assert _nmax(got["db"][i], rb[i]) <= bar("db", 1e-5), i
    assert _nmax(got["dhT"], rhT) <= bar("dhT", 1e-5)
    assert _nmax(got["dh0"], rh0) <= bar("dh0", 1e-5)
    # padded nodes: dZ is exactly zero there and the products add zeros
    if zero.any():
        assert not got["dhT"].reshape(b * v, h)[zero].any()
        assert not got["dh0"].reshape(b * v, h)[zero].any()
        assert max(os_) < 2 or np.abs(got["dhT"].reshape(b * v, h)[~zero]).max() > 0
    return got


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("os_", [
    (1,),                   # one head, o = 1: Ot = 4, NI = 1 with a single live lane
    (1000, 63),             # NI = 16 (o % 64 != 0) and NI = 1 (o = 63, o % 4 != 0); second head at offset 1000
    (64, 65, 129, 128),     # four heads (GGNN_MAX_HEADS): NI = 1 full, NI = 2 from below, NI = 4 from below, NI = 2 full
    (257, 256, 1024, 1),    # NI = 16 from below, NI = 4 full, NI = 16 full (HEAD_MAXO), o = 1 last; offsets 260, 516, 1540
])
def test_heads_output_sizes(os_, spread):
    """Every NI branch of the softmax and dz templates, both sides of each
    boundary, in calls of 1, 2 and 4 heads; with Glorot-sized logits and with
    biases of +-100."""
    _check(3, 11, 64, os_, spread=spread)


@pytest.mark.parametrize("h,yard", [
    (3, ()),        # H % 4 != 0: rows of hT, h0, dhT, dh0 off 16-byte boundaries; K = 6 (a partial dropout quad)
    (50, ()),       # H % 4 != 0, one launch per half
    (100, ()),      # H % 4 == 0 but H % 64 != 0: one launch per half on aligned rows
    (400, "all"),   # the reference's default hidden size: one launch per half, K = 800 logit sums
    (128, ()),      # H % 64 == 0: both halves in one launch (output / operand split at H)
])
def test_heads_hidden_sizes(h, yard):
    _check(3, 11, h, (65, 7), yard=yard)
    _check(3, 11, h, (65, 7), spread=True, keep=1.0, yard=yard)


@pytest.mark.parametrize("b,v,h,yard", [
    (1, 1, 12, ()),                    # rows 1: a single labelled row
    (1, 7, 12, ()),                    # rows 7: less than one softmax block's 8 rows
    (1, 257, 64, ()),                  # rows 257: dW split-K Z = 2, 1-row last chunk (both halves in one launch)
    (3, 100, 12, ()),                  # rows 300: Z = 2, 44-row last chunk, one launch per half
    (17, 241, 12, ("dW", "db")),       # rows 4097: second k_head_dz trip (one row in it); Z = 17, 1-row last chunk
    (1, 12289, 64, ("dW", "db")),      # rows 12289: KC = 288, Z = 43, 193-row last chunk
    (130, 127, 12, ("dW", "db")),      # rows 16510: second k_head_softmax trip; KC = 352, Z = 47
])
def test_heads_row_counts(b, v, h, yard):
    _check(b, v, h, (5, 3), keep=0.9, yard=yard)


@pytest.mark.parametrize("tn", [0.75, 20.0 + 1e-7, 7680.5])   # tnum_scale = 2^-1, 2^4, 2^12
def test_heads_target_num(tn):
    _check(3, 11, 64, (65, 7), tn=tn)
    _check(3, 11, 50, (65, 7), tn=tn)


def test_heads_keep_half_big_seed_and_no_dropout():
    # keep = 0.5 with a seed >= 2^32 (the upper Philox key word); keep = 1: no mask at all
    _check(3, 11, 64, (65, 7), keep=0.5, seed=BIG_SEED)
    _check(3, 11, 50, (65, 7), keep=0.5, seed=BIG_SEED, spread=True)
    _check(3, 11, 64, (65, 7), keep=1.0)


def test_heads_without_d_loss():
    # d_loss = NULL: the factor is 1
    _check(3, 11, 64, (65, 7), d_loss=None)


def test_heads_workspace_small_shape_after_large():
    """OutputHeads keeps one workspace and reuses it for a smaller shape.  A
    large shape, then the whole workspace filled with NaN bytes, then forward
    and backward at a smaller shape (another H, another Ot: every region moves):
    bit-identical to a fresh OutputHeads -- every element read is first written
    in the same call."""
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    big = _inputs(4, 64, 64, (150, 46), seed=1, spread=False)
    small = _inputs(3, 7, 50, (65,), seed=2, spread=True)
    for small_shape in (small, _inputs(1, 257, 64, (5, 3), seed=3, spread=False)):
        oh = OutputHeads(64)
        _run(torch, oh, big[0], big[1], big[2], 0.85, 99, 4.0, D_LOSS, poison=False)
        n_big = oh._ws.numel()
        oh._ws.fill_(255)
        reused = _run(torch, oh, small_shape[0], small_shape[1], small_shape[2], 0.85, 99, 3.0, D_LOSS, poison=False)
        assert oh._ws.numel() == n_big             # the large call's workspace, not a new one
        fresh = _run(torch, OutputHeads(small_shape[0].shape[2]), small_shape[0], small_shape[1], small_shape[2], 0.85, 99, 3.0, D_LOSS,
                     poison=False)
        for k in ("probs", "dW", "db"):
            for a, c in zip(reused[k], fresh[k]):
                assert np.array_equal(a, c), k
        for k in ("loss", "dhT", "dh0"):
            assert np.array_equal(reused[k], fresh[k]), k
        assert np.isfinite(reused["dhT"]).all() and np.isfinite(reused["loss"]).all()
