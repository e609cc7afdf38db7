"""The max-margin training loss on the GPU: ggnn_margin_loss against the host
form (evaluation.margin_loss_arrays) on the same float32 inputs -- the
integers and the copies equal exactly, the two floating-point results inside
the rounding of a float32 -- and params['structured_loss'] = "*-margin"
through train_step (eager, captured, replayed) and build_loss().backward()
against the float64 oracle, teacher-forced: the cost-augmented tree is
discrete, so it is recomputed by the host form from the device's own
probabilities, required to equal the device's, and then put into the oracle's
backward in the marginals' place."""
import numpy as np
import pytest

import ggnn_oracle as O
import margin_loss_cases as MC
import trajectory_cases as TC
import tree_loss_cases as TL
from decode_cases import _torch
from ggnn_amd import evaluation as E
from test_gpu_heads import TOL, _nmax

pytestmark = pytest.mark.gpu

KINDS = ("nonprojective-margin", "projective-margin")


def _dev(torch, *arrays):
    dev = torch.device("cuda")
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


def _launch(torch, oh, p, y, n, family, single_root, tn, cost, start=0.0):
    """One ggnn_margin_loss; loss = [start, 7] before.  Returns numpy (marg,
    heads, value, hamming, status, used, loss)."""
    loss = torch.tensor([start, 7.0], dtype=torch.float32, device=p.device)
    out = oh.margin_loss(p, y, n, family, single_root, tn, loss, cost)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.float32] + [torch.int32] * 3
    return tuple(t.cpu().numpy() for t in out) + (loss.cpu().numpy(),)


@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family,shape", MC.ABI_CASES, ids=MC.ABI_IDS)
def test_abi_equals_the_host_form(family, shape, single_root):
    torch = _torch()
    from ggnn_amd._lib import PROJ_LDS_MAXN
    from ggnn_amd.heads import OutputHeads
    b, v, o = shape
    oh = OutputHeads(64)
    for seed in MC.SEEDS:
        for cost in MC.COSTS:
            p, y, n, kinds = MC.batch(family, shape, seed, cost)
            if family == 1 and shape == MC.SHAPES[1][-1]:
                assert n.max() > PROJ_LDS_MAXN and 2 <= n[:b].min() <= PROJ_LDS_MAXN     # both storage tiers in one grid
            ref = MC.reference(family, shape, seed, single_root, cost)
            tn = ref["tn"]
            assert ref["used"].tolist() == MC.expected_used(family, b)                   # no graph is left out
            p_t, y_t, n_t = _dev(torch, p, y, n)
            marg, heads, value, hamming, status, used, loss = _launch(torch, oh, p_t, y_t, n_t, family, single_root,
                                                                       tn, cost)
            # the integers and the copies: exactly
            assert np.array_equal(used, ref["used"]) and np.array_equal(status, ref["status"]), (used, status, kinds)
            assert np.array_equal(heads, ref["heads"]), [kinds[g] for g in range(len(n))
                                                         if not np.array_equal(heads[g], ref["heads"][g])]
            assert np.array_equal(hamming, ref["hamming"])
            assert marg.tobytes() == ref["marg"].tobytes()
            # max(0, l) per graph: doubles, one rounding to float32
            raw = np.maximum(ref["raw"], 0.0)
            err = np.abs(value.astype(np.float64) - raw)
            bound = 2.0 ** -22 * np.maximum(1.0, np.abs(ref["raw"]))
            print("family %d %s seed %d cost %g single_root %d: value err at most %.3g of its bound, active %d of %d used"
                  % (family, shape, seed, cost, single_root, (err / bound).max(), int((value > 0).sum()),
                     int(used.sum())))
            assert (err <= bound).all(), (err, bound)
            assert (value[used == 0] == 0).all() and ((value > 0) == (ref["raw"] > 0)).all()
            # the added loss: the per-graph values are doubles, the one float32 rounding is the final add
            off = abs(float(loss[0]) - ref["term"])
            print("loss term %.9g, host %.9g, off by %.3g (bound %.3g)" % (loss[0], ref["term"], off,
                                                                            2.0 ** -22 * abs(ref["term"])))
            assert off <= 2.0 ** -22 * abs(ref["term"]) and loss[1] == 7.0           # (loss_in = 0)
            # a second launch gives the same bytes; into a loss that is not zero the term is added
            again = _launch(torch, oh, p_t, y_t, n_t, family, single_root, tn, cost, start=1.5)
            for a, c in zip((marg, heads, value, hamming, status, used), again):
                assert a.tobytes() == c.tobytes()
            assert abs(float(again[6][0]) - (1.5 + ref["term"])) <= 2.0 ** -22 * (1.5 + abs(ref["term"]))
            assert again[6][1] == 7.0
            # target_num in device memory: bit for bit the by-value form
            tn_t = torch.tensor([tn], dtype=torch.float32, device=p_t.device)
            by_dev = _launch(torch, oh, p_t, y_t, n_t, family, single_root, tn_t, cost)
            for a, c in zip((marg, heads, value, hamming, status, used, loss), by_dev):
                assert a.tobytes() == c.tobytes()


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd._lib import GGNNError
    from ggnn_amd.heads import OutputHeads
    oh = OutputHeads(64)
    p, y, n, _ = MC.batch(0, (6, 9, 12), 0, 1.0)
    p_t, y_t, n_t = _dev(torch, p, y, n)
    loss = torch.zeros(2, dtype=torch.float32, device=p_t.device)
    good = dict(probs_head=p_t, gold_head=y_t, n_nodes=n_t, family=0, single_root=True, target_num=3.0, loss=loss,
                cost=1.0)
    for bad in (dict(family=2), dict(family="projective-margin"), dict(gold_head=y_t[:, :, :9]),
                dict(gold_head=y_t.double()), dict(n_nodes=n_t.long()), dict(n_nodes=n_t[:2]),
                dict(probs_head=p_t.cpu()), dict(loss=loss.double()), dict(cost=-1.0), dict(cost=64.5),
                dict(cost=float("nan")), dict(cost=None),
                dict(workspace=torch.empty(8, dtype=torch.uint8, device=p_t.device))):
        with pytest.raises(ValueError):
            oh.margin_loss(**dict(good, **bad))
    with pytest.raises(GGNNError):
        oh.margin_loss(**dict(good, target_num=0.0))
    # the library's own checks, behind the binding's
    import ctypes
    from ggnn_amd import _lib
    lib = _lib.load()
    b, v, o = p.shape
    need = int(lib.ggnn_margin_loss_workspace_bytes(b, v, o, 0))
    assert need >= 4 * b * v * o + 12 * b * v + 12 * b
    ws = torch.empty(need, dtype=torch.uint8, device=p_t.device)
    outs = [torch.empty(b * v * o, dtype=torch.float32, device=p_t.device) for _ in range(6)]
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(cost=1.0, marg=None, nbytes=need):
        d = _lib.dims(b, v, 64, 1, 1, True, "fp32")
        return lib.ggnn_margin_loss(ctypes.byref(d), P(p_t), o, P(y_t), P(n_t), 0, 1, cost, 3.0,
                                    P(outs[0] if marg is None else marg), P(outs[1]), P(outs[2]), P(outs[3]),
                                    P(outs[4]), P(outs[5]), P(loss), P(ws), nbytes,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call() == 0
    torch.cuda.synchronize()
    loss.zero_()
    for kw in (dict(cost=-0.5), dict(cost=65.0), dict(cost=float("nan")), dict(cost=float("inf")), dict(marg=p_t),
               dict(nbytes=need - 1)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert loss.cpu().tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ the model
def _step_heads(m):
    """The OutputHeads object the model's last step ran on."""
    return next(reversed(m._graphs.values())).heads


def _margin_oracle(m, before, fd, probs_dev, family, cost, single_root=True):
    """The float64 composition of one max-margin step at the variables
    ``before``: trajectory_cases._oracle_forward, the host form of the loss on
    the DEVICE's float32 head probabilities (teacher forcing: T* is discrete),
    then the oracle's backward with onehot(T*) / y / the oracle's own
    probabilities in head 0's probs place.  Returns (loss, local loss, 13
    gradients, the host form's outputs)."""
    spec = TC.spec_of(m)
    drop = dict(embed=m.last_embed, path=m.last_dropout, heads=m.last_heads)
    f = TC._oracle_forward(spec, before, fd, drop)
    e, hd = drop["embed"], drop["heads"]
    b, v = int(fd["num_graphs"]), int(fd["num_vertices"])
    y = np.asarray(fd["target_values_head"], np.float32).reshape(b, v, spec.o)
    n = m._feed_n_nodes(fd)
    host = E.margin_loss_arrays(probs_dev.reshape(b, v, spec.o), y, n, family, single_root, hd["target_num"], cost)
    term, marg, used = host[0], host[1].astype(np.float64), host[6]
    marg[used == 0] = f["probs"][0][used == 0]
    dWs, dbs, dhT, dh0_heads = O.heads_backward(f["hT"], f["h0"], f["heads"], [marg, f["probs"][1]], hd["keep"],
                                                hd["seed"], hd["target_num"])
    gp = O.backward(f["A"], dhT, f["caches"], f["w64"])
    dts, _ = O.embed_backward(f["segs"], f["wi"], spec.hidden, dh0_heads + gp["h0"], e["keep"], e["seed"])
    grads = [gp[k] for k in TC.NAMES[:6]] + [dts[0] + dts[3], dts[1], dts[2], dWs[0], dbs[0], dWs[1], dbs[1]]
    local = float(sum(f["losses"]))
    return local + term, local, grads, host


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_matches_the_teacher_forced_float64_composition(kind):
    """The same real dev batch three times: the step runs eagerly (a shape's
    first batch), is captured, and is replayed."""
    torch = _torch()
    cost = 1.0
    m, data = TL.dev_model(structured_loss=kind)
    family = E.MARGIN_LOSS_KINDS[kind]
    fd = TL.dev_feeds(m, data)[0]
    b = int(fd["num_graphs"])
    params = m.trainable_variables()
    for step in range(3):
        before = [p.detach().cpu().numpy().astype(np.float64) for p in params]
        loss = float(m.train_step(dict(fd)).detach())
        grads = [p.grad.detach().cpu().numpy() for p in params]
        used = m.ops["tree_loss_used"].cpu().numpy()
        hamming = m.ops["margin_loss_hamming"].cpu().numpy()
        probs_dev = m.ops["computed_values"].detach().cpu().numpy()
        oh = _step_heads(m)
        ref_loss, local, ref_grads, host = _margin_oracle(m, before, fd, probs_dev, family, cost)
        _, _, h_heads, h_value, h_hamming, h_status, h_used = host
        assert used.dtype == np.int32 and used.tolist() == [1] * b == h_used.tolist()
        assert np.array_equal(oh.margin_heads.cpu().numpy(), h_heads)              # T*: the device's is the host's
        assert hamming.dtype == np.int32 and np.array_equal(hamming, h_hamming)
        assert np.abs(oh.margin_value.cpu().numpy() - h_value).max() <= 2.0 ** -22 * max(1.0, h_value.max())
        print("%s step %d: loss %.6f (oracle %.6f, local %.6f), hamming %d" % (kind, step, loss, ref_loss, local,
                                                                                 int(hamming.sum())))
        assert abs(loss - ref_loss) <= TOL * abs(ref_loss)
        for i, (g, r) in enumerate(zip(grads, ref_grads)):
            assert _nmax(g, r) <= TOL, (step, TC.NAMES[i], _nmax(g, r))
    st = m.graph_stats
    assert (st["uncaptured"], st["captured"], st["replayed"], st["eager"]) == (1, 1, 2, 0), st


def test_eager_backward_equals_the_train_step_gradients():
    """build_loss().backward() (HeadsFunction carries the option) against
    train_step's flat buffer on one feed, every dropout off."""
    torch = _torch()
    m, data = TL.dev_model(structured_loss="projective-margin", learning_rate=0.0, structured_loss_margin=2.5)
    fd = TL.dev_feeds(m, data)[0]
    params = m.trainable_variables()
    m.feed(dict(fd))
    for p in params:
        p.grad = None
    loss = m.build_loss()
    assert m.ops["tree_loss_used"].cpu().tolist() == [1] * int(fd["num_graphs"])
    eager_hamming = m.ops["margin_loss_hamming"].cpu().tolist()
    loss.backward()
    eager = [p.grad.detach().cpu().numpy().astype(np.float64) for p in params]
    eager_loss = float(loss.detach())
    # (learning rate 0 keeps the variables; train_step writes its gradients into the flat buffer)
    step_loss = float(m.train_step(dict(fd)).detach())
    flat = [p.grad.detach().cpu().numpy() for p in params]
    assert m.ops["margin_loss_hamming"].cpu().tolist() == eager_hamming and sum(eager_hamming) > 0
    assert abs(step_loss - eager_loss) <= 1e-5 * abs(eager_loss)
    for i, (g, r) in enumerate(zip(flat, eager)):
        assert _nmax(g, r) <= 1e-5, (TC.NAMES[i], _nmax(g, r))


def _one_step(torch, **params):
    m, data = TL.dev_model(**params)
    loss = m.train_step(dict(TL.dev_feeds(m, data)[0]))
    torch.cuda.synchronize()
    return (loss.detach().cpu().numpy().tobytes(), m.train_buffer().flat.detach().cpu().numpy().tobytes(),
            m.ops["margin_loss_hamming"])


@pytest.mark.parametrize("kind", [None, "nonprojective", "projective"])
def test_the_margin_is_read_by_the_margin_kinds_only(kind):
    torch = _torch()
    plain = _one_step(torch, structured_loss=kind)
    other = _one_step(torch, structured_loss=kind, structured_loss_margin=2.5)
    assert plain[0] == other[0] and plain[1] == other[1] and plain[2] is None and other[2] is None
    if kind is not None:                                    # and the margin kinds read it
        a = _one_step(torch, structured_loss=kind + "-margin")
        c = _one_step(torch, structured_loss=kind + "-margin", structured_loss_margin=2.5)
        assert a[0] != c[0] and a[0] != plain[0] and a[1] != plain[1]


@pytest.mark.parametrize("kind", KINDS)
def test_training_on_one_batch_brings_the_hamming_distance_down(kind):
    """A direction check only: after a few steps on one batch the cost-
    augmented trees hold fewer wrong heads than at step 1."""
    torch = _torch()
    m, data = TL.dev_model(structured_loss=kind, learning_rate=0.01)
    fd = TL.dev_feeds(m, data)[0]
    sums = []
    for _ in range(8):
        m.train_step(dict(fd))
        sums.append(int(m.ops["margin_loss_hamming"].sum().item()))
    print(kind, "hamming per step:", sums)
    assert sums[-1] < sums[0]
