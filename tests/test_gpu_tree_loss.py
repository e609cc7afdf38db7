"""The tree-structured training loss on the GPU: ggnn_tree_loss against the
float64 host form (evaluation.tree_loss_arrays) at the marginal bars of
test_gpu_tree_marginals.py / test_gpu_projective_marginals.py, OutputHeads'
forward / backward with tree_loss= against the oracle's heads with the GPU's
marginals in head 0's probs place, and params['structured_loss'] through
train_step (eager, captured, replayed), build_loss().backward(), the default
and a feed outside the closed-form masks."""
import numpy as np
import pytest

import ggnn_oracle as O
import trajectory_cases as TC
import tree_loss_cases as TL
from decode_cases import _torch
from ggnn_amd import evaluation as E
from test_gpu_heads import TOL, _nmax
from test_tree_marginals import CAP

pytestmark = pytest.mark.gpu

ABI_CASES = [(f, s) for f in (0, 1) for s in TL.SHAPES[f]]


def _dev(torch, *arrays):
    dev = torch.device("cuda")
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


def _launch(torch, oh, p, y, n, family, single_root, tn, start=0.0):
    """One ggnn_tree_loss; loss = [start, 7] before.  Returns numpy (marg, logz, status, used, loss)."""
    loss = torch.tensor([start, 7.0], dtype=torch.float32, device=p.device)
    out = oh.tree_loss(p, y, n, family, single_root, tn, loss)
    torch.cuda.synchronize()
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.int32 and out[3].dtype == torch.int32
    return tuple(t.cpu().numpy() for t in out) + (loss.cpu().numpy(),)


@pytest.mark.parametrize("single_root", [True, False], ids=["single-root", "multi-root"])
@pytest.mark.parametrize("family,shape", ABI_CASES, ids=["%s-%dx%dx%d" % (("all", "proj")[f], *s) for f, s in ABI_CASES])
def test_abi_equals_the_host_form(family, shape, single_root):
    torch = _torch()
    from ggnn_amd._lib import LAPL_LDS_MAXN, MARG_LDS_MAXN
    from ggnn_amd.heads import OutputHeads
    tier = (LAPL_LDS_MAXN, MARG_LDS_MAXN)[family]
    b, v, o = shape
    oh = OutputHeads(64)
    for seed in TL.SEEDS:
        p, y, n, kinds = TL.abi_batch(family, shape, seed)
        if shape == TL.SHAPES[family][-1]:
            assert n.max() > tier and 2 <= n[:b].min() <= tier          # both storage tiers in one grid
        ref = TL.abi_reference(family, shape, seed, single_root)
        tn = ref["tn"]
        assert ref["used"].tolist() == [1] * b + [0] * len(TL.SPECIALS)  # no regular graph is left out
        p_t, y_t, n_t = _dev(torch, p, y, n)
        marg, logz, status, used, loss = _launch(torch, oh, p_t, y_t, n_t, family, single_root, tn)
        assert np.array_equal(used, ref["used"]) and np.array_equal(status, ref["status"]), (used, status, kinds)
        bound = 0.0
        for g in range(len(n)):
            if not used[g]:
                assert marg[g].tobytes() == p[g].tobytes(), kinds[g]
                continue
            m, bar = int(n[g]), float(ref["bar"][g])
            bar_z = bar / 4 + abs(ref["logz"][g]) * 2.0 ** -23
            err = np.abs(marg[g].astype(np.float64) - ref["marg"][g]).max()
            err_z = abs(float(logz[g]) - ref["logz"][g])
            rows = np.abs(marg[g, 1:m].astype(np.float64).sum(axis=1) - 1).max()
            rows_bar = m * 2.0 ** -20 + (bar if family == 0 else 0.0)
            print("family %d n %d seed %d single_root %d: marg err %.3g (bar %.3g), logz err %.3g (bound %.3g), "
                  "row sums off by %.3g (bound %.3g)" % (family, m, seed, single_root, err, bar, err_z, bar_z, rows,
                                                         rows_bar))
            assert bar <= CAP
            # (ln Z per graph: the family's own test's bound; the loss below: the issue's sum of bar_z)
            assert err <= bar and err_z <= (bar_z if family == 0 else bar / 4) and rows <= rows_bar, (
                kinds[g], m, err, bar, err_z, bar_z, rows)
            assert (marg[g, 0] == 0).all() and (marg[g, m:] == 0).all() and (marg[g, :, m:] == 0).all()
            bound += bar_z
        # the added loss: the ln Z bound of every used graph, plus the rounding of the stored fp32
        bound = bound / tn + 2.0 ** -23 * abs(ref["term"])
        print("loss term %.9g, host %.9g, off by %.3g (bound %.3g)" % (loss[0], ref["term"],
                                                                        abs(float(loss[0]) - ref["term"]), bound))
        assert abs(float(loss[0]) - ref["term"]) <= bound
        assert loss[1] == 7.0
        # a second launch gives the same bytes; into a loss that is not zero the term is added
        again = _launch(torch, oh, p_t, y_t, n_t, family, single_root, tn, start=1.5)
        for a, c in zip((marg, logz, status, used), again):
            assert a.tobytes() == c.tobytes()
        assert again[4][0] == np.float32(1.5) + loss[0] and again[4][1] == 7.0
        # target_num in device memory: bit for bit the by-value form
        tn_t = torch.tensor([tn], dtype=torch.float32, device=p_t.device)
        by_dev = _launch(torch, oh, p_t, y_t, n_t, family, single_root, tn_t)
        for a, c in zip((marg, logz, status, used, loss), by_dev):
            assert a.tobytes() == c.tobytes()


def test_binding_validates_its_arguments():
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    oh = OutputHeads(64)
    p, y, n, _ = TL.abi_batch(0, (6, 9, 12), 0)
    p_t, y_t, n_t = _dev(torch, p, y, n)
    loss = torch.zeros(2, dtype=torch.float32, device=p_t.device)
    good = dict(probs_head=p_t, gold_head=y_t, n_nodes=n_t, family=0, single_root=True, target_num=3.0, loss=loss)
    for bad in (dict(family=2), dict(family="eisner"), dict(gold_head=y_t[:, :, :9]), dict(gold_head=y_t.double()),
                dict(n_nodes=n_t.long()), dict(n_nodes=n_t[:2]), dict(probs_head=p_t.cpu()), dict(loss=loss.double()),
                dict(workspace=torch.empty(8, dtype=torch.uint8, device=p_t.device))):
        with pytest.raises(ValueError):
            oh.tree_loss(**dict(good, **bad))
    from ggnn_amd._lib import GGNNError
    with pytest.raises(GGNNError):
        oh.tree_loss(**dict(good, target_num=0.0))
    torch.cuda.synchronize()
    assert loss.cpu().tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ OutputHeads.forward / backward
@pytest.mark.parametrize("family", ["nonprojective", "projective"])
def test_heads_forward_backward_with_tree_loss(family):
    """test_heads_forward_backward_parity's first shape with tree golds on head
    0: chains of uneven sizes, one graph with a gold cycle (not used)."""
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    b, v, h, os_, keep = 4, 20, 64, (150, 12), 1.0
    rng = np.random.default_rng(b * v)
    dev = torch.device("cuda")
    hT = rng.uniform(-1, 1, (b, v, h)).astype(np.float32)
    h0 = rng.uniform(-0.5, 0.5, (b, v, h)).astype(np.float32)
    n = np.asarray([17, 12, 17, 9], np.int32)
    heads_np, heads_t, labels = [], [], []
    for o in os_:
        W = (np.sqrt(6.0 / (2 * h + o)) * (2 * rng.random((2 * h, o)) - 1)).astype(np.float32)
        bb = rng.normal(size=o).astype(np.float32) * 0.1
        y = np.zeros((b, v, o), np.float32)
        if o == os_[0]:
            for g in range(b):
                hs = [0] + list(range(0, int(n[g]) - 1))
                if g == 2:
                    hs[3], hs[4] = 4, 3                    # a cycle
                y[g] = TL.heads_to_gold(hs, v, o)
        else:
            for g in range(b):
                y[g, np.arange(1, n[g]), rng.integers(0, o, int(n[g]) - 1)] = 1
        heads_np.append(dict(W=W, b=bb, labels=y))
        heads_t.append((torch.from_numpy(W).to(dev), torch.from_numpy(bb).to(dev)))
        labels.append(torch.from_numpy(y).to(dev))
    tn = float(heads_np[0]["labels"].sum()) + O.SMALL_NUMBER
    seed = 99
    oh = OutputHeads(h)
    hT_t, h0_t, n_t = torch.from_numpy(hT).to(dev), torch.from_numpy(h0).to(dev), torch.from_numpy(n).to(dev)
    probs, loss = oh.forward(hT_t, h0_t, heads_t, labels, keep, seed, tn, tree_loss=(family, True, n_t))
    marg_t, used = oh.tree_marg, oh.tree_used.cpu().numpy()
    assert used.tolist() == [1, 1, 0, 1]
    rp, rl = O.heads_forward(hT, h0, heads_np, keep, seed, tn)
    # the returned probabilities are still the softmax, the marginals are not
    for i in range(2):
        assert np.abs(probs[i].cpu().numpy() - rp[i]).max() <= 1e-5
    marg = marg_t.cpu().numpy()
    assert marg[2].tobytes() == probs[0][2].cpu().numpy().tobytes()
    assert np.abs(marg[0] - probs[0][0].cpu().numpy()).max() > 1e-2
    # the loss: the cross-entropy plus ln Z of the used graphs (the host form on the device's probabilities)
    term, h_marg, _, _, h_used = E.tree_loss_arrays(probs[0].cpu().numpy(), heads_np[0]["labels"], n, family, True, tn)
    assert h_used.tolist() == used.tolist() and term < 0
    assert abs(float(loss[0]) - (rl[0] + term)) <= 1e-5 * abs(rl[0] + term) + 1e-6
    assert abs(float(loss[1]) - rl[1]) <= 1e-5 * abs(rl[1]) + 1e-6
    assert np.abs(marg - h_marg).max() <= CAP
    before = [p.clone() for p in probs]
    dws, dbs, dhT, dh0 = oh.backward(hT_t, h0_t, heads_t, labels, probs, tn)
    rw, rb, rhT, rh0 = O.heads_backward(hT, h0, heads_np, [marg, probs[1].cpu().numpy()], keep, seed, tn)
    for i in range(2):
        assert _nmax(dws[i].cpu().numpy(), rw[i]) <= 1e-5
        assert _nmax(dbs[i].cpu().numpy(), rb[i]) <= 1e-5
        assert torch.equal(probs[i], before[i])             # the caller's probabilities are not written
    assert _nmax(dhT.cpu().numpy(), rhT) <= 1e-5
    assert _nmax(dh0.cpu().numpy(), rh0) <= 1e-5
    # and it is not the local gradient
    lw = O.heads_backward(hT, h0, heads_np, [p.cpu().numpy() for p in probs], keep, seed, tn)[0]
    assert _nmax(dws[0].cpu().numpy(), lw[0]) > 1e-2
    # a forward without the option forgets the marginals
    oh.forward(hT_t, h0_t, heads_t, labels, keep, seed, tn)
    assert oh.tree_marg is None and oh.tree_used is None


# ------------------------------------------------------------------ the model
def _structured_oracle(m, before, fd, family, single_root=True):
    """The float64 composition of one structured step at the variables
    ``before``: trajectory_cases._oracle_forward, the float64 host form of the
    loss on the float32-cast oracle probabilities, then the oracle's backward
    with those marginals in head 0's probs place.  Returns (loss, local loss,
    13 gradients, used)."""
    spec = TC.spec_of(m)
    drop = dict(embed=m.last_embed, path=m.last_dropout, heads=m.last_heads)
    f = TC._oracle_forward(spec, before, fd, drop)
    e, hd = drop["embed"], drop["heads"]
    b, v = int(fd["num_graphs"]), int(fd["num_vertices"])
    y = np.asarray(fd["target_values_head"], np.float32).reshape(b, v, spec.o)
    n = m._feed_n_nodes(fd)
    term, marg, _, _, used = E.tree_loss_arrays(f["probs"][0].astype(np.float32), y, n, family, single_root,
                                                hd["target_num"])
    dWs, dbs, dhT, dh0_heads = O.heads_backward(f["hT"], f["h0"], f["heads"], [marg, f["probs"][1]], hd["keep"],
                                                hd["seed"], hd["target_num"])
    gp = O.backward(f["A"], dhT, f["caches"], f["w64"])
    dts, _ = O.embed_backward(f["segs"], f["wi"], spec.hidden, dh0_heads + gp["h0"], e["keep"], e["seed"])
    grads = [gp[k] for k in TC.NAMES[:6]] + [dts[0] + dts[3], dts[1], dts[2], dWs[0], dbs[0], dWs[1], dbs[1]]
    local = float(sum(f["losses"]))
    return local + term, local, grads, used


@pytest.mark.parametrize("family", ["nonprojective", "projective"])
def test_train_step_matches_the_float64_composition(family):
    """The same real dev batch three times: the step runs eagerly (a shape's
    first batch), is captured, and is replayed."""
    torch = _torch()
    m, data = TL.dev_model(structured_loss=family)
    fd = TL.dev_feeds(m, data)[0]
    params = m.trainable_variables()
    for step in range(3):
        before = [p.detach().cpu().numpy().astype(np.float64) for p in params]
        loss = float(m.train_step(dict(fd)).detach())
        grads = [p.grad.detach().cpu().numpy() for p in params]
        used = m.ops["tree_loss_used"].cpu().numpy()
        ref_loss, local, ref_grads, ref_used = _structured_oracle(m, before, fd, family)
        assert used.dtype == np.int32 and used.tolist() == [1] * int(fd["num_graphs"]) == ref_used.tolist()
        print("step %d: loss %.6f (oracle %.6f, local %.6f)" % (step, loss, ref_loss, local))
        assert abs(loss - ref_loss) <= TOL * abs(ref_loss)
        assert loss < local and ref_loss < local               # Z < 1: some probability lies outside the trees
        for i, (g, r) in enumerate(zip(grads, ref_grads)):
            assert _nmax(g, r) <= TOL, (step, TC.NAMES[i], _nmax(g, r))
    st = m.graph_stats
    assert (st["uncaptured"], st["captured"], st["replayed"], st["eager"]) == (1, 1, 2, 0), st


def test_eager_backward_equals_the_train_step_gradients():
    """build_loss().backward() (HeadsFunction carries the option) against
    train_step's flat buffer on one feed, every dropout off."""
    torch = _torch()
    m, data = TL.dev_model(structured_loss="nonprojective", learning_rate=0.0)
    fd = TL.dev_feeds(m, data)[0]
    params = m.trainable_variables()
    m.feed(dict(fd))
    for p in params:
        p.grad = None
    loss = m.build_loss()
    assert m.ops["tree_loss_used"].cpu().tolist() == [1] * int(fd["num_graphs"])
    loss.backward()
    eager = [p.grad.detach().cpu().numpy().astype(np.float64) for p in params]
    eager_loss = float(loss.detach())
    # (learning rate 0 keeps the variables; train_step writes its gradients into the flat buffer)
    step_loss = float(m.train_step(dict(fd)).detach())
    flat = [p.grad.detach().cpu().numpy() for p in params]
    assert abs(step_loss - eager_loss) <= 1e-5 * abs(eager_loss)
    for i, (g, r) in enumerate(zip(flat, eager)):
        assert _nmax(g, r) <= 1e-5, (TC.NAMES[i], _nmax(g, r))


def _one_step(torch, fd, **params):
    m, data = TL.dev_model(**params)
    loss = m.train_step(dict(fd(m, data)))
    torch.cuda.synchronize()
    return (loss.detach().cpu().numpy().tobytes(), m.train_buffer().flat.detach().cpu().numpy().tobytes(),
            None if m.ops["tree_loss_used"] is None else m.ops["tree_loss_used"].cpu().tolist())


def test_default_is_the_local_step_bit_for_bit():
    torch = _torch()
    first = lambda m, data: TL.dev_feeds(m, data)[0]
    absent = _one_step(torch, first)
    none = _one_step(torch, first, structured_loss=None)
    on = _one_step(torch, first, structured_loss="nonprojective")
    assert absent[0] == none[0] and absent[1] == none[1] and absent[2] is None and none[2] is None
    assert on[0] != absent[0] and on[1] != absent[1] and set(on[2]) == {1}


def test_a_feed_outside_the_closed_form_trains_with_the_local_loss():
    torch = _torch()

    def odd(m, data):
        fd = TL.dev_feeds(m, data)[0]
        mask = np.array(fd["node_mask"], copy=True)
        mask.reshape(-1)[0] = 0.5                              # not get_mask's closed form: no node counts
        return dict(fd, node_mask=mask)
    off = _one_step(torch, odd)
    on = _one_step(torch, odd, structured_loss="nonprojective")
    assert on[0] == off[0] and on[1] == off[1]
    assert on[2] == [0] * len(on[2]) and len(on[2]) > 0
