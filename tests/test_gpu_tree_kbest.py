"""ggnn_tree_kbest on the GPU against the host form
(evaluation.tree_kbest_arrays): heads, totals, count and status bit-identical,
integers, no tolerance.  The two launches of tests/tree_kbest_cases.py: the main
one (v = 34: n = 1, 2, 3, 5, 23, 33, 34, a graph with a word that has no
allowed head and a range-rule violator) at K = 1, 2, 16, and the wave-boundary
one (v = 66: n = 63, 64, 65, 66) at K = 2, both root modes and the three input
kinds (tree_scores of softmax rows, 25 % forbidden arcs, tie-heavy coarse
scores); one graph n = v = 256 at K = 2; garbage in the padding; rank 0 against
ggnn_tree_decode made to run; two launches' bytes; K = 4 as a prefix of K = 16;
the caller's workspace of exactly the stated bytes; the binding's checks; the
model's predict_batch(kbest=, kbest_family="nonprojective") / parse_kbest(
family="nonprojective") against the host chain."""
import numpy as np
import pytest

from decode_cases import _synthetic_model, _synthetic_raw, _torch
from ggnn_amd import evaluation as E
from tree_kbest_cases import KINDS, launch, reference, scores_batch, with_garbage

pytestmark = pytest.mark.gpu


def _run(torch, s, n, K, single_root, workspace=None):
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    out = OutputHeads(64).tree_kbest(t(s), t(n), K, single_root, workspace)
    torch.cuda.synchronize()
    assert all(x.dtype == torch.int32 for x in out)
    return tuple(x.cpu().numpy() for x in out)


def _same(got, ref, what):
    for name, a, c in zip(("heads", "totals", "count", "status"), got, ref):
        assert a.shape == c.shape and a.tobytes() == c.tobytes(), (what, name, np.argwhere(a != c)[:8].tolist())


@pytest.mark.parametrize("single_root", [True, False], ids=["single", "multi"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [1, 2, 16])
def test_kernel_lists_equal_host_lists(K, kind, single_root):
    torch = _torch()
    s, n = launch("main", kind)
    assert s.shape == (9, 34, 37) and n.tolist() == [1, 2, 3, 5, 23, 33, 34, 6, 4]
    ref = reference("main", kind, single_root, K)
    got = _run(torch, s, n, K, single_root)
    _same(got, ref, (K, kind, single_root))
    _same(_run(torch, s, n, K, single_root), got, "two launches")
    if kind == "soft" and K == 16:
        assert got[2][2] == (2 if single_root else 3)             # count < K: the list ends with the trees


@pytest.mark.parametrize("single_root", [True, False], ids=["single", "multi"])
@pytest.mark.parametrize("kind", KINDS)
def test_wave_boundary_lists_equal_host_lists(kind, single_root):
    torch = _torch()
    s, n = launch("wave", kind)
    assert s.shape == (4, 66, 69) and n.tolist() == [63, 64, 65, 66]
    got = _run(torch, s, n, 2, single_root)
    _same(got, reference("wave", kind, single_root, 2), (kind, single_root))
    _same(_run(torch, s, n, 2, single_root), got, "two launches")


def test_one_graph_of_256_nodes():
    torch = _torch()
    s = scores_batch([256], 256, 256, "soft", 5)
    got = _run(torch, s, np.asarray([256], np.int32), 2, True)
    _same(got, E.tree_kbest_arrays(s, [256], 2, True), "n = v = 256")
    assert got[2].tolist() == [2] and got[1][0, 0] >= got[1][0, 1]


@pytest.mark.parametrize("single_root", [True, False], ids=["single", "multi"])
def test_garbage_in_the_padding_changes_nothing(single_root):
    torch = _torch()
    s, n = launch("main", "forbid")
    dirty = with_garbage(s, n)
    assert not np.array_equal(s, dirty)
    _same(_run(torch, dirty, n, 2, single_root), reference("main", "forbid", single_root, 2), single_root)


@pytest.mark.parametrize("kind", ["forbid", "ties"])
def test_rank_0_is_the_tree_decodes_tree(kind):
    """ggnn_tree_decode on a pred without heads (so that its pass runs) returns
    rank 0's heads, and leaves alone what the k-best gives status 2."""
    torch = _torch()
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    s, n = launch("main", kind)
    b, v, _ = s.shape
    for single_root in (True, False):
        heads, _, count, status = _run(torch, s, n, 2, single_root)
        pred = torch.full((b, v, 2), -1, dtype=torch.int32, device=dev)
        st = OutputHeads(64).tree_decode(torch.from_numpy(np.array(s)).to(dev), torch.from_numpy(np.array(n)).to(dev),
                                         pred, single_root=single_root).cpu().numpy()
        pred = pred.cpu().numpy()
        # (the decode has no range rule: the violator, graph 8, is repaired there and status 2 here)
        assert np.array_equal(st[:8], status[:8]) and (st[4:7] == 1).all() and status[8] == 2
        assert np.array_equal(np.where((st == 1)[:, None], pred[:, :, 0], -1)[:8], heads[:8, 0])


def test_k4_is_a_prefix_of_k16():
    torch = _torch()
    s, n = launch("main", "ties")
    for single_root in (True, False):
        a = _run(torch, s, n, 4, single_root)
        c = _run(torch, s, n, 16, single_root)
        assert a[0].tobytes() == np.ascontiguousarray(c[0][:, :4]).tobytes()
        assert a[1].tobytes() == np.ascontiguousarray(c[1][:, :4]).tobytes()
        assert np.array_equal(a[2], np.minimum(c[2], 4)) and np.array_equal(a[3], c[3]) and (c[2] > 4).any()


@pytest.mark.parametrize("K", [1, 16])
def test_callers_workspace_of_exactly_the_stated_bytes(K):
    torch = _torch()
    from ggnn_amd import _lib
    s, n = launch("main", "soft")
    b, v, _ = s.shape
    need = int(_lib.load().ggnn_tree_kbest_workspace_bytes(b, v, K))
    assert need == b * 4 * (K * (2 * v + 16) + 16) > 0
    ws = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=torch.device("cuda"))
    mine = _run(torch, s, n, K, True)
    _same(_run(torch, s, n, K, True, workspace=ws[:need]), mine, "own workspace")
    _same(mine, reference("main", "soft", True, K), "reference")
    assert (ws[need:].cpu().numpy() == 0xA5).all()                # nothing past the stated bytes
    assert not (ws[:need].cpu().numpy() == 0xA5).all()            # (the records were written there)
    with pytest.raises(ValueError):
        _run(torch, s, n, K, True, workspace=ws[:need - 1])


def test_binding_and_library_validate_their_arguments():
    import ctypes
    torch = _torch()
    from ggnn_amd import _lib
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda")
    oh = OutputHeads(64)
    s = torch.from_numpy(scores_batch([4, 4], 4, 6, "soft", 1)).to(dev)
    n = torch.full((2,), 4, dtype=torch.int32, device=dev)
    for bad in (dict(scores=s.float()), dict(scores=s.cpu()), dict(n_nodes=n.long()), dict(n_nodes=n[:1]),
                dict(scores=s[:, :, :3]), dict(K=0), dict(K=17),
                dict(workspace=torch.empty(4096, dtype=torch.float32, device=dev)),
                dict(workspace=torch.empty(4096, dtype=torch.uint8)),
                dict(workspace=torch.empty(8, dtype=torch.uint8, device=dev))):
        with pytest.raises(ValueError):
            oh.tree_kbest(**dict(dict(scores=s, n_nodes=n, K=2), **bad))
    # the library itself: one byte less, K = 0, K = 17 and v > o are error returns without a launch
    lib = _lib.load()
    v = 12
    big = torch.zeros(1, v, v, dtype=torch.int32, device=dev)
    need = int(lib.ggnn_tree_kbest_workspace_bytes(1, v, 2))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = [torch.full(shape, 7, dtype=torch.int32, device=dev) for shape in ((1, 2, v), (1, 2), (1,), (1,))]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    one = torch.full((1,), v, dtype=torch.int32, device=dev)

    def call(v_, o, K, nbytes):
        d = _lib.dims(1, v_, 64, 1, 1, True, "fp32")
        return lib.ggnn_tree_kbest(ctypes.byref(d), ptr(big), o, ptr(one), 1, K, *(ptr(t) for t in out), ptr(ws), nbytes,
                                   None)
    for args in ((v, v, 2, need - 1), (v, v, 0, need), (v, v, 17, need), (v, v - 1, 2, need)):
        assert call(*args) == -1, args
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 7).all() for t in out)         # nothing was launched
    heads, totals, count, status = oh.tree_kbest(s, n, 2)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [1, 1] and count.cpu().tolist() == [2, 2]


def test_model_lists_agree_with_the_host_chain():
    _torch()
    from ggnn_amd.decoding import HostDecoder, decode_chain
    m = _synthetic_model(False)
    raw = _synthetic_raw()
    K = 3
    trees, log_probs = m.parse_kbest(raw, K, family="nonprojective")
    data = m.process_raw_graphs([{**d, "id": k} for k, d in enumerate(raw)], False)
    o, oe = m.params["output_size"], m.output_size_edges
    compared = 0
    for feed in m.make_minibatch_iterator(data, False):
        b, v = int(feed["num_graphs"]), int(feed["num_vertices"])
        plain = m.predict_batch(dict(feed))
        got = m.predict_batch(dict(feed), kbest=K, kbest_family="nonprojective")
        assert set(got) - set(plain) == {"kbest_heads", "kbest_count", "kbest_status", "kbest_log_prob"}
        assert np.array_equal(got["heads"], plain["heads"])
        hp = m.ops["computed_values"].detach().reshape(b, v, o).cpu().numpy()
        hp_e = m.ops["computed_values_edges"].detach().reshape(b, v, oe).cpu().numpy()
        n = np.asarray(got["n_nodes"], np.int32)
        host = decode_chain(HostDecoder(), hp, hp_e, n, None, False, True, kbest=K, kbest_family="nonprojective")
        assert got["kbest_heads"].tobytes() == host["kbest_heads"].tobytes()
        assert np.array_equal(got["kbest_count"], host["kbest_count"])
        assert np.array_equal(got["kbest_status"], host["kbest_status"])
        scale = np.log(2.0) / 2.0 ** E.tree_score_shift(v)
        present = np.arange(K)[None, :] < host["kbest_count"][:, None]
        want = np.where(present, host["kbest_total"].astype(np.float64) * scale, -np.inf).astype(np.float32)
        assert got["kbest_log_prob"].tobytes() == want.tobytes()
        mbr = m.predict_batch(dict(feed), tree="mbr", kbest=K, kbest_family="nonprojective")   # never the marginals' scores
        assert mbr["kbest_heads"].tobytes() == got["kbest_heads"].tobytes()
        for g, k in enumerate(got["sentences_id"]):
            m_g = int(n[g])
            c = int(got["kbest_count"][g])
            assert [[h for h, _ in t] for t in trees[k]] == [list(map(int, x[1:m_g])) for x in got["kbest_heads"][g, :c]]
            assert log_probs[k] == [float(x) for x in got["kbest_log_prob"][g, :c]]
        compared += b
    assert compared == len(raw)
