"""Edge shapes of the embedding front-end kernels (k_embed_fwd, k_embed_bwd,
k_embed_bwd_det + k_embed_fin, k_embed_rows in csrc/k_head.h) through
``EmbeddingFrontEnd`` against the float64 oracle, on the same ids and the same
Philox seeds.  Every backward case runs both forms: the fixed-point
deterministic one (ggnn_embed_backward_ws) and the fp32 atomics
(ggnn_embed_backward), except a segment without a d_table, which only the
workspace form accepts.

Reached here: ids outside [0, rows) (skipped by all four kernels; each gradient
table sits between sentinel margins), widths 1, 3, 65 and 130 (one, two and
three lane trips of k_embed_fin), widths that fill H exactly and widths that
leave padding, H % 4 != 0, b * v = 1 and b * v = 1, 2, 3 (mod 4), eight
segments of which three share a table, a segment without a gradient, the capped
grids (4096 blocks backward, 8192 forward), a squared-norm partial count that
is no multiple of 256, one id hit by every lookup, and the IndexedSlices pair
lookup_rows -> union_backward in one process.

Bars (those of test_embed_forward_backward_parity): forward 1e-6, table
gradients 1e-5 of max |ref|, squared lookup norms 1e-5 relative; bit equality
and the fixed-point bound where stated.
"""
import numpy as np
import pytest

import ggnn_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
BIG_SEED = 0x1234ABCDEF55          # >= 2^32: the upper key word is in use

# tables: (rows, width); segs: table index per segment, in concat order
LAYOUTS = {
    # widths 1 + 3 + 3 + 3 fill H = 10 exactly (no padding), H % 4 != 0, one table looked up twice
    "exact10": dict(H=10, tables=[(6, 1), (5, 3), (7, 3)], segs=[0, 1, 2, 1]),
    # widths 65 and 130: two and three lane trips of k_embed_fin; 5 columns of padding
    "wide200": dict(H=200, tables=[(9, 65), (4, 130)], segs=[0, 1]),
    # eight segments (EMB_MAXSEG), three of them on table 0 and its d_table; 21 columns of padding
    "eight64": dict(H=64, tables=[(11, 3), (5, 1), (8, 20), (3, 2), (6, 7), (9, 4)], segs=[0, 1, 2, 0, 3, 4, 0, 5]),
    # the capped grids: 199 of 256 columns; 394 of 512 columns
    "cap256": dict(H=256, tables=[(40, 65), (30, 130), (50, 3), (20, 1)], segs=[0, 1, 2, 3]),
    "cap512": dict(H=512, tables=[(40, 65), (30, 130), (50, 3), (20, 1)], segs=[0, 1, 2, 3, 1, 0]),
    # one id hit by every lookup
    "hot68": dict(H=68, tables=[(5, 65), (4, 3)], segs=[0, 1]),
    # one segment as wide as H (the slices case)
    "full24": dict(H=24, tables=[(13, 24)], segs=[0]),
}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _nmax(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


class Case:
    """One layout at one batch shape: tables, ids, upstream gradients on the
    host (float32 values) and on the device."""

    def __init__(self, torch, layout, b, v, seed, oor=None, hot=None):
        L = LAYOUTS[layout]
        self.torch, self.b, self.v, self.H = torch, b, v, L["H"]
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(seed)
        self.tables = [rng.normal(size=t).astype(np.float32) for t in L["tables"]]
        self.seg_table = list(L["segs"])
        nseg = len(self.seg_table)
        self.ncols = nseg + 1
        self.cols = [nseg - i for i in range(nseg)]          # (columns in reverse: column != segment index)
        wi = np.zeros((b, v, self.ncols), np.int64)
        for s, ti in enumerate(self.seg_table):
            rows = self.tables[ti].shape[0]
            ids = rng.integers(0, rows, (b, v)) if hot is None else np.full((b, v), hot)
            if oor is not None:
                # ids just outside the table (-1 and rows), and, "far", a large positive and the most negative id
                bad = np.array([-1, rows] + ([1 << 30, -(1 << 31)] if oor == "far" else []))
                hit = rng.random(b * v) < 0.25
                pick = bad[rng.integers(0, len(bad), b * v)]
                k = min(len(bad), b * v)                     # (every bad value at least once when b * v allows)
                where = rng.permutation(b * v)[:k]
                hit[where], pick[where] = True, bad[:k]
                ids = np.where(hit, pick, ids.reshape(-1)).reshape(b, v)
            wi[:, :, self.cols[s]] = ids
        self.wi = wi
        self.G = rng.normal(size=(b, v, self.H)).astype(np.float32)
        self.G2 = rng.normal(size=(b, v, self.H)).astype(np.float32)
        self.segs_np = [(self.tables[ti], self.cols[s]) for s, ti in enumerate(self.seg_table)]
        self.tables_t = [torch.from_numpy(t).to(self.dev) for t in self.tables]
        self.segs = [(self.tables_t[ti], self.cols[s]) for s, ti in enumerate(self.seg_table)]
        self.wi_t = torch.from_numpy(wi.astype(np.int32)).to(self.dev)

    def grad_buffers(self):
        """One gradient table per table, each inside a larger sentinel-filled
        buffer (a margin wider than any row either side; every other margin is
        an odd number of floats, so that table starts off a 16-byte boundary)."""
        torch = self.torch
        out = []
        for i, t in enumerate(self.tables):
            m, n = 132 + (i % 2), t.size
            buf = torch.full((m + n + m,), SENTINEL, dtype=torch.float32, device=self.dev)
            out.append((buf[m:m + n].view(t.shape), buf, m, n))
        return out

    def check_forward(self, keep, seed):
        from ggnn_amd.heads import EmbeddingFrontEnd
        h0 = EmbeddingFrontEnd(self.H).forward(self.segs, self.wi_t, keep, seed)
        ref = O.embed_forward(self.segs_np, self.wi, self.H, keep, seed)
        got = h0.cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
        assert not got[ref == 0.0].any()      # dropped, padded and out-of-range elements are exactly 0
        return ref

    def check_backward(self, keep, seed, deterministic, add=True, no_grad_seg=None):
        """Table gradients, squared lookup norms, untouched margins, zeroed workspace."""
        from ggnn_amd.heads import EmbeddingFrontEnd
        torch = self.torch
        fe = EmbeddingFrontEnd(self.H, deterministic=deterministic)
        assert fe.deterministic == deterministic
        bufs = self.grad_buffers()
        dtables = [bufs[ti][0] for ti in self.seg_table]
        if no_grad_seg is not None:
            dtables[no_grad_seg] = None
        G_t = torch.from_numpy(self.G).to(self.dev)
        G2_t = torch.from_numpy(self.G2).to(self.dev) if add else None
        sq = torch.full((len(self.segs),), float("nan"), dtype=torch.float32, device=self.dev)
        fe.backward(self.segs, self.wi_t, G_t, keep, seed, dh0_add=G2_t, dtables=dtables, sq_out=sq)
        torch.cuda.synchronize()
        up = self.G.astype(np.float64) + (self.G2 if add else 0.0)
        rd, rsq = O.embed_backward(self.segs_np, self.wi, self.H, up, keep, seed)
        sq_ref = np.zeros(len(self.segs))
        for ti in range(len(self.tables)):
            mine = [s for s, u in enumerate(self.seg_table) if u == ti and s != no_grad_seg]
            view, buf, m, n = bufs[ti]
            assert bool((buf[:m] == SENTINEL).all()) and bool((buf[m + n:] == SENTINEL).all()), "margin of table %d" % ti
            if not mine:
                assert bool((view == SENTINEL).all())      # no gradient asked for: not touched at all
                continue
            ref = sum(rd[s] for s in mine)
            assert _nmax(view.cpu().numpy(), ref) <= 1e-5, "table %d" % ti
            sq_ref[mine[0]] = sum(rsq[s] for s in mine)   # one norm per table, in its first segment's slot
        got_sq = sq.cpu().numpy()
        np.testing.assert_allclose(got_sq, sq_ref, rtol=1e-5, atol=0)
        assert not got_sq[sq_ref == 0.0].any()
        if deterministic:
            for ws in fe._ws.values():
                assert int(ws.count_nonzero()) == 0, "the deterministic workspace is not all zero after the call"
        return fe, [b_[0] for b_ in bufs], got_sq


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("layout,b,v,keep,oor", [
    ("exact10", 1, 1, 1.0, None),      # b = v = 1; widths fill H exactly, H % 4 != 0
    ("exact10", 3, 7, 0.6, "near"),    # b * v = 21 = 1 (mod 4); ids -1 and rows (one row before / after the table)
    ("exact10", 2, 5, 0.6, "far"),     # b * v = 10 = 2 (mod 4); also a large positive id and INT32_MIN
    ("wide200", 1, 3, 1.0, None),      # b * v = 3; widths 65, 130: the lane loop of k_embed_fin; padding columns
    ("wide200", 5, 23, 0.55, "far"),   # b * v = 115 = 3 (mod 4), dropout over the last partial row quad
    ("eight64", 3, 7, 0.7, None),      # eight segments, three sharing one table and one d_table
    ("eight64", 2, 5, 1.0, "near"),    # the same with out-of-range ids in every segment
])
def test_embed_edges(layout, b, v, keep, oor, deterministic):
    torch = _torch()
    c = Case(torch, layout, b, v, seed=b * 100 + v, oor=oor)
    c.check_forward(keep, BIG_SEED)
    c.check_backward(keep, BIG_SEED, deterministic)


def test_embed_segment_without_gradient():
    """A segment whose d_table is NULL (workspace form only): its columns are
    skipped, its squared-norm slot is 0, the other segments are unaffected --
    also when the skipped segment shares its table with segments that do have
    a gradient."""
    torch = _torch()
    c = Case(torch, "eight64", 3, 7, seed=5, oor="near")
    c.check_backward(0.7, BIG_SEED, True, no_grad_seg=2)    # table 2's only segment: no gradient for the table
    c.check_backward(0.7, BIG_SEED, True, no_grad_seg=3)    # one of table 0's three segments
    c.check_backward(1.0, 0, True, no_grad_seg=0)           # table 0's first segment: the slot moves to segment 3


@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("layout,b,v", [
    # ceil(rows / 4) * H / 256 = 4128 blocks > EMB_SQ_BLOCKS = 4096: the backward's grid-stride loop takes a
    # second trip; keep < 1: the Philox quad counters at r up to 16509
    ("cap256", 130, 127),
    # 1250 quads * 64 / 256 = 313 squared-norm partials: more than 256 and no multiple of it (k_embed_fin's
    # last block sums two partials per thread, the last threads none)
    ("eight64", 50, 100),
])
def test_embed_backward_large_grids(layout, b, v, deterministic):
    torch = _torch()
    c = Case(torch, layout, b, v, seed=b + v, oor="far")
    c.check_backward(0.8, BIG_SEED, deterministic)


def test_embed_forward_capped_grid():
    """(130, 127, 512): 4128 quads * 512 / 256 = 8256 blocks > grid1d's 8192:
    k_embed_fwd's grid-stride loop takes a second trip."""
    torch = _torch()
    c = Case(torch, "cap512", 130, 127, seed=3, oor="far")
    c.check_forward(1.0, 0)


@pytest.mark.parametrize("deterministic", [True, False])
def test_embed_hot_row(deterministic):
    """Every one of 2000 lookups hits id 2 (keep 1, no dh0_add).  The
    deterministic form rounds each addend to 2^-40 (at most 2^-41 off each) and
    converts the exact fixed-point sum to float32 once: within one float32 ulp
    of the float64 sum plus lookups * 2^-41.  The atomics form: the usual bar."""
    torch = _torch()
    b, v = 8, 250
    c = Case(torch, "hot68", b, v, seed=9, hot=2)
    _, dts, _ = c.check_backward(1.0, 0, deterministic, add=False)
    if not deterministic:
        return
    rd, _ = O.embed_backward(c.segs_np, c.wi, c.H, c.G.astype(np.float64), 1.0, 0)
    for got, ref in zip(dts, rd):
        got = got.cpu().numpy().astype(np.float64)
        bound = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + b * v * 2.0 ** -41
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
        assert not got[[0, 1, 3]].any()                     # rows nobody looked up stay zero


@pytest.mark.parametrize("layout,seg,b,v", [
    # one segment as wide as H, one squared-norm partial block in both calls: the two calls add the same
    # squares in the same order, so the norm is the same bits too
    ("full24", 0, 3, 7),
    # a segment among others (offset 4, width 20): table bits equal; the norm's fp32 sum runs in another order
    ("eight64", 2, 3, 7),
])
def test_embed_slices_union_matches_dense_backward(layout, seg, b, v):
    """IndexedSlices in one process: lookup_rows with cap > rows (ids past the
    batch and out-of-range ids are -1), fed to union_backward, gives the bits of
    backward's table gradient; the two halves of the slices in either order
    give those bits again (64-bit fixed-point sums do not depend on the order)."""
    torch = _torch()
    from ggnn_amd.heads import EmbeddingFrontEnd
    c = Case(torch, layout, b, v, seed=21, oor="far")
    keep, seed, dev = 0.7, BIG_SEED, c.dev
    ti = c.seg_table[seg]
    assert c.seg_table.count(ti) == 1
    fe, dts, sq = c.check_backward(keep, seed, True)
    dense = dts[ti].clone()
    rows_n, width = c.tables[ti].shape
    n, cap = b * v, 32
    rows = torch.full((cap, width), float("nan"), dtype=torch.float32, device=dev)
    ids = torch.full((cap,), 12345, dtype=torch.int32, device=dev)
    G_t, G2_t = torch.from_numpy(c.G).to(dev), torch.from_numpy(c.G2).to(dev)
    fe.lookup_rows(c.segs, seg, c.wi_t, G_t, keep, seed, rows, ids, dh0_add=G2_t)
    # the slices against the oracle's masked upstream gradient
    off = sum(c.tables[u].shape[1] for u in c.seg_table[:seg])
    up = c.G.astype(np.float64) + c.G2
    mask = O.emb_keep_mask(n, c.H, keep, seed)
    up = np.where(mask, up.reshape(n, c.H) / np.float64(np.float32(keep)), 0.0)[:, off:off + width]
    ids_ref = c.wi[:, :, c.cols[seg]].reshape(-1)
    ids_ref = np.where((ids_ref >= 0) & (ids_ref < rows_n), ids_ref, -1)
    assert (ids_ref == -1).any()
    assert np.array_equal(ids.cpu().numpy(), np.concatenate([ids_ref, np.full(cap - n, -1)]))
    got_rows = rows.cpu().numpy()
    assert np.abs(got_rows[:n] - up).max() <= 1e-6 * max(1.0, np.abs(up).max())
    assert not got_rows[n:].any()
    table = c.tables_t[ti]

    def union(r, i):
        dt = torch.full_like(table, float("nan"))
        s = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        fe.union_backward(table, dt, r, i, s)
        torch.cuda.synchronize()
        return dt, s

    dt, s = union(rows, ids)
    assert torch.equal(dt, dense)
    if layout == "full24":
        assert float(s) == float(sq[seg])
    else:
        assert abs(float(s) - float(sq[seg])) <= 1e-6 * float(sq[seg])
    h = cap // 2
    for order in ((0, 1), (1, 0)):
        r = torch.cat([rows[o * h:(o + 1) * h] for o in order]).contiguous()
        i = torch.cat([ids[o * h:(o + 1) * h] for o in order]).contiguous()
        dt2, s2 = union(r, i)
        assert torch.equal(dt2, dense)
        # (the squared norm is an fp32 sum in row order: equal to rounding, not to the bit, once the rows move)
        assert abs(float(s2) - float(sq[seg])) <= 1e-6 * float(sq[seg])
    for ws in fe._ws.values():
        assert int(ws.count_nonzero()) == 0
