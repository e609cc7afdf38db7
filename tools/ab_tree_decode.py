"""Timing of the tree-constrained decode (ggnn_tree_decode) against the plain
decode and against its host form, HIP events around warmed-up launches.

    python tools/ab_tree_decode.py                 # the two kernel sizes
    python tools/ab_tree_decode.py --epoch         # + score_epoch / parse on the dev set

Per size (b, v, o) and regime it prints one JSON line:
  decode_ms        ggnn_heads_decode alone
  decode_tree_ms   ggnn_heads_decode + ggnn_tree_decode (scores built before)
  scores_ms        heads.tree_scores (torch plumbing) alone
  host_ms          the batch's scores / n / pred fetched + evaluation.tree_decode_arrays
Regimes: "flat" -- head probabilities as an untrained model gives them (a
softmax of N(0, 0.1^2) logits over the real columns: the arg-max is close to
random and nearly every graph is repaired, the worst case); "peaked" -- 0.9 on
a gold tree's arcs: every graph takes the fast path.  The device and host
statuses and tree totals are compared on the way.

    python tools/ab_tree_decode.py --projective [--epoch]

alternates, in the same process, the MST path above with decode +
ggnn_projective_decode on the same inputs and adds to every line
  decode_proj_ms   ggnn_heads_decode + ggnn_projective_decode
  proj_ms          decode_proj_ms - decode_ms (beside tree_ms)
  proj_status      graphs with status 0 / 1 / 2 (beside status, the MST's)
  host_proj_ms     the fetch + evaluation.projective_decode_arrays
and a third regime, "peaked-projective": 0.9 on a random PROJECTIVE gold
tree's arcs, so every graph takes the projective fast path ("peaked"'s gold
trees generally cross: there the arg-max is a non-projective tree, the MST
pass takes its fast path and the projective pass repairs every graph with few
changes).  --epoch then also scores the dev set with tree="projective".

    python tools/ab_tree_decode.py --marginals [--epoch]

alternates, in one process, the plain decode, decode + projective pass, the
projective marginals alone (ggnn_projective_marginals with scores) and the
whole MBR chain (decode, marginals, decode of the marginals, projective pass
on their scores) on the same inputs; per line
  decode_ms / decode_proj_ms / proj_ms   as above
  marg_ms          ggnn_projective_marginals alone
  mbr_ms           the MBR chain;  mbr_extra_ms = mbr_ms - decode_ms
  mbr_status       graphs whose marginals' arg-max was a projective tree / was
                   replaced by the MBR tree / without marginals
  host_marg_ms     the fetch + evaluation.projective_marginals_arrays (float64;
                   timed on the first 32 graphs and scaled to the batch)
  marg_err         largest |marg - float64 host form| of the batch
--epoch then scores the dev set with tree="projective" against
tree="projective-mbr" (time, UAS, repaired graphs, fetched bytes).

    python tools/ab_tree_decode.py --tree-marginals [--epoch]

alternates, in one process, the plain decode, decode + MST pass, the
projective marginals, the marginals over all dependency trees
(ggnn_tree_marginals with scores) and the "mbr" chain built on them (decode,
marginals, decode of the marginals, MST pass on their scores) on the same
inputs, and writes its lines to profiles/tree_marginals_ab.jsonl (--out) too;
per line
  decode_ms / decode_tree_ms / tree_ms / marg_ms   as above
  lapl_ms          ggnn_tree_marginals alone
  mbr_ms           the "mbr" chain;  mbr_extra_ms = mbr_ms - decode_ms
  mbr_status       graphs whose marginals' arg-max was a tree / was replaced
                   by the MBR tree / without marginals
  host_lapl_ms     the fetch + evaluation.tree_marginals_arrays (float64, the
                   first 32 graphs, scaled to the batch)
  lapl_err, lapl_err_over_bar   largest |marg - float64 host form| of those
                   graphs, and against n * cond * 2^-24
--epoch then scores the dev set with tree=True against tree="mbr" (time, UAS,
repaired and infeasible graphs, fetched bytes) and parses it with tree="mbr"
and with tree=True, confidence="nonprojective".

    python tools/ab_tree_decode.py --tree-sample

alternates, in one process, ggnn_tree_marginals (the yardstick: one inversion
per graph) and ggnn_tree_sample at K = 1, 4 and 16 samples per graph on the
marginals' outputs, and times the float64 host form
(evaluation.tree_sample_arrays, K = 1, the first 8 graphs, scaled to the
batch); writes its lines to profiles/tree_sample_ab.jsonl (--out) too; per line
  lapl_ms          ggnn_tree_marginals (without scores)
  sample_k1_ms / sample_k4_ms / sample_k16_ms   ggnn_tree_sample alone
  sample_k*_per_round   the sampler's time per round of workgroups (b * K over
                   the device's compute units) over the marginals' own
  host_sample_ms   the fetch + the host form, K = 1
  differ, samples  the K = 4 samples of the first 8 graphs that are not the
                   float64 host form's trees (all explained: asserted)
  log_prob_err     the largest |log_prob - float64| of those samples

    python tools/ab_tree_decode.py --projective-sample

alternates, in one process, ggnn_projective_marginals (the yardstick: the
sampler runs its inside passes and leaves the outside pass out) and
ggnn_projective_sample at K = 1, 4, 16 and 64 samples per graph, flat regime,
median of 5 windows, and times the float64 host form
(evaluation.projective_sample_arrays, K = 1, the first 8 graphs, scaled to the
batch); writes its lines to profiles/proj_sample_ab.jsonl (--out) too; per line
  chunk            GGNN_PROJ_SAMPLE_CHUNK of the library that ran
  marg_ms          ggnn_projective_marginals (without scores)
  sample_k1_ms / sample_k4_ms / sample_k16_ms / sample_k64_ms   the sampler alone
  k1_not_slower    sample_k1_ms <= marg_ms
  host_sample_ms   the fetch + the host form, K = 1
  differ, samples  the K = 4 samples of the first 8 graphs that are not the
                   float64 host form's trees (all explained: asserted)
  log_prob_err     the largest |log_prob - float64| of those samples

    python tools/ab_tree_decode.py --projective-kbest

alternates, in one process, ggnn_projective_decode on a pred without heads (the
yardstick: its pass runs on every graph and fills the 1-best tables) and
ggnn_projective_kbest at K = 1, 4 and 16, flat regime, median of 5 windows, and
times the host form (evaluation.projective_kbest_arrays, K = 4, the first 8
graphs, scaled to the batch); writes its lines to profiles/proj_kbest_ab.jsonl
(--out) too; per line
  lds_maxn         ggnn_projective_kbest_lds_maxn(K) of the library that ran
  decode_ms        the reset of pred + ggnn_projective_decode
  kbest_k1_ms / kbest_k4_ms / kbest_k16_ms   ggnn_projective_kbest alone
  host_kbest_k4_ms the host form, K = 4 (its outputs equal the kernel's bit for
                   bit, and rank 0 is the decode's tree: asserted)
  trees            the trees the K = 4 launch returned
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(b, v, o, oe, regime, seed):
    rng = np.random.default_rng(seed)
    n = rng.integers(v // 2, v + 1, b).astype(np.int32)
    ph = np.zeros((b, v, o), np.float32)
    for g in range(b):
        k = int(n[g])
        logits = rng.normal(0, 0.1, (v, k))
        if regime != "flat":
            gold = np.zeros(v, int)
            if regime == "peaked":
                gold[2:k] = [rng.integers(1, i) for i in range(2, k)]     # word 1 is the one ROOT child
            else:                                                     # peaked-projective
                from ggnn_amd.evaluation import random_projective_heads
                gold[1:k] = random_projective_heads(k, rng)[1:]
            logits[np.arange(1, k), gold[1:k]] += np.log(9.0 * (k - 1))
        e = np.exp(logits - logits.max(axis=1, keepdims=True))
        ph[g, :, :k] = e / e.sum(axis=1, keepdims=True)
    pe = rng.random((b, v, oe)).astype(np.float32) + 0.01
    return ph, pe, n


def timed(torch, fn, warmup=5, rounds=5, calls=40):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        z.record()
        z.synchronize()
        ms.append(a.elapsed_time(z) / calls)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def alternated(torch, fns, warmup=5, rounds=5, calls=40):
    """timed() of several paths with their rounds interleaved: (median, min, max) per path."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            z.record()
            z.synchronize()
            ms[k].append(a.elapsed_time(z) / calls)
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in ms]


def kernel_sizes(torch, sizes, projective=False):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    for (b, v, o) in sizes:
        for regime in ("flat", "peaked") + (("peaked-projective",) if projective else ()):
            ph, pe, n = batch(b, v, o, 46, regime, seed=b + v)
            ph_d, pe_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, pe, n))
            scores = tree_scores(ph_d, n_d, v)

            def plain():
                return oh.decode([ph_d, pe_d], n_d)

            def with_tree():
                pred, _, _ = oh.decode([ph_d, pe_d], n_d)
                return pred, oh.tree_decode(scores, n_d, pred)

            out = {"b": b, "v": v, "o": o, "regime": regime}
            out["decode_ms"], out["decode_ms_min"], out["decode_ms_max"] = timed(torch, plain)
            out["decode_tree_ms"], out["decode_tree_ms_min"], out["decode_tree_ms_max"] = timed(torch, with_tree)
            out["scores_ms"] = timed(torch, lambda: tree_scores(ph_d, n_d, v))[0]
            out["tree_ms"] = out["decode_tree_ms"] - out["decode_ms"]
            pred0 = plain()[0]
            pred, status = with_tree()
            torch.cuda.synchronize()
            host_ms = []
            for _ in range(2):
                t = time.perf_counter()
                s_h, n_h, p_h = scores.cpu().numpy(), n_d.cpu().numpy(), pred0.cpu().numpy()
                h_pred, _, h_status = E.tree_decode_arrays(s_h, n_h, p_h, True)
                host_ms.append((time.perf_counter() - t) * 1e3)
            out["host_ms"] = min(host_ms)
            status, pred = status.cpu().numpy(), pred.cpu().numpy()
            assert np.array_equal(status, h_status)
            for g in np.flatnonzero(status == 1):
                assert E.is_tree(pred[g, :, 0], n_h[g], True, s_h[g])
                assert E.tree_total(s_h[g], pred[g, :, 0], n_h[g]) == E.tree_total(s_h[g], h_pred[g, :, 0], n_h[g])
            out["status"] = [int((status == k).sum()) for k in (0, 1, 2)]
            out["device_faster_than_host"] = out["tree_ms"] < out["host_ms"]
            if projective:
                def with_proj():
                    pred, _, _ = oh.decode([ph_d, pe_d], n_d)
                    return pred, oh.projective_decode(scores, n_d, pred)

                calls = 40 if b * v <= 2048 or regime == "peaked-projective" else 10
                (t_plain, t_tree, t_proj) = alternated(torch, [plain, with_tree, with_proj], calls=calls)
                out["decode_ms"], out["decode_ms_min"], out["decode_ms_max"] = t_plain
                out["decode_tree_ms"], out["decode_tree_ms_min"], out["decode_tree_ms_max"] = t_tree
                out["decode_proj_ms"], out["decode_proj_ms_min"], out["decode_proj_ms_max"] = t_proj
                out["tree_ms"] = t_tree[0] - out["decode_ms"]
                out["proj_ms"] = t_proj[0] - out["decode_ms"]
                pred, status = with_proj()
                torch.cuda.synchronize()
                t = time.perf_counter()
                s_h, n_h, p_h = scores.cpu().numpy(), n_d.cpu().numpy(), pred0.cpu().numpy()
                h_pred, _, h_status = E.projective_decode_arrays(s_h, n_h, p_h, True)
                out["host_proj_ms"] = (time.perf_counter() - t) * 1e3
                status, pred = status.cpu().numpy(), pred.cpu().numpy()
                assert np.array_equal(status, h_status)
                changed = 0
                for g in np.flatnonzero(status == 1):
                    assert E.is_tree(pred[g, :, 0], n_h[g], True, s_h[g]) and E.is_projective(pred[g, :, 0], n_h[g])
                    assert E.tree_total(s_h[g], pred[g, :, 0], n_h[g]) == E.tree_total(s_h[g], h_pred[g, :, 0], n_h[g])
                    changed += int((pred[g, 1:n_h[g], 0] != p_h[g, 1:n_h[g], 0]).sum())
                out["proj_status"] = [int((status == k).sum()) for k in (0, 1, 2)]
                out["proj_heads_changed"] = changed
            print(json.dumps(out), flush=True)


def marginals_sizes(torch, sizes):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    for (b, v, o) in sizes:
        for regime in ("flat", "peaked", "peaked-projective"):
            ph, pe, n = batch(b, v, o, 46, regime, seed=b + v)
            ph_d, pe_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, pe, n))
            scores = tree_scores(ph_d, n_d, v)

            def plain():
                return oh.decode([ph_d, pe_d], n_d)

            def with_proj():
                pred, _, _ = oh.decode([ph_d, pe_d], n_d)
                return pred, oh.projective_decode(scores, n_d, pred)

            def marginals():
                return oh.projective_marginals(ph_d, n_d, True)

            def mbr():
                oh.decode([ph_d, pe_d], n_d)
                marg, _, m_scores, m_status = oh.projective_marginals(ph_d, n_d, True)
                pred, _, _ = oh.decode([marg, pe_d], n_d)
                return pred, oh.projective_decode(m_scores, n_d, pred), m_status

            calls = 40 if b * v <= 2048 else 10
            t = alternated(torch, [plain, with_proj, marginals, mbr], calls=calls)
            out = {"b": b, "v": v, "o": o, "regime": regime}
            for key, x in zip(("decode_ms", "decode_proj_ms", "marg_ms", "mbr_ms"), t):
                out[key], out[key + "_min"], out[key + "_max"] = x
            out["proj_ms"] = out["decode_proj_ms"] - out["decode_ms"]
            out["mbr_extra_ms"] = out["mbr_ms"] - out["decode_ms"]
            marg, logz, m_scores, m_status = marginals()
            pred, status, _ = mbr()
            torch.cuda.synchronize()
            tm = time.perf_counter()
            k = min(b, 32)                                            # (the float64 host form: the first 32 graphs)
            h = E.projective_marginals_arrays(ph_d[:k].cpu().numpy(), n_d[:k].cpu().numpy(), True)
            out["host_marg_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
            out["host_marg_graphs"] = k
            assert np.array_equal(m_status[:k].cpu().numpy(), h[3])
            out["marg_err"] = float(np.abs(marg[:k].cpu().numpy().astype(np.float64) - h[0]).max())
            status = np.where(m_status.cpu().numpy() == 1, status.cpu().numpy(), 2)
            out["mbr_status"] = [int((status == k).sum()) for k in (0, 1, 2)]
            print(json.dumps(out), flush=True)


def tree_marginals_sizes(torch, sizes, emit):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    for (b, v, o) in sizes:
        for regime in ("flat", "peaked", "peaked-projective"):
            ph, pe, n = batch(b, v, o, 46, regime, seed=b + v)
            ph_d, pe_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, pe, n))
            scores = tree_scores(ph_d, n_d, v)

            def plain():
                return oh.decode([ph_d, pe_d], n_d)

            def with_tree():
                pred, _, _ = oh.decode([ph_d, pe_d], n_d)
                return pred, oh.tree_decode(scores, n_d, pred)

            def projective():
                return oh.projective_marginals(ph_d, n_d, True)

            def marginals():
                return oh.tree_marginals(ph_d, n_d, True)

            def mbr():
                oh.decode([ph_d, pe_d], n_d)
                marg, _, m_scores, m_status = oh.tree_marginals(ph_d, n_d, True)
                pred, _, _ = oh.decode([marg, pe_d], n_d)
                return pred, oh.tree_decode(m_scores, n_d, pred), m_status, m_scores

            calls = 40 if b * v <= 2048 else 10
            t = alternated(torch, [plain, with_tree, projective, marginals, mbr], calls=calls)
            out = {"b": b, "v": v, "o": o, "regime": regime}
            for key, x in zip(("decode_ms", "decode_tree_ms", "marg_ms", "lapl_ms", "mbr_ms"), t):
                out[key], out[key + "_min"], out[key + "_max"] = x
            out["tree_ms"] = out["decode_tree_ms"] - out["decode_ms"]
            out["mbr_extra_ms"] = out["mbr_ms"] - out["decode_ms"]
            marg, logz, _, m_status = marginals()
            pred, status, _, m_scores = mbr()
            torch.cuda.synchronize()
            tm = time.perf_counter()
            k = min(b, 32)                                            # (the float64 host form: the first 32 graphs)
            n_h = n_d[:k].cpu().numpy()
            h = E.tree_marginals_arrays(ph_d[:k].cpu().numpy(), n_h, True)
            out["host_lapl_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
            out["host_lapl_graphs"] = k
            assert np.array_equal(m_status[:k].cpu().numpy(), h[3])
            err = np.abs(marg[:k].cpu().numpy().astype(np.float64) - h[0]).max(axis=(1, 2))
            out["lapl_err"] = float(err.max())
            out["lapl_err_over_bar"] = float((err / (n_h * h[4] * 2.0 ** -24)).max())
            out["cond_max"] = float(h[4].max())
            s_h, p_h = m_scores[:k].cpu().numpy(), pred[:k].cpu().numpy()
            assert all(E.is_tree(p_h[g, :, 0], n_h[g], True, s_h[g]) for g in range(k))
            status = np.where(m_status.cpu().numpy() == 1, status.cpu().numpy(), 2)
            out["mbr_status"] = [int((status == k).sum()) for k in (0, 1, 2)]
            emit(out)


def tree_sample_sizes(torch, sizes, emit):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    oh = OutputHeads(64)
    for (b, v, o) in sizes:
        for regime in ("flat", "peaked", "peaked-projective"):
            ph, _, n = batch(b, v, o, 46, regime, seed=b + v)
            ph_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, n))
            have = oh.tree_marginals(ph_d, n_d, True, with_scores=False)

            def marginals():
                return oh.tree_marginals(ph_d, n_d, True, with_scores=False)

            def sampler(k):
                return lambda: oh.tree_sample(ph_d, n_d, k, 1, True, have)

            calls = 40 if b * v <= 2048 else 5
            t = alternated(torch, [marginals] + [sampler(k) for k in (1, 4, 16)], calls=calls)
            out = {"b": b, "v": v, "o": o, "regime": regime, "compute_units": cus}
            for key, x in zip(("lapl_ms", "sample_k1_ms", "sample_k4_ms", "sample_k16_ms"), t):
                out[key], out[key + "_min"], out[key + "_max"] = x
            rounds = lambda groups: -(-groups // cus)
            for k in (1, 4, 16):
                out["sample_k%d_per_round" % k] = ((out["sample_k%d_ms" % k] / rounds(b * k))
                                                   / (out["lapl_ms"] / rounds(b)))
            heads, log_prob, status = oh.tree_sample(ph_d, n_d, 4, 1, True, have)
            torch.cuda.synchronize()
            k = min(b, 8)                                             # (the float64 host form: the first 8 graphs)
            n_h = n[:k]
            tm = time.perf_counter()
            E.tree_sample_arrays(ph_d[:k].cpu().numpy(), n_h, 1, 1, True)
            out["host_sample_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
            out["host_sample_graphs"] = k
            h_heads, h_lp, h_status, margin = E.tree_sample_arrays(ph[:k], n_h, 4, 1, True)
            cond = E.tree_marginals_arrays(ph[:k], n_h, True)[4]
            assert np.array_equal(status[:k].cpu().numpy(), h_status)
            got = heads[:k].cpu().numpy()
            diff = (got != h_heads).any(axis=2) & (h_status == 1)
            assert all(margin[g, s] < n_h[g] * cond[g] * 2.0 ** -24 for g, s in np.argwhere(diff))
            same = ~diff & (h_status == 1)
            out["samples"], out["differ"] = int((h_status == 1).sum()), int(diff.sum())
            out["log_prob_err"] = float(np.abs(log_prob[:k].cpu().numpy().astype(np.float64) - h_lp)[same].max())
            emit(out)


def projective_sample_sizes(torch, sizes, emit):
    from ggnn_amd import _lib
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    oh = OutputHeads(64)
    ks = (1, 4, 16, 64)
    for (b, v, o) in sizes:
        ph, _, n = batch(b, v, o, 46, "flat", seed=b + v)
        ph_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, n))

        def marginals():
            return oh.projective_marginals(ph_d, n_d, True, with_scores=False)

        def sampler(k):
            return lambda: oh.projective_sample(ph_d, n_d, k, 1, True)

        calls = 40 if b * v <= 2048 else 5
        t = alternated(torch, [marginals] + [sampler(k) for k in ks], calls=calls)
        out = {"b": b, "v": v, "o": o, "regime": "flat", "compute_units": cus, "chunk": _lib.PROJ_SAMPLE_CHUNK}
        for key, x in zip(["marg_ms"] + ["sample_k%d_ms" % k for k in ks], t):
            out[key], out[key + "_min"], out[key + "_max"] = x
        out["k1_not_slower"] = out["sample_k1_ms"] <= out["marg_ms"]
        heads, log_prob, status, _ = oh.projective_sample(ph_d, n_d, 4, 1, True)
        torch.cuda.synchronize()
        k = min(b, 8)                                                 # (the float64 host form: the first 8 graphs)
        n_h = n[:k]
        tm = time.perf_counter()
        E.projective_sample_arrays(ph_d[:k].cpu().numpy(), n_h, 1, 1, True)
        out["host_sample_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
        out["host_sample_graphs"] = k
        h_heads, h_lp, h_status, margin, _ = E.projective_sample_arrays(ph[:k], n_h, 4, 1, True)
        span_max = E.projective_marginals_arrays(ph[:k], n_h, True)[4]
        assert np.array_equal(status[:k].cpu().numpy(), h_status)
        got = heads[:k].cpu().numpy()
        diff = (got != h_heads).any(axis=2) & (h_status == 1)
        bar = lambda g: 4 * n_h[g] * (np.log2(n_h[g]) + 4 + span_max[g]) * 2.0 ** -24
        assert all(margin[g, s] < bar(g) for g, s in np.argwhere(diff))
        assert all(E.is_projective(got[g, s], n_h[g]) for g, s in np.argwhere(h_status == 1))
        same = ~diff & (h_status == 1)
        out["samples"], out["differ"] = int((h_status == 1).sum()), int(diff.sum())
        out["log_prob_err"] = float(np.abs(log_prob[:k].cpu().numpy().astype(np.float64) - h_lp)[same].max())
        emit(out)


def projective_kbest_sizes(torch, sizes, emit):
    from ggnn_amd import _lib
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    ks = (1, 4, 16)
    for (b, v, o) in sizes:
        ph, _, n = batch(b, v, o, 46, "flat", seed=b + v)
        ph_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, n))
        scores = tree_scores(ph_d, n_d, v)
        pred = torch.empty(b, v, 2, dtype=torch.int32, device=dev)

        def decode():
            pred.fill_(-1)                                            # no tree: the pass runs on every graph
            return oh.projective_decode(scores, n_d, pred)

        def kbest(k):
            return lambda: oh.projective_kbest(scores, n_d, k, True)

        calls = 40 if b * v <= 2048 else 5
        t = alternated(torch, [decode] + [kbest(k) for k in ks], calls=calls)
        out = {"b": b, "v": v, "o": o, "regime": "flat",
               "lds_maxn": {str(k): int(_lib.load().ggnn_projective_kbest_lds_maxn(k)) for k in ks}}
        for key, x in zip(["decode_ms"] + ["kbest_k%d_ms" % k for k in ks], t):
            out[key], out[key + "_min"], out[key + "_max"] = x
        assert (decode().cpu().numpy() == 1).all()
        got = [x.cpu().numpy() for x in kbest(4)()]
        assert np.array_equal(got[0][:, 0], pred.cpu().numpy()[:, :, 0])    # rank 0: the decode's tree
        k = min(b, 8)                                                 # (the host form: the first 8 graphs)
        tm = time.perf_counter()
        ref = E.projective_kbest_arrays(scores[:k].cpu().numpy(), n[:k], 4, True)
        out["host_kbest_k4_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
        out["host_kbest_graphs"] = k
        assert all(np.array_equal(a[:k], c) for a, c in zip(got, ref))       # bit-identical
        out["trees"] = int(got[2].sum())
        emit(out)


def epoch_tree_mbr(torch, emit):
    from ggnn_amd import evaluation as E
    from ggnn_amd.batching import DATA_DIR, TRAIN_WITH_DEV, read_btb_json, wsj_model_sizes
    from ggnn_amd.model import DenseGGNNChemModel
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20,
                                   "compact_adjacency": True}, seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False)
    paths = (("tree", {"tree": True}), ("mbr", {"tree": "mbr"}))
    for _, kw in paths:
        m.score_epoch(data, **kw)                                     # both paths warm
    out = {"what": "score_epoch, 1700 dev sentences, batch 20, untrained model", "tree_s": [], "mbr_s": []}
    for _ in range(3):                                                # alternating
        for key, kw in paths:
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = m.score_epoch(data, **kw)
            torch.cuda.synchronize()
            out[key + "_s"].append(round(time.perf_counter() - t, 4))
            out[key + "_uas"] = r[2]
            out[key + "_stats"] = dict(m.decode_stats)
    emit(out)
    raw = read_btb_json(os.path.join(DATA_DIR, TRAIN_WITH_DEV["train_file"]))
    trees = lambda ps: sum(1 for d, p in zip(raw, ps) if len(p) == len(d["node_features"]) - 1
                           and E.is_tree([-1] + [x[0] for x in p], len(p) + 1, True))
    t = time.perf_counter()
    mbr = m.parse(raw, tree="mbr")
    secs = time.perf_counter() - t
    mst, conf = m.parse(raw, tree=True, confidence="nonprojective")
    flat = [c for cs in conf for c in cs]
    emit({"what": 'parse(dev, tree="mbr") and parse(dev, tree=True, confidence="nonprojective")',
          "sentences": len(raw), "mbr_single_rooted_trees": trees(mbr), "mst_single_rooted_trees": trees(mst),
          "parse_mbr_s": round(secs, 3), "confidences": len(flat), "confidence_min": min(flat),
          "confidence_max": max(flat), "confidence_mean": float(np.mean(flat)),
          "aligned": all(len(c) == len(p) for c, p in zip(conf, mst))})


def epoch_mbr(torch):
    from ggnn_amd.batching import TRAIN_WITH_DEV, wsj_model_sizes
    from ggnn_amd.model import DenseGGNNChemModel
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20,
                                   "compact_adjacency": True}, seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False)
    paths = (("projective", {"tree": "projective"}), ("projective_mbr", {"tree": "projective-mbr"}))
    for _, kw in paths:
        m.score_epoch(data, **kw)                                     # both paths warm
    out = {"what": "score_epoch, 1700 dev sentences, batch 20, untrained model", "projective_s": [],
           "projective_mbr_s": []}
    for _ in range(3):                                                # alternating
        for key, kw in paths:
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = m.score_epoch(data, **kw)
            torch.cuda.synchronize()
            out[key + "_s"].append(round(time.perf_counter() - t, 4))
            out[key + "_uas"] = r[2]
            out[key + "_stats"] = dict(m.decode_stats)
    print(json.dumps(out), flush=True)


def epoch(torch, projective=False):
    from ggnn_amd import evaluation as E
    from ggnn_amd.batching import DATA_DIR, TRAIN_WITH_DEV, read_btb_json, wsj_model_sizes
    from ggnn_amd.model import DenseGGNNChemModel
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 20,
                                   "compact_adjacency": True}, seed=0,
                           embedding_sizes=dict(loc=32, pos=16, word=32, edge=16), **wsj_model_sizes())
    data = m.load_data(TRAIN_WITH_DEV["train_file"], False)
    m.score_epoch(data)
    m.score_epoch(data, tree=True)                                    # both paths warm
    out = {"what": "score_epoch, 1700 dev sentences, batch 20, untrained model", "plain_s": [], "tree_s": []}
    paths = (("plain_s", {}), ("tree_s", {"tree": True}))
    if projective:
        m.score_epoch(data, tree="projective")
        out["projective_s"] = []
        paths += (("projective_s", {"tree": "projective"}),)
    for _ in range(3):                                                # alternating
        for key, kw in paths:
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = m.score_epoch(data, **kw)
            torch.cuda.synchronize()
            out[key].append(round(time.perf_counter() - t, 4))
            out[key[:-2] + "_uas"] = r[2]
            out[key[:-2] + "_stats"] = dict(m.decode_stats)
    print(json.dumps(out), flush=True)
    raw = read_btb_json(os.path.join(DATA_DIR, TRAIN_WITH_DEV["train_file"]))
    t = time.perf_counter()
    parsed = m.parse(raw, tree=True)
    secs = time.perf_counter() - t
    plain = m.parse(raw)
    trees = sum(1 for d, p in zip(raw, parsed)
                if len(p) == len(d["node_features"]) - 1 and E.is_tree([-1] + [x[0] for x in p], len(p) + 1, True))
    plain_trees = sum(1 for d, p in zip(raw, plain)
                      if len(p) == len(d["node_features"]) - 1
                      and E.is_tree([-1] + [x[0] for x in p], len(p) + 1, True))
    print(json.dumps({"what": "parse(dev, tree=True)", "sentences": len(raw), "single_rooted_trees": trees,
                      "arg_max_trees": plain_trees, "parse_tree_s": round(secs, 3)}), flush=True)
    if projective:
        t = time.perf_counter()
        proj = m.parse(raw, tree="projective")
        secs = time.perf_counter() - t
        count = lambda ps: sum(1 for d, p in zip(raw, ps)
                               if len(p) == len(d["node_features"]) - 1
                               and E.is_tree([-1] + [x[0] for x in p], len(p) + 1, True)
                               and E.is_projective([-1] + [x[0] for x in p], len(p) + 1))
        print(json.dumps({"what": 'parse(dev, tree="projective")', "sentences": len(raw),
                          "projective_trees": count(proj), "mst_projective_trees": count(parsed),
                          "arg_max_projective_trees": count(plain), "parse_projective_s": round(secs, 3)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", action="store_true", help="also time score_epoch and check parse on the dev set")
    ap.add_argument("--projective", action="store_true",
                    help="alternate the MST pass with ggnn_projective_decode (and tree=\"projective\" with --epoch)")
    ap.add_argument("--marginals", action="store_true",
                    help="alternate the plain decode, the projective pass, ggnn_projective_marginals and the MBR "
                         "chain (and tree=\"projective\" against tree=\"projective-mbr\" with --epoch)")
    ap.add_argument("--tree-marginals", action="store_true",
                    help="alternate the plain decode, the MST pass, ggnn_projective_marginals, ggnn_tree_marginals "
                         "and the \"mbr\" chain (and tree=True against tree=\"mbr\" with --epoch)")
    ap.add_argument("--tree-sample", action="store_true",
                    help="alternate ggnn_tree_marginals with ggnn_tree_sample at 1, 4 and 16 samples per graph")
    ap.add_argument("--projective-sample", action="store_true",
                    help="alternate ggnn_projective_marginals with ggnn_projective_sample at 1, 4, 16 and 64 samples "
                         "per graph")
    ap.add_argument("--projective-kbest", action="store_true",
                    help="alternate ggnn_projective_decode (its pass made to run) with ggnn_projective_kbest at K = 1, "
                         "4 and 16")
    ap.add_argument("--out", default=None,
                    help="where --tree-marginals / --tree-sample / --projective-sample / --projective-kbest also write "
                         "their lines (default: profiles/tree_marginals_ab.jsonl / tree_sample_ab.jsonl / "
                         "proj_sample_ab.jsonl / proj_kbest_ab.jsonl)")
    ap.add_argument("--sizes", default="20x40x150,256x128x150")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ab_tree_decode.py needs a HIP device"
    head = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    print(json.dumps(head), flush=True)
    sizes = [tuple(int(x) for x in s.split("x")) for s in args.sizes.split(",")]
    if args.tree_marginals or args.tree_sample or args.projective_sample or args.projective_kbest:
        name = ("proj_kbest_ab.jsonl" if args.projective_kbest else "proj_sample_ab.jsonl" if args.projective_sample
                else "tree_sample_ab.jsonl" if args.tree_sample else "tree_marginals_ab.jsonl")
        with open(args.out or os.path.join(ROOT, "profiles", name), "w") as f:
            def emit(line):
                text = json.dumps(line)
                print(text, flush=True)
                f.write(text + "\n")
                f.flush()
            f.write(json.dumps(head) + "\n")
            if args.projective_kbest:
                projective_kbest_sizes(torch, sizes, emit)
                return
            if args.projective_sample:
                projective_sample_sizes(torch, sizes, emit)
                return
            if args.tree_sample:
                tree_sample_sizes(torch, sizes, emit)
                return
            tree_marginals_sizes(torch, sizes, emit)
            if args.epoch:
                epoch_tree_mbr(torch, emit)
        return
    if args.marginals:
        marginals_sizes(torch, sizes)
        if args.epoch:
            epoch_mbr(torch)
        return
    kernel_sizes(torch, sizes, args.projective)
    if args.epoch:
        epoch(torch, args.projective)


if __name__ == "__main__":
    main()
