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
        if regime == "peaked":
            gold = np.zeros(v, int)
            gold[2:k] = [rng.integers(1, i) for i in range(2, k)]     # word 1 is the one ROOT child
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


def kernel_sizes(torch, sizes):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    for (b, v, o) in sizes:
        for regime in ("flat", "peaked"):
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
            print(json.dumps(out), flush=True)


def epoch(torch):
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
    for _ in range(3):                                                # alternating
        for key, kw in (("plain_s", {}), ("tree_s", {"tree": True})):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", action="store_true", help="also time score_epoch and check parse on the dev set")
    ap.add_argument("--sizes", default="20x40x150,256x128x150")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ab_tree_decode.py needs a HIP device"
    print(json.dumps({"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}), flush=True)
    kernel_sizes(torch, [tuple(int(x) for x in s.split("x")) for s in args.sizes.split(",")])
    if args.epoch:
        epoch(torch)


if __name__ == "__main__":
    main()
