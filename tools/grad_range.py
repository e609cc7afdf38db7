"""How wide is dL/dh_T's range within a real batch?  

The backward runs on S * dL/dh_T with one power of two S per batch
(ggnn_common.h gscale); a graph whose gradient lies 2^-12 or more below the
batch's largest one loses f16 limb bits (tests/test_slice_inputs.py,
test_single_scale_range_limit).  This measures, on the CPU with the float64
oracle alone, the per-graph max |dL/dh_T| relative to the batch's maximum for
a randomly initialised model of the reference's default size (hidden 400,
T = 4, C = 92) on the first sentences of the dev set, batched as the reference
batches them (buckets of similar length, 20 sentences).

    python tools/grad_range.py [--sentences 100] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import ggnn_oracle as O  # noqa: E402
from ggnn_amd.batching import DATA_DIR, TRAIN_WITH_DEV, read_btb_json, wsj_model_sizes  # noqa: E402
from ggnn_amd.model import DenseGGNNChemModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    sz = wsj_model_sizes()
    m = DenseGGNNChemModel(params={"random_seed": a.seed}, device="cpu", **sz)
    raw = read_btb_json(os.path.join(DATA_DIR, TRAIN_WITH_DEV["train_file"]))[:a.sentences]
    W = m.weights
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    h, T = m.params["hidden_size"], m.params["num_timesteps"]
    o, oe = m.params["output_size"], m.output_size_edges
    w64 = {"edge_weights": f64(W["edge_weights"]), "edge_biases": f64(W["edge_biases"])}
    w64.update({k: f64(t) for k, t in W["node_gru"].items()})
    segs = [(f64(W["loc_embeddings"]), 0), (f64(W["pos_embeddings"]), 1), (f64(W["word_embeddings"]), 2),
            (f64(W["loc_embeddings"]), 3)]
    g0, ge = W["regression_gate_task0"], W["regression_gate_task_edges0"]
    ratios, batches = [], 0
    for fd in m.make_minibatch_iterator(m.process_raw_graphs(raw, False), False):
        b, v = fd["num_graphs"], fd["num_vertices"]
        A = np.asarray(fd["adjacency_matrix"], np.float64)
        h0 = O.embed_forward(segs, np.asarray(fd["word_inputs"]), h)
        hT, _ = O.forward(A, h0, w64, T, keep_cache=False)
        heads = [dict(W=f64(g0["weights"][0]), b=f64(g0["biases"][0]),
                      labels=np.asarray(fd["target_values_head"], np.float64).reshape(b, v, o)),
                 dict(W=f64(ge["weights"][0]), b=f64(ge["biases"][0]),
                      labels=np.asarray(fd["target_values_edges"], np.float64).reshape(b, v, oe))]
        tn = float(np.asarray(fd["target_mask"])[0].sum()) + O.SMALL_NUMBER
        probs, _ = O.heads_forward(hT, h0, heads, target_num=tn)
        _, _, dhT, _ = O.heads_backward(hT, h0, heads, probs, target_num=tn)
        per_graph = np.abs(dhT).max(axis=(1, 2))
        zero_rows = int((np.abs(dhT).max(axis=2) == 0).sum())
        r = per_graph / per_graph.max()
        ratios += r.tolist()
        batches += 1
        print("batch %2d: b = %2d, v = %3d, max |dL/dh_T| %.3e (S = 2^%d), quietest graph 2^%.2f of it, "
              "%d of %d rows exactly 0" % (batches, b, v, per_graph.max(), -int(np.floor(np.log2(per_graph.max()))),
                                           np.log2(r.min()), zero_rows, b * v))
    ratios = np.array(ratios)
    print("%d sentences in %d batches: smallest per-graph max |dL/dh_T| / batch max = %.4f = 2^%.2f; median 2^%.2f"
          % (len(ratios), batches, ratios.min(), np.log2(ratios.min()), np.log2(np.median(ratios))))


if __name__ == "__main__":
    main()
