"""A/B timing of the config-3 training step (bench.py's step without the side
lines): engine variants alternate in one process, so box-to-box clock
differences cancel.  Prints one JSON line per variant and round with the clean
step time and the HIP-event kernel breakdown.

    python tools/ab_step.py --variants skip,dense --rounds 3
    GGNN_LIB=other.so python tools/ab_step.py ...   (a library build A/B: two runs)

Variants: skip (channel skipping, the default engine), dense
(skip_empty_channels=False), keepXX (training dropout at keep 0.XX), ekXX /
stXX (edge-weight / state dropout alone at keep 0.XX).

--structured-loss {nonprojective,projective}: every variant runs three times
per round: as it is, (name + "+marginals") with the family's marginal kernel
alone after the backward (the yardstick) and (name + "+tree_loss") with
ggnn_tree_loss there, on fixed head probabilities [b, v, 150] (the softmax of
N(0, 2^2) logits) and the graphs' own heads as gold (--trees; a chain
otherwise; multi-root, the random trees have several ROOT children;
projective: a random projective tree of the graph's size, the random trees
cross): what params['structured_loss'] adds to a step, all three alternating
in one process.  A first line says how many graphs the loss used.

--structured-loss {nonprojective-margin,projective-margin} (--margin, default
1.0): every variant runs three times per round: as it is, (name +
"+tree_loss") with the likelihood loss of the same family (the yardstick) and
(name + "+margin_loss") with ggnn_margin_loss there, on the same inputs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="skip,dense")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trees", action="store_true", help="b=256 dependency trees, v=30, C=92 (real density)")
    ap.add_argument("--reference", action="store_true",
                    help="with --trees: the reference's model (hidden 400, T = 4), edge lists staged once, pair mode")
    ap.add_argument("--batch", type=int, default=256, help="graphs per batch (20: run_epoch's batch_size)")
    ap.add_argument("--structured-loss", default=None,
                    choices=("nonprojective", "projective", "nonprojective-margin", "projective-margin"),
                    help="also time every variant with ggnn_tree_loss / ggnn_margin_loss of this family in the step")
    ap.add_argument("--margin", type=float, default=1.0, help="the margin kinds' cost of a wrong head")
    args = ap.parse_args()
    kind = args.structured_loss
    margin = bool(kind) and kind.endswith("-margin")
    if margin:
        args.structured_loss = kind[:-len("-margin")]      # the family, as the likelihood loss names it
    import torch
    from ggnn_amd import _lib
    from ggnn_amd.dist import GRAD_ORDER, FlatGradients
    from ggnn_amd.engine import PropagationEngine
    from ggnn_amd.evaluation import random_projective_heads
    from ggnn_amd.heads import OutputHeads
    from ggnn_amd.optim import ClipAdam
    import ggnn_oracle as O

    dev = torch.device("cuda", 0)
    b, v, h, C, T = args.batch, 128, 256, 8, 5
    if args.reference:
        args.trees, h, T = True, 400, 4
    graphs = None
    if args.trees:
        v, C = 30, 92
        rng = np.random.default_rng(13)
        E = C // 2
        pz = 1.0 / np.arange(1, E + 1)
        pz /= pz.sum()
        A = np.zeros((b, C, v, v), np.float32)
        graphs = []
        for g in range(b):
            n = int(rng.integers(v // 2, v + 1))
            ed = [(int(rng.integers(0, i)), int(rng.choice(E, p=pz)) + 1, i) for i in range(1, n)]
            graphs.append(ed)
            A[g] = O.graph_to_adj_mat_bd(ed, v, E, dtype=np.float32)
        h0 = rng.uniform(-0.2, 0.2, (b, v, h)).astype(np.float32)
    else:
        A, h0 = O.synthetic_batch(b, v, h, C, seed=1)
    w = O.synthetic_weights(h, C, seed=1)
    A_d, h0_d = torch.from_numpy(A).to(dev), torch.from_numpy(h0).to(dev)
    w_d = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in w.items()}
    dhT = torch.from_numpy(np.random.default_rng(7).standard_normal((b, v, h)).astype(np.float32)).to(dev)
    opt = ClipAdam([w_d[k] for k in GRAD_ORDER], learning_rate=0.003)

    tl = None
    if args.structured_loss:
        # the heads' side of the step: fixed probabilities, the graphs' heads as gold
        o = 150
        rng_h = np.random.default_rng(29)
        z = rng_h.normal(0.0, 2.0, (b, v, o))
        p = np.exp(z - z.max(axis=2, keepdims=True))
        p = (p / p.sum(axis=2, keepdims=True)).astype(np.float32)
        y = np.zeros((b, v, o), np.float32)
        nn = np.full(b, v, np.int32)
        for g in range(b):
            ed = graphs[g] if graphs is not None else [(i - 1, 1, i) for i in range(1, v)]
            nn[g] = len(ed) + 1
            if args.structured_loss == "projective":    # (the random trees cross: a random projective tree instead)
                ed = [(hd, 1, i) for i, hd in enumerate(random_projective_heads(nn[g], rng_h)) if i]
            for src, _, dst in ed:
                y[g, dst, src] = 1.0
        oh = OutputHeads(h)
        tl = dict(oh=oh, p=torch.from_numpy(p).to(dev), y=torch.from_numpy(y).to(dev),
                  n=torch.from_numpy(nn).to(dev), loss=torch.zeros(2, device=dev), tn=float(nn.sum() - b))

    def make(variant, extra=None):
        keep = 1.0
        ekeep = skeep = None     # edge / state keep when they differ (variants ekXX, stXX)
        kw = {}
        if variant == "dense":
            kw["skip_empty_channels"] = False
        elif variant.startswith("keep"):
            keep = float("0." + variant[4:])
        elif variant.startswith("ek"):
            ekeep, skeep = float("0." + variant[2:]), 1.0
        elif variant.startswith("st"):
            ekeep, skeep = 1.0, float("0." + variant[2:])
        eng = PropagationEngine(h, C, device=dev, **kw)
        if args.reference:
            eng.set_adjacency_edges(graphs, v, C // 2)      # once, as bench.py's real-density lines
        grads = FlatGradients(h, C, True, device=dev)
        gv = dict(grads.views)
        gv["h0"] = torch.empty((b, v, h), device=dev)
        out = torch.empty((b, v, h), device=dev)
        n = [0]

        def step():
            n[0] += 1
            ek = keep if ekeep is None else ekeep
            sk = keep if skeep is None else skeep
            pack = eng.pack_weights(w_d, T=T, edge_keep=ek, seed=n[0])
            if not args.reference:
                eng.set_adjacency(A_d)
            eng.forward(h0_d, pack, T, training=True, out=out, state_keep=sk)
            eng.backward(dhT, gv)
            opt.step([grads.views[k] for k in GRAD_ORDER])
            if extra == "tree_loss":
                tl["oh"].tree_loss(tl["p"], tl["y"], tl["n"], args.structured_loss, False, tl["tn"], tl["loss"])
            elif extra == "margin_loss":
                tl["oh"].margin_loss(tl["p"], tl["y"], tl["n"], args.structured_loss, False, tl["tn"], tl["loss"],
                                     args.margin)
            elif extra == "marginals":      # the family's marginal kernel alone: the yardstick of the two new launches
                run = tl["oh"].projective_marginals if args.structured_loss == "projective" else tl["oh"].tree_marginals
                run(tl["p"], tl["n"], False, with_scores=False)
        return step

    steps = {}
    for vn in args.variants.split(","):
        steps[vn] = make(vn)
        if tl is not None and not margin:
            steps[vn + "+marginals"] = make(vn, "marginals")
        if tl is not None:
            steps[vn + "+tree_loss"] = make(vn, "tree_loss")
        if margin:
            steps[vn + "+margin_loss"] = make(vn, "margin_loss")
    if tl is not None:
        used = tl["oh"].tree_loss(tl["p"], tl["y"], tl["n"], args.structured_loss, False, tl["tn"], tl["loss"])[3]
        first = {"structured_loss": kind, "b": b, "v": v, "o": 150, "used_graphs": int(used.sum().item())}
        if margin:
            out = tl["oh"].margin_loss(tl["p"], tl["y"], tl["n"], args.structured_loss, False, tl["tn"], tl["loss"],
                                       args.margin)
            first.update(margin=args.margin, margin_used_graphs=int(out[5].sum().item()),
                         margin_active_graphs=int((out[2] > 0).sum().item()),
                         margin_hamming=int(out[3].sum().item()))
        print(json.dumps(first), flush=True)
    for r in range(args.rounds):
        for vn, step in steps.items():
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            timer = _lib.KernelTimer(max_launches=200 * args.steps)
            with timer:
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
            br = {k: round(timer.total_ms[k] / args.steps, 4) for k in timer.total_ms if timer.launches.get(k)}
            print(json.dumps({"variant": vn, "round": r, "ms_per_step": round(dt * 1e3, 4), "kernels": br,
                              "lib": os.environ.get("GGNN_LIB", "ggnn_amd/libggnn.so"), "trees": args.trees}),
                  flush=True)


if __name__ == "__main__":
    main()
