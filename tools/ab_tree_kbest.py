"""Timing of ggnn_tree_kbest (the K best trees over all dependency trees), HIP
events around warmed-up launches, in the manner of tools/ab_tree_decode.py
(its batches and its alternated windows: median of 5, flat regime).

    python tools/ab_tree_kbest.py

alternates, in one process and per size (b, v, o), ggnn_tree_decode on a pred
without heads (the yardstick: its pass runs on every graph, the cost of one
launch of contractions), ggnn_projective_kbest and ggnn_tree_kbest at every K
of the size, and writes its lines to profiles/tree_kbest_ab.log (--out) too;
per line
  decode_ms        the reset of pred + ggnn_tree_decode
  proj_k<K>_ms     ggnn_projective_kbest alone
  tree_k<K>_ms     ggnn_tree_kbest alone (2 K - 1 launches)
  host_k4_ms       the host form, K = 4, the first 4 graphs, scaled to the batch
                   (its outputs equal the kernel's bit for bit, and rank 0 is
                   the decode's tree: asserted)
  trees            the trees the largest K returned

    python tools/ab_tree_kbest.py --decode-only [--lib PATH]

times ggnn_tree_decode alone (the pass made to run) through the C ABI of the
library at PATH (default: the package's own), for the A/B of the solver's
factoring against a library built from the parent commit: run it several times
per library, alternating, and compare the medians with the spread of the
parent's own runs.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ab_tree_decode import alternated, batch      # noqa: E402

SIZES = ((256, 40, 150, (1, 4, 16)), (256, 128, 150, (16,)), (20, 40, 150, (1, 4, 16)))


def kbest_sizes(torch, emit):
    from ggnn_amd import evaluation as E
    from ggnn_amd.heads import OutputHeads, tree_scores
    dev = torch.device("cuda", 0)
    oh = OutputHeads(64)
    for (b, v, o, ks) in SIZES:
        ph, _, n = batch(b, v, o, 46, "flat", seed=b + v)
        ph_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, n))
        scores = tree_scores(ph_d, n_d, v)
        pred = torch.empty(b, v, 2, dtype=torch.int32, device=dev)

        def decode():
            pred.fill_(-1)                                            # no tree: the pass runs on every graph
            return oh.tree_decode(scores, n_d, pred)

        proj = lambda k: (lambda: oh.projective_kbest(scores, n_d, k, True))
        tree = lambda k: (lambda: oh.tree_kbest(scores, n_d, k, True))
        calls = 20 if b * v <= 2048 else 5
        t = alternated(torch, [decode] + [proj(k) for k in ks] + [tree(k) for k in ks], calls=calls)
        out = {"b": b, "v": v, "o": o, "regime": "flat", "n_mean": float(n.mean())}
        keys = ["decode_ms"] + ["proj_k%d_ms" % k for k in ks] + ["tree_k%d_ms" % k for k in ks]
        for key, x in zip(keys, t):
            out[key], out[key + "_min"], out[key + "_max"] = x
        assert (decode().cpu().numpy() == 1).all()
        got = [x.cpu().numpy() for x in tree(ks[-1])()]
        assert np.array_equal(got[0][:, 0], pred.cpu().numpy()[:, :, 0])    # rank 0: the decode's tree
        k = min(b, 4)                                                 # (the host form: the first 4 graphs)
        got4 = [x[:k].cpu().numpy() for x in tree(4)()]
        tm = time.perf_counter()
        ref = E.tree_kbest_arrays(scores[:k].cpu().numpy(), n[:k], 4, True)
        out["host_k4_ms"] = (time.perf_counter() - tm) * 1e3 * b / k
        out["host_graphs"] = k
        assert all(np.array_equal(a, c) for a, c in zip(got4, ref))          # bit-identical
        out["trees"] = int(got[2].sum())
        emit(out)


def decode_only(torch, path, emit):
    from ggnn_amd import _lib
    from ggnn_amd.heads import tree_scores
    lib = ctypes.CDLL(path or _lib.LIB)
    P = ctypes.c_void_p
    lib.ggnn_tree_decode.restype = ctypes.c_int
    lib.ggnn_tree_decode.argtypes = [ctypes.POINTER(_lib.GGNNDims), P, ctypes.c_int32, P, ctypes.c_int32, P, P, P, P, P,
                                     ctypes.c_size_t, P]
    dev = torch.device("cuda", 0)
    for (b, v, o, _) in SIZES:
        ph, _, n = batch(b, v, o, 46, "flat", seed=b + v)
        ph_d, n_d = (torch.from_numpy(x).to(dev) for x in (ph, n))
        scores = tree_scores(ph_d, n_d, v)
        pred = torch.empty(b, v, 2, dtype=torch.int32, device=dev)
        status = torch.empty(b, dtype=torch.int32, device=dev)
        d = _lib.dims(b, v, 64, 1, 1, True, "fp32")

        def decode():
            pred.fill_(-1)
            rc = lib.ggnn_tree_decode(ctypes.byref(d), scores.data_ptr(), o, n_d.data_ptr(), 1, pred.data_ptr(), None,
                                      None, status.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
            assert rc == 0

        (t,) = alternated(torch, [decode], calls=20 if b * v <= 2048 else 10)
        decode()
        assert (status.cpu().numpy() == 1).all()
        emit({"lib": os.path.basename(path or _lib.LIB), "b": b, "v": v, "o": o, "decode_ms": t[0], "decode_ms_min": t[1],
              "decode_ms_max": t[2], "heads_sum": int(pred[:, :, 0].sum())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode-only", action="store_true", help="time ggnn_tree_decode alone, through the library at --lib")
    ap.add_argument("--lib", default=None, help="the library of --decode-only (default: the package's own)")
    ap.add_argument("--out", default=None, help="where the lines are written too (default: profiles/tree_kbest_ab.log; "
                                                "--decode-only: appended)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "ab_tree_kbest.py needs a HIP device"
    head = {"device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
    with open(args.out or os.path.join(ROOT, "profiles", "tree_kbest_ab.log"), "a" if args.decode_only else "w") as f:
        def emit(line):
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")
            f.flush()
        emit(head)
        if args.decode_only:
            decode_only(torch, args.lib, emit)
        else:
            kbest_sizes(torch, emit)


if __name__ == "__main__":
    main()
