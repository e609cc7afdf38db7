"""What the decode tests share (test_gpu_decode.py, test_gpu_tree_decode.py,
test_gpu_projective_decode.py, test_gpu_projective_marginals.py and the CPU
files beside them): the GPU guard, the small synthetic model and treebank, the
staged batch's device scores and the bytes score_epoch may fetch."""
import numpy as np
import pytest


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _synthetic_model(graphs, hidden=64, device=None, seed=0, **params):
    """hidden 64: the general path; 128: the specialised kernels and the
    fused forward (the embedding concat is 16 + 16 + 8 + 24 wide).
    device="cpu": the same variables, seeds and feeds on a machine without a
    GPU (no step can run there).  seed: of the initial variables and of the
    Philox seeds the model draws."""
    from ggnn_amd.model import DenseGGNNChemModel
    return DenseGGNNChemModel(params={"hidden_size": hidden, "num_timesteps": 2, "batch_size": 5,
                                      "compact_adjacency": True, "hip_graphs": graphs, **params},
                              num_edge_types=6, output_size_edges=12, pos_size=46, vocab_size=200, max_nodes=40,
                              seed=seed, device=device, embedding_sizes=dict(loc=16, pos=8, word=24, edge=16))


def _synthetic_raw():
    from ggnn_amd.batching import synthetic_treebank
    return synthetic_treebank(23, num_edge_types=6, output_size_edges=12, pos_size=46, vocab_size=200, max_nodes=40,
                              seed=2)


def _device_scores(m, n_nodes, v):
    """tree_scores of the probabilities the model holds for the batch it just ran."""
    import torch
    from ggnn_amd.heads import tree_scores
    b, o = len(n_nodes), m.params["output_size"]
    probs = m.ops["computed_values"].detach().reshape(b, v, o)
    return tree_scores(probs, torch.from_numpy(np.asarray(n_nodes)).to(probs.device), v).cpu().numpy()


def _batch_bytes(m, data, per_graph):
    return sum(4 + 4 * per_graph * int(f["num_graphs"]) for f in m.make_minibatch_iterator(data, False))
