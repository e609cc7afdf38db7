"""GPU parity: the HIP engine (through the C ABI) against the CPU oracle.

Tolerances (north_star: "within 1e-3 fp32 / 1e-2 bf16"):
  * precision="fp32" (GGNN_FP32_PARITY: every non-exact MFMA operand as an f16
    hi/lo limb pair, fp32 accumulation -- the parity mode): against the
    float64 restatement of the reference, forward max|h_gpu - h_ref| <= 1e-3
    and every gradient's max error normalised by its max |ref| <= 1e-3.
  * precision="fp16" (single f16 MFMA operands): normalised RMS error of the
    T-step output <= 1e-2, of every gradient <= 5e-2.
  * precision="bf16" (single bf16 MFMA operands): the engine must reproduce
    the reference math with bf16-rounded operands (oracle
    forward_bf16_operands).  The only allowed differences are fp32
    accumulation order and, through it, rare 1-ulp flips of a bf16-rounded
    operand: for one timestep median |diff| <= 1e-6, mean |diff| <= 1e-5,
    max |diff| <= 1e-2.  Against the float64 reference the normalised RMS
    error of the T-step output must not exceed the emulation's own by more
    than 25 % and stays <= 2e-2 for T <= 3 (bf16's 8-bit mantissa alone gives
    ~1.2e-2 at T = 3 on the SURVEY §8d data, where X reaches rms ~2 and the
    GRU is steep); of every gradient <= 5e-2 (the bf16-rounded forward
    activations enter every backward product -- the fp32 mode is the parity
    mode for gradients).
"""
import json
import os

import numpy as np
import pytest

import ggnn_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
FP16_RMS_TOL = 1e-2
BF16_RMS_TOL = 1e-2
BF16_RMS_CAP = 2e-2
GRADS = ("h0", "edge_weights", "edge_biases", "gates_kernel", "gates_bias", "candidate_kernel", "candidate_bias")


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _case(b, v, h, C, seed, use_bias=True, density=0.1):
    A, h0 = O.synthetic_batch(b, v, h, C, seed=seed, density=density)
    w = O.synthetic_weights(h, C, seed=seed)
    if not use_bias:
        w["edge_biases"] = np.zeros_like(w["edge_biases"])
    return A, h0, w


def _f64(w):
    return {k: x.astype(np.float64) for k, x in w.items()}


def _run(A, h0, w, T, precision, use_bias=True, dhT=None, skip=True, generic=False, unfused=False):
    torch = _torch()
    from ggnn_amd.engine import PropagationEngine
    b, C, v, _ = A.shape
    eng = PropagationEngine(h0.shape[-1], C, use_edge_bias=use_bias, precision=precision, skip_empty_channels=skip,
                            force_generic=generic, unfused_forward=unfused)
    dev = eng.device
    pack = eng.pack_weights({k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in w.items()})
    eng.set_adjacency(torch.from_numpy(np.ascontiguousarray(A)).to(dev))
    out = eng.forward(torch.from_numpy(np.ascontiguousarray(h0)).to(dev), pack, T, training=dhT is not None)
    res = {"hT": out.cpu().numpy()}
    if dhT is not None:
        g = eng.backward(torch.from_numpy(np.ascontiguousarray(dhT)).to(dev))
        res.update({k: (None if t is None else t.cpu().numpy()) for k, t in g.items()})
    torch.cuda.synchronize()
    return res


def _nrms(x, ref):
    return float(np.sqrt(np.mean((x - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))


def _nmax(x, ref):
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-30))


SHAPES = [
    (3, 20, 128, 4, 2),     # ragged v -> padded to 32
    (8, 64, 128, 4, 3),     # config-2 shape (b=32 in full)
    (2, 128, 256, 8, 2),    # config-3 shape, small batch
    (4, 100, 256, 4, 3),    # v -> 128, odd C
    (5, 50, 256, 6, 2),     # v -> 64, N not a multiple of 128
]


@pytest.mark.parametrize("b,v,h,C,T", SHAPES + [(5, 50, 64, 6, 1)])
def test_forward_fp32_parity(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 7 + v)
    ref, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), _f64(w), T, keep_cache=False)
    got = _run(A, h0, w, T, "fp32")["hT"]
    assert np.abs(got - ref).max() <= FP32_TOL


def test_config2_full_batch_forward_fp32_parity():
    """configs[1] exactly as BASELINE.json names it: b = 32 synthetic dense
    graphs, v = 64, hidden 128, e = 2 (C = 4), T = 3, forward only (SURVEY §8d
    generator, seed 0), against the float64 reference at the fp32 bar."""
    b, v, h, C, T = 32, 64, 128, 4, 3
    A, h0 = O.synthetic_batch(b, v, h, C, seed=0)
    w = O.synthetic_weights(h, C, seed=0)
    ref, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), _f64(w), T, keep_cache=False)
    got = _run(A, h0, w, T, "fp32")["hT"]
    assert np.abs(got - ref).max() <= FP32_TOL
    assert _nrms(got, ref) <= 1e-5


def test_fp16_within_1e_2_rms_on_config3_t5():
    """north_star's 16-bit bar on configs[2]'s OWN data (config-3 shape: v = 128,
    hidden 256, C = 8, T = 5, the SURVEY §8d dense synthetic adjacency): the
    GGNN_FP16 mode (single f16 MFMA operands, fp32 accumulation) is within
    1e-2 normalised RMS of the float64 reference on the OUTPUT of
    compute_final_node_representations (the quantity north_star bounds),
    and equal to its own rounding emulation.  (No policy with a bf16 operand
    can be, and no single-limb policy meets 1e-2 in max |err| there:
    tests/test_precision_policies.py.)  The gradients run the same T = 5
    chain backwards through the saturated GRU: measured 2.5-3.0e-2 normalised
    RMS, held to the fp16 mode's 5e-2 gradient bound (the fp32-parity mode is
    the parity mode for gradients)."""
    b, v, h, C, T = 8, 128, 256, 8, 5
    A, h0 = O.synthetic_batch(b, v, h, C, seed=1)
    w = O.synthetic_weights(h, C, seed=1)
    dhT = np.random.default_rng(7).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "fp16", dhT=dhT)
    errs = {"hT_nrms": _nrms(got["hT"], ref), "hT_max": float(np.abs(got["hT"] - ref).max())}
    emu = O.forward_operand_policy(A, h0, w, T, "f16", "f16")
    errs["emulation_hT_nrms"] = _nrms(emu, ref)
    for k in GRADS:
        errs[k] = _nrms(got[k].reshape(gref[k].shape), gref[k])
    print("fp16 at config 3, T = 5:", errs)
    assert errs["hT_nrms"] <= FP16_RMS_TOL
    assert abs(errs["hT_nrms"] - errs["emulation_hT_nrms"]) <= 0.1 * errs["emulation_hT_nrms"]
    for k in GRADS:
        assert errs[k] <= 5 * FP16_RMS_TOL, (k, errs[k])


@pytest.mark.parametrize("b,v,h,C,T", [
    (4, 64, 256, 4, 3),     # v -> 64, N % 128 == 0: the 128-row k_gru_fwd2 outside the fused forward
    (1, 128, 256, 2, 17),   # T > FUSED_MAXT: per-timestep k_prop_fwd + k_gru_fwd2 fallback at config-3 sizes
])
def test_unfused_forward_paths_fp32_parity(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 7 + T)
    dhT = np.random.default_rng(3).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "fp32", dhT=dhT)
    # Long unrolls amplify the split mode's ~2^-22 rounding through the
    # recurrence (measured, fused and per-timestep paths alike: max |err| 5e-5
    # at T = 5, 3.6e-4 at T = 12, 1.0e-3 at T = 16, 1.2e-3 at T = 17; normalised
    # RMS stays < 1e-4): the max-error bound scales with T beyond the
    # reference's T = 4..5
    tol = FP32_TOL if T <= 8 else 4 * FP32_TOL
    assert np.abs(got["hT"] - ref).max() <= tol
    assert _nrms(got["hT"], ref) <= 1e-4
    for k in GRADS:
        assert _nmax(got[k].reshape(gref[k].shape), gref[k]) <= tol, k
    inf = _run(A, h0, w, T, "fp32")  # inference path (no saves)
    assert np.abs(inf["hT"] - ref).max() <= tol


@pytest.mark.parametrize("b,v,h,C,T", SHAPES)
def test_backward_fp32_parity(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 13 + v)
    dhT = np.random.default_rng(5).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    hT, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "fp32", dhT=dhT)
    assert np.abs(got["hT"] - hT).max() <= FP32_TOL
    for k in GRADS:
        assert _nmax(got[k].reshape(gref[k].shape), gref[k]) <= FP32_TOL, k


# The reference's loss is divided by task_target_num = sum(target_mask) + 1e-7
# ~ b (chem_tensorflow.py:360,399-403), so in training dL/dh_T is ~1e-4..1e-6
# per element, not N(0,1): 2^-12 ~ 1/b at b = 4096 targets, 2^-16 deeper still.
# The backward must hold the same 1e-3 bar there (the engine scales the
# backward by an exact power of two, ggnn_common.h gscale).
LOSS_SCALES = [2.0 ** -12, 2.0 ** -16]


@pytest.mark.parametrize("scale", LOSS_SCALES)
@pytest.mark.parametrize("b,v,h,C,T", [(2, 128, 256, 8, 5), (5, 50, 256, 6, 2), (3, 20, 128, 4, 2)])
def test_backward_fp32_parity_at_loss_scale(b, v, h, C, T, scale):
    A, h0, w = _case(b, v, h, C, seed=b * 17 + v)
    dhT = (np.random.default_rng(6).standard_normal((b, v, h)) * scale).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    hT, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "fp32", dhT=dhT)
    for k in GRADS:
        assert _nmax(got[k].reshape(gref[k].shape), gref[k]) <= FP32_TOL, (k, _nmax(got[k].reshape(gref[k].shape),
                                                                                     gref[k]))


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_backward_16bit_at_loss_scale(precision):
    """The 16-bit modes keep their statistical bound at loss-scale gradients
    (f16 alone would flush 2^-16-sized operands to subnormals)."""
    b, v, h, C, T = 4, 64, 256, 8, 3
    A, h0, w = _case(b, v, h, C, seed=21)
    dhT = (np.random.default_rng(4).standard_normal((b, v, h)) * 2.0 ** -16).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    hT, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, precision, dhT=dhT)
    for k in GRADS:
        assert _nrms(got[k].reshape(gref[k].shape), gref[k]) <= 5 * FP16_RMS_TOL, k


def test_full_config3_backward_at_loss_scale():
    """Config 3 at full size (b=256, v=128, h=256, C=8, T=5) with dL/dh_T at the
    btb loss's scale: each sampled graph's dL/dh0 equals the oracle's for that
    graph alone, and the weight gradients are linear over graphs."""
    b, v, h, C, T = 256, 128, 256, 8, 5
    A, h0, w = _case(b, v, h, C, seed=2)
    dhT = (np.random.default_rng(12).standard_normal((b, v, h)) * 2.0 ** -14).astype(np.float32)
    full = _run(A, h0, w, T, "fp32", dhT=dhT)
    w64 = _f64(w)
    for gi in (0, 131, 255):
        A64 = A[gi:gi + 1].astype(np.float64)
        _, caches = O.forward(A64, h0[gi:gi + 1].astype(np.float64), w64, T)
        gref = O.backward(A64, dhT[gi:gi + 1].astype(np.float64), caches, w64)
        assert _nmax(full["h0"][gi:gi + 1], gref["h0"]) <= FP32_TOL, gi
    h1 = _run(A[:128], h0[:128], w, T, "fp32", dhT=dhT[:128])
    h2 = _run(A[128:], h0[128:], w, T, "fp32", dhT=dhT[128:])
    for k in GRADS[1:]:
        assert _nmax(full[k], h1[k] + h2[k]) <= 1e-5, k


@pytest.mark.timeout(400)
@pytest.mark.parametrize("dropout", [False, True])
def test_full_config3_all_gradients_vs_float64_oracle(dropout):
    """The bench's own workload, configs[2] at full size (b = 256, v = 128,
    h = 256, C = 8, T = 5): h_T and ALL SEVEN gradients of the whole batch
    against the float64 oracle run over the whole batch -- the weight
    gradients sum 256 x 128 x 5 rows of single-f16-operand products (k_wgrad256:
    per-chunk partial tiles summed in chunk order by k_wgrad_reduce, no
    atomics), which the per-graph checks above do not reach.
    dropout=False: once with N(0,1) dL/dh_T and once with the same dL/dh_T
    at the btb loss's scale 2^-14 (a power of two, so the oracle's gradients
    scale exactly; the engine picks another backward gscale).  dropout=True:
    the reference's training feed, keep 0.9 for edge weights and GRU state
    (chem_tensorflow_dense.py:860-861), the same Philox seed on both sides.
    Bar: max |err| / max |ref| <= 1e-3 (FP32_TOL), per gradient.
    References: chem_tensorflow.py:496; chem_tensorflow_dense.py:391-437."""
    b, v, h, C, T = 256, 128, 256, 8, 5
    A, h0, w = _case(b, v, h, C, seed=4)
    dhT = np.random.default_rng(14).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    dr = dict(edge_keep=0.9, state_keep=0.9, seed=0x5EED_0004) if dropout else None
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T, dropout=dr)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    del caches
    errs = {}
    for scale in ((1.0,) if dropout else (1.0, 2.0 ** -14)):
        d = (dhT * np.float32(scale)).astype(np.float32)
        got = _run_dropout(A, h0, w, T, "fp32", dr, d) if dropout else _run(A, h0, w, T, "fp32", dhT=d)
        e = {"hT": float(np.abs(got["hT"] - ref).max())}
        for k in GRADS:
            e[k] = _nmax(got[k].reshape(gref[k].shape), scale * gref[k])
        errs[scale] = e
        del got
    print("config 3 full batch, dropout=%s:" % dropout, errs)
    for scale, e in errs.items():
        assert e["hT"] <= FP32_TOL, (scale, e)
        for k in GRADS:
            assert e[k] <= FP32_TOL, (scale, k, e)


@pytest.mark.parametrize("dropout", [False, True])
def test_backward_hi_weight_limbs_long_unroll(dropout):
    """round 5 gave k_gru_bwd (Wc^T / Wg^T) and k_prop_bwd (W_c^T)
    the weights' hi f16 limb only (7.7e-4 measured at config 3, T = 5); since
    round 6 both take their limb corrections on the fp8 MFMA.
    The error compounds over timesteps, so the bar is checked beyond the
    reference's T = 4..5 and its hidden 256 at T = 8 -- the longest unroll
    DESIGN claims 1e-3 for -- with N(0,1) and loss-scale dL/dh_T and with the
    training dropout, every gradient at max |err| / max |ref| <= 1e-3.
    References: chem_tensorflow_dense.py:237-241,333,391-437; chem_tensorflow.py:496."""
    b, v, h, C, T = 8, 128, 256, 8, 8
    A, h0, w = _case(b, v, h, C, seed=31)
    dhT = np.random.default_rng(15).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    dr = dict(edge_keep=0.9, state_keep=0.9, seed=0x5EED_0008) if dropout else None
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T, dropout=dr)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    errs = {}
    for scale in (1.0, 2.0 ** -14):
        d = (dhT * np.float32(scale)).astype(np.float32)
        got = _run_dropout(A, h0, w, T, "fp32", dr, d) if dropout else _run(A, h0, w, T, "fp32", dhT=d)
        e = {"hT": float(np.abs(got["hT"] - ref).max())}
        for k in GRADS:
            e[k] = _nmax(got[k].reshape(gref[k].shape), scale * gref[k])
        errs[scale] = e
    print("T = 8, hidden 256, dropout=%s:" % dropout, errs)
    for scale, e in errs.items():
        assert e["hT"] <= FP32_TOL, (scale, e)
        for k in GRADS:
            assert e[k] <= FP32_TOL, (scale, k, e)


def test_backward_fp8_corrections_on_round5_worst_case():
    """Round 6: the split-mode backward's limb corrections run on the block-scaled
    fp8 MFMA (k_prop_bwd: dM W_c^T; k_gru_bwd: f16 dz x f16 W + e5m2 dz x e4m3
    W_lo).  Seed 5 at T = 8 is the input where the oracle's
    emulation puts round 5's hi-only k_gru_bwd weights at 1.01e-3 of the 1e-3
    bar and the shipped fp8 form at 5.4e-4 (tests/test_precision_policies.py):
    the GPU must hold every gradient within 1e-3 of float64 there, and within
    1.5x of the emulated policy's own error.
    References: chem_tensorflow_dense.py:237-241,333,391-437; chem_tensorflow.py:496."""
    b, v, h, C, T = 8, 128, 256, 8, 8
    A, h0, w = _case(b, v, h, C, seed=5)
    dhT = np.random.default_rng(105).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    emu = O.backward_operand_policy(A64, dhT.astype(np.float64), caches, w64, "f16x2", "f8lo", "f8corr", "f16")
    got = _run(A, h0, w, T, "fp32", dhT=dhT)
    e = {k: _nmax(got[k].reshape(gref[k].shape), gref[k]) for k in GRADS}
    e_emu = max(_nmax(emu[k], gref[k]) for k in GRADS)
    print("seed 5, T = 8: GPU", e, "emulated policy max %.3g" % e_emu)
    for k in GRADS:
        assert e[k] <= FP32_TOL, (k, e)
    assert max(e.values()) <= 1.5 * e_emu + 1e-4, (e, e_emu)


@pytest.mark.parametrize("b,v,h,C,T", SHAPES)
def test_forward_bf16_matches_rounding_emulation(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 7 + v)
    emu = O.forward_bf16_operands(A, h0, w, T)
    ref, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), _f64(w), T, keep_cache=False)
    got = _run(A, h0, w, T, "bf16")["hT"]
    assert _nrms(got, ref) <= min(BF16_RMS_CAP, 1.25 * _nrms(emu, ref))
    assert _nrms(got, emu) <= _nrms(got, ref)     # the rounding model explains the error
    emu1 = O.forward_bf16_operands(A, h0, w, 1)
    d1 = np.abs(_run(A, h0, w, 1, "bf16")["hT"] - emu1)
    assert np.median(d1) <= 1e-6 and d1.mean() <= 1e-5 and d1.max() <= 1e-2, (np.median(d1), d1.mean(), d1.max())


@pytest.mark.parametrize("b,v,h,C,T", SHAPES[:4])
def test_backward_bf16_statistical(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 13 + v)
    dhT = np.random.default_rng(5).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    hT, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "bf16", dhT=dhT)
    for k in GRADS:
        assert _nrms(got[k].reshape(gref[k].shape), gref[k]) <= 5 * BF16_RMS_TOL, k


@pytest.mark.parametrize("b,v,h,C,T", SHAPES[:4])
def test_fp16_statistical(b, v, h, C, T):
    A, h0, w = _case(b, v, h, C, seed=b * 13 + v)
    dhT = np.random.default_rng(5).standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    hT, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "fp16", dhT=dhT)
    assert _nrms(got["hT"], hT) <= FP16_RMS_TOL
    for k in GRADS:
        assert _nrms(got[k].reshape(gref[k].shape), gref[k]) <= 5 * FP16_RMS_TOL, k


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_no_edge_bias(precision):
    A, h0, w = _case(3, 40, 128, 4, seed=11, use_bias=False)
    dhT = np.random.default_rng(2).standard_normal(h0.shape).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, 2, use_edge_bias=False)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64, use_edge_bias=False)
    got = _run(A, h0, w, 2, precision, use_bias=False, dhT=dhT)
    tol = FP32_TOL if precision == "fp32" else 5 * BF16_RMS_TOL
    metric = _nmax if precision == "fp32" else _nrms
    assert metric(got["hT"], ref) <= tol
    assert got["edge_biases"] is None
    for k in ("h0", "edge_weights", "gates_kernel", "candidate_kernel"):
        assert metric(got[k].reshape(gref[k].shape), gref[k]) <= tol, k


def test_edge_cases_isolated_and_tiny():
    # all-zero adjacency: X = 0 (no neighbour sends, beta not added), h' = GRU(0, h)
    b, v, h, C, T = 3, 7, 128, 4, 2
    A = np.zeros((b, C, v, v), np.float32)
    _, h0, w = _case(b, v, h, C, seed=1)
    ref, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), _f64(w), T, keep_cache=False)
    assert np.abs(_run(A, h0, w, T, "fp32")["hT"] - ref).max() <= FP32_TOL
    # one graph with one node and a self loop, v = 1
    A1 = np.ones((1, C, 1, 1), np.float32)
    h1 = np.full((1, 1, h), 0.1, np.float32)
    ref1, _ = O.forward(A1.astype(np.float64), h1.astype(np.float64), _f64(w), 3, keep_cache=False)
    assert np.abs(_run(A1, h1, w, 3, "fp32")["hT"] - ref1).max() <= FP32_TOL


def test_full_config3_batch_properties():
    """Config 3 (b=256, v=128, h=256, C=8, T=5) at full size: graphs are
    independent, so each sampled graph of the full-batch run must equal the
    oracle on that graph alone; the weight gradients of the full batch must
    equal the sum of the two half batches' (linearity over graphs)."""
    b, v, h, C, T = 256, 128, 256, 8, 5
    A, h0, w = _case(b, v, h, C, seed=1)
    dhT = np.random.default_rng(3).standard_normal((b, v, h)).astype(np.float32)
    full = _run(A, h0, w, T, "fp32", dhT=dhT)
    for gi in (0, 77, 255):
        ref, _ = O.forward(A[gi:gi + 1].astype(np.float64), h0[gi:gi + 1].astype(np.float64), _f64(w), T,
                           keep_cache=False)
        assert np.abs(full["hT"][gi:gi + 1] - ref).max() <= FP32_TOL
    h1 = _run(A[:128], h0[:128], w, T, "fp32", dhT=dhT[:128])
    h2 = _run(A[128:], h0[128:], w, T, "fp32", dhT=dhT[128:])
    assert np.array_equal(full["hT"][:128], h1["hT"]) and np.array_equal(full["hT"][128:], h2["hT"])
    for k in GRADS[1:]:
        assert _nmax(full[k], h1[k] + h2[k]) <= 1e-5, k
    np.testing.assert_array_equal(full["h0"][:128], h1["h0"])


def test_forward_is_deterministic():
    A, h0, w = _case(16, 128, 256, 8, seed=9)
    a = _run(A, h0, w, 3, "bf16")["hT"]
    b_ = _run(A, h0, w, 3, "bf16")["hT"]
    assert np.array_equal(a, b_)


def test_errors_are_raised_not_ignored():
    torch = _torch()
    from ggnn_amd import _lib
    from ggnn_amd.engine import PropagationEngine
    eng = PropagationEngine(128, 4)
    with pytest.raises(RuntimeError):
        eng.forward(torch.zeros((2, 8, 128), device=eng.device), None, 1)
    with pytest.raises(ValueError):
        eng.set_adjacency(torch.zeros((2, 3, 8, 8), device=eng.device))
    with pytest.raises(_lib.GGNNError):      # hidden outside 1..4096
        PropagationEngine(5000, 4).dims(1, 1, 1)
    with pytest.raises(_lib.GGNNError):      # C > 4096
        PropagationEngine(128, 5000).dims(1, 1, 1)
    with pytest.raises(_lib.GGNNError):
        eng.dims(0, 20, 1)
    PropagationEngine(100, 4).dims(1, 1, 1)  # any other hidden size / v: the general path
    eng.dims(1, 200, 1)


@pytest.mark.parametrize("hidden", [128, 400])
def test_drop_in_model_on_reference_dev_batches(hidden):
    """DenseGGNNChemModel fed with real WSJ dev minibatches (golden fixture of
    the reference's own data, C = 2*46 = 92 channels): forward and autograd
    backward against the oracle, fp32 mode; hidden 128 on the specialised
    kernels, the reference's default 400 on the general path."""
    torch = _torch()
    from ggnn_amd.model import DenseGGNNChemModel
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batching_golden.npz"))
    data = json.loads(str(g["raw_json"]))
    m = DenseGGNNChemModel(params={"hidden_size": hidden, "num_timesteps": 3, "batch_size": 8},
                           num_edge_types=int(g["num_edge_types"]), output_size_edges=int(g["output_size_edges"]),
                           pos_size=int(g["pos_size"]), bucket_max_nodes=int(g["bucket_max_nodes"]),
                           precision="fp32")
    feeds = list(m.make_minibatch_iterator(m.process_raw_graphs(data[:24], False), False))
    w64 = {"edge_weights": m.weights["edge_weights"].detach().cpu().numpy().astype(np.float64),
           "edge_biases": m.weights["edge_biases"].detach().cpu().numpy().astype(np.float64)}
    w64.update({k: t.detach().cpu().numpy().astype(np.float64) for k, t in m.weights["node_gru"].items()})
    rng = np.random.default_rng(0)
    for fd in feeds[:3]:
        m.feed(fd)
        b, v = fd["num_graphs"], fd["num_vertices"]
        h0 = rng.uniform(-0.5, 0.5, (b, v, hidden)).astype(np.float32)
        h0_t = torch.from_numpy(h0).to(m.device).requires_grad_(True)
        out = m.compute_final_node_representations(h0_t)
        A64 = np.asarray(fd["adjacency_matrix"], np.float64)
        ref, caches = O.forward(A64, h0.astype(np.float64), w64, 3)
        assert np.abs(out.detach().cpu().numpy() - ref).max() <= FP32_TOL
        dhT = rng.standard_normal(out.shape).astype(np.float32)
        for p in m.parameters():
            p.grad = None
        out.backward(torch.from_numpy(dhT).to(m.device))
        gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
        assert _nmax(h0_t.grad.cpu().numpy(), gref["h0"]) <= FP32_TOL
        assert _nmax(m.weights["edge_weights"].grad.cpu().numpy(), gref["edge_weights"]) <= FP32_TOL
        assert _nmax(m.weights["node_gru"]["gates_kernel"].grad.cpu().numpy(), gref["gates_kernel"]) <= FP32_TOL


def test_old_ordering_served_by_engine():
    """--old (compute_timestep_normal, chem_tensorflow_dense.py:350-389) runs
    through the engine and matches the oracle's per-channel summation order;
    --pr identity is refused."""
    torch = _torch()
    from ggnn_amd.model import DenseGGNNChemModel
    b, v, h, C, T = 3, 40, 128, 4, 3
    A, h0 = O.synthetic_batch(b, v, h, C, seed=7, density=0.1)
    m = DenseGGNNChemModel(args={"--pr": "btb", "--old": True},
                           params={"hidden_size": h, "num_timesteps": T, "batch_size": b},
                           num_edge_types=C // 2, precision="fp32", seed=3)
    w64 = {"edge_weights": m.weights["edge_weights"].detach().cpu().numpy().astype(np.float64),
           "edge_biases": m.weights["edge_biases"].detach().cpu().numpy().astype(np.float64)}
    w64.update({k: t.detach().cpu().numpy().astype(np.float64) for k, t in m.weights["node_gru"].items()})
    m.feed({"adjacency_matrix": A, "num_graphs": b, "num_vertices": v})
    out = m.compute_final_node_representations(torch.from_numpy(h0).to(m.device))
    ref, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), w64, T, ordering="old", keep_cache=False)
    assert np.abs(out.detach().cpu().numpy() - ref).max() <= FP32_TOL
    # compute_timestep_normal ignores fixed_ts's weight choice: the fixed_ts=1
    # call of make_model (chem_tensorflow.py:321-322) still uses edge_weights
    # (chem_tensorflow_dense.py:342-370), only T changes
    out1 = m.compute_final_node_representations(torch.from_numpy(h0).to(m.device), fixed_ts=1)
    ref1, _ = O.forward(A.astype(np.float64), h0.astype(np.float64), w64, 1, ordering="old", keep_cache=False)
    assert np.abs(out1.detach().cpu().numpy() - ref1).max() <= FP32_TOL
    m2 = DenseGGNNChemModel(args={"--pr": "identity"}, params={"hidden_size": h, "num_timesteps": T},
                            num_edge_types=C // 2, precision="fp32", seed=3)
    m2.feed({"adjacency_matrix": A, "num_graphs": b, "num_vertices": v})
    with pytest.raises(NotImplementedError):
        m2.compute_final_node_representations(torch.from_numpy(h0).to(m2.device))


# ------------------------------------------------------------------ dropout
@pytest.mark.parametrize("b,v,h,C,T,t", [(3, 21, 128, 4, 3, 0), (2, 128, 256, 8, 5, 4), (5, 50, 64, 6, 2, 1)])
def test_dropout_masks_bit_exact(b, v, h, C, T, t):
    """The keep-masks the kernels apply equal the oracle's Philox restatement
    bit for bit (integer work: exact)."""
    _torch()
    from ggnn_amd.engine import PropagationEngine
    eng = PropagationEngine(h, C, precision="fp32")
    seed = 0x1234_5678_9ABC + t
    for keep in (0.9, 0.5):
        me = eng.dropout_mask("edge", b, v, T, t, keep, seed).cpu().numpy().astype(bool)
        assert np.array_equal(me, O.edge_keep_mask(C, h, t, keep, seed))
        ms = eng.dropout_mask("state", b, v, T, t, keep, seed).cpu().numpy().astype(bool)
        assert np.array_equal(ms, O.state_keep_mask(b, v, h, t, keep, seed))
    assert eng.dropout_mask("state", b, v, T, t, 1.0, seed).cpu().numpy().all()


def _run_dropout(A, h0, w, T, precision, dr, dhT, generic=False):
    torch = _torch()
    from ggnn_amd.engine import PropagationEngine
    b, C, v, _ = A.shape
    eng = PropagationEngine(h0.shape[-1], C, precision=precision, force_generic=generic)
    dev = eng.device
    pack = eng.pack_weights({k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in w.items()},
                            T=T, edge_keep=dr["edge_keep"], seed=dr["seed"])
    eng.set_adjacency(torch.from_numpy(np.ascontiguousarray(A)).to(dev))
    out = eng.forward(torch.from_numpy(np.ascontiguousarray(h0)).to(dev), pack, T, training=True,
                      state_keep=dr["state_keep"])
    g = eng.backward(torch.from_numpy(np.ascontiguousarray(dhT)).to(dev))
    res = {"hT": out.cpu().numpy()}
    res.update({k: (None if x is None else x.cpu().numpy()) for k, x in g.items()})
    return res


@pytest.mark.parametrize("b,v,h,C,T,ek,sk", [
    (3, 20, 128, 4, 3, 0.9, 0.9),      # the reference's training feed (keep 0.9 for both, :860-861)
    (2, 128, 256, 8, 3, 0.9, 0.9),
    (4, 50, 256, 6, 2, 1.0, 0.7),      # state dropout only
    (4, 50, 128, 6, 2, 0.6, 1.0),      # edge dropout only
    # round 6: the fused forward's state keep bits read by the backward -- v = 100
    # (padded to 128: dL/dh_T staged by k_pad_state's own draws, k_prop_bwd
    # reading the bits) and v = 128 state dropout only (dL/dh_T read in place,
    # k_gru_bwd applying the last timestep's bits)
    (3, 100, 256, 4, 3, 0.9, 0.8),
    (2, 128, 256, 4, 4, 1.0, 0.7),
])
def test_dropout_fp32_parity(b, v, h, C, T, ek, sk):
    A, h0, w = _case(b, v, h, C, seed=b * 3 + v)
    dhT = np.random.default_rng(8).standard_normal((b, v, h)).astype(np.float32)
    dr = dict(edge_keep=ek, state_keep=sk, seed=987654321 + T)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T, dropout=dr)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run_dropout(A, h0, w, T, "fp32", dr, dhT)
    assert np.abs(got["hT"] - ref).max() <= FP32_TOL
    for k in GRADS:
        assert _nmax(got[k].reshape(gref[k].shape), gref[k]) <= FP32_TOL, k
    # dropout is really on: the same step without it differs by O(1)
    nodrop, _ = O.forward(A64, h0.astype(np.float64), w64, T, keep_cache=False)
    assert np.abs(nodrop - ref).max() > 0.05


def test_dropout_bf16_statistical():
    b, v, h, C, T = 4, 64, 256, 8, 3
    A, h0, w = _case(b, v, h, C, seed=5)
    dhT = np.random.default_rng(9).standard_normal((b, v, h)).astype(np.float32)
    dr = dict(edge_keep=0.9, state_keep=0.9, seed=42)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T, dropout=dr)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run_dropout(A, h0, w, T, "bf16", dr, dhT)
    assert _nrms(got["hT"], ref) <= BF16_RMS_CAP
    for k in GRADS:
        assert _nrms(got[k].reshape(gref[k].shape), gref[k]) <= 5 * BF16_RMS_TOL, k


def test_drop_in_model_training_feed_applies_dropout():
    """make_minibatch_iterator(is_training=True) feeds keep = 0.9 for both
    dropouts (chem_tensorflow_dense.py:860-861): the model's output must equal
    the oracle with the Philox masks of the seed it drew."""
    torch = _torch()
    from ggnn_amd.model import DenseGGNNChemModel
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batching_golden.npz"))
    data = json.loads(str(g["raw_json"]))
    m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 8},
                           num_edge_types=int(g["num_edge_types"]), output_size_edges=int(g["output_size_edges"]),
                           pos_size=int(g["pos_size"]), bucket_max_nodes=int(g["bucket_max_nodes"]),
                           precision="fp32")
    fd = next(iter(m.make_minibatch_iterator(m.process_raw_graphs(data[:16], True), True)))
    assert fd["graph_state_keep_prob"] == 0.9 and fd["edge_weight_dropout_keep_prob"] == 0.9
    m.feed(fd)
    b, v = fd["num_graphs"], fd["num_vertices"]
    h0 = np.random.default_rng(1).uniform(-0.5, 0.5, (b, v, 128)).astype(np.float32)
    out = m.compute_final_node_representations(torch.from_numpy(h0).to(m.device))
    w64 = {"edge_weights": m.weights["edge_weights"].detach().cpu().numpy().astype(np.float64),
           "edge_biases": m.weights["edge_biases"].detach().cpu().numpy().astype(np.float64)}
    w64.update({k: t.detach().cpu().numpy().astype(np.float64) for k, t in m.weights["node_gru"].items()})
    ref, _ = O.forward(np.asarray(fd["adjacency_matrix"], np.float64), h0.astype(np.float64), w64, 2,
                       keep_cache=False, dropout=m.last_dropout)
    assert np.abs(out.detach().cpu().numpy() - ref).max() <= FP32_TOL


# ------------------------------------------------- compact adjacency producer
def _random_graphs(rng, b, v, E, n_edges):
    gs = []
    for _ in range(b):
        n = int(rng.integers(0, n_edges + 1))
        src = rng.integers(0, v, n)
        dst = rng.integers(0, v, n)          # includes dest = 0 (prev-word edge wraps to v-1, as numpy does)
        lab = rng.integers(1, E + 1, n)
        g = np.stack([src, lab, dst], 1).tolist()
        if n > 1:
            g.append(g[0])                   # a duplicate edge
        gs.append(g)
    return gs


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("b,v,E", [(3, 20, 2), (3, 32, 2), (4, 64, 4), (2, 128, 4), (5, 50, 46)])
def test_adjacency_from_edges_is_byte_identical(b, v, E, precision):
    """ggnn_set_adjacency_edges stages exactly the bytes that ggnn_set_adjacency
    stages from the reference's dense graph_to_adj_mat_bd feed."""
    torch = _torch()
    from ggnn_amd.engine import PropagationEngine
    rng = np.random.default_rng(b * 100 + v + E)
    graphs = _random_graphs(rng, b, v, E, 3 * v)
    A = np.stack([O.graph_to_adj_mat_bd(g, v, E) for g in graphs]).astype(np.float32)
    eng = PropagationEngine(128, 2 * E, precision=precision)
    eng.set_adjacency(torch.from_numpy(A).to(eng.device))
    dense = eng._adj.clone()
    eng.set_adjacency_edges(graphs, v, E)
    assert torch.equal(eng._adj[:dense.numel()], dense)


def test_adjacency_from_edges_on_reference_dev_graphs():
    """Real WSJ dev sentences (golden fixture, E = 46): the edge path feeds the
    same forward as the reference's dense adjacency."""
    torch = _torch()
    from ggnn_amd.engine import PropagationEngine
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batching_golden.npz"))
    data = json.loads(str(g["raw_json"]))
    E, v = int(g["num_edge_types"]), 64
    graphs = [d["graph"] for d in data[:12] if max(max(e[0], e[2]) for e in d["graph"]) < v]
    A = np.stack([O.graph_to_adj_mat_bd(gr, v, E) for gr in graphs]).astype(np.float32)
    eng = PropagationEngine(128, 2 * E, precision="fp32")
    w = O.synthetic_weights(128, 2 * E, seed=4)
    pack = eng.pack_weights({k: torch.from_numpy(np.ascontiguousarray(x)).to(eng.device) for k, x in w.items()})
    h0 = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (len(graphs), v, 128)).astype(np.float32))
    h0 = h0.to(eng.device)
    eng.set_adjacency(torch.from_numpy(A).to(eng.device))
    a = eng.forward(h0, pack, 2).cpu().numpy()
    eng.set_adjacency_edges(graphs, v, E)
    b_ = eng.forward(h0, pack, 2).cpu().numpy()
    assert np.array_equal(a, b_)


def test_adjacency_from_edges_rejects_out_of_range():
    _torch()
    from ggnn_amd.engine import PropagationEngine
    eng = PropagationEngine(128, 4)
    with pytest.raises(IndexError):
        eng.set_adjacency_edges([[[0, 3, 1]]], 8, 2)     # label 3 > E
    with pytest.raises(IndexError):
        eng.set_adjacency_edges([[[0, 1, 8]]], 8, 2)     # node 8 >= v


def test_drop_in_model_compact_adjacency_feed():
    """params['compact_adjacency']: batches carry edge lists only and the model
    stages them on the device; outputs equal the dense-feed model's."""
    torch = _torch()
    from ggnn_amd.model import DenseGGNNChemModel
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "batching_golden.npz"))
    data = json.loads(str(g["raw_json"]))
    outs = []
    for compact in (False, True):
        m = DenseGGNNChemModel(params={"hidden_size": 128, "num_timesteps": 2, "batch_size": 8,
                                       "compact_adjacency": compact},
                               num_edge_types=int(g["num_edge_types"]), output_size_edges=int(g["output_size_edges"]),
                               pos_size=int(g["pos_size"]), bucket_max_nodes=int(g["bucket_max_nodes"]),
                               precision="fp32", seed=3)
        fd = next(iter(m.make_minibatch_iterator(m.process_raw_graphs(data[:16], False), False)))
        assert (fd["adjacency_matrix"] is None) == compact
        m.feed(fd)
        h0 = np.random.default_rng(1).uniform(-0.5, 0.5, (fd["num_graphs"], fd["num_vertices"], 128))
        outs.append(m.compute_final_node_representations(torch.from_numpy(h0.astype(np.float32)).to(m.device))
                    .detach().cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------ optimizer
def test_clip_adam_matches_tf1_semantics():
    """ggnn_adam_step: tf.clip_by_norm per tensor + TF1 Adam, 3 steps, against
    the float64 oracle (chem_tensorflow.py:494-503)."""
    torch = _torch()
    from ggnn_amd.dist import grad_shapes
    from ggnn_amd.optim import ClipAdam
    rng = np.random.default_rng(0)
    shapes = list(grad_shapes(128, 4).values())
    p0 = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in shapes]
    dev = torch.device("cuda", 0)
    params = [torch.from_numpy(x.copy()).to(dev) for x in p0]
    opt = ClipAdam(params, learning_rate=0.003, clamp_gradient_norm=1.0)
    ref_p = [x.astype(np.float64) for x in p0]
    ref_m = [np.zeros_like(x) for x in ref_p]
    ref_v = [np.zeros_like(x) for x in ref_p]
    for t in range(1, 4):
        # tensor norms on both sides of the clip (small biases stay unclipped)
        grads = [rng.standard_normal(s).astype(np.float32) * (0.01 if len(s) == 1 else 0.5) for s in shapes]
        opt.step([torch.from_numpy(g).to(dev) for g in grads], grad_scale=0.5)
        O.adam_step(ref_p, grads, ref_m, ref_v, t, lr=0.003, clip_norm=1.0, grad_scale=0.5)
    torch.cuda.synchronize()
    for got, ref in zip(params, ref_p):
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-6


def test_edge_dropout_long_unroll_packs_in_several_launches():
    """T = 12 timesteps under edge dropout: 2T + 7 pack jobs exceed one launch's
    job table; the packs must still be the per-timestep masked weights."""
    A, h0, w = _case(2, 20, 128, 4, seed=31)
    dhT = np.random.default_rng(2).standard_normal(h0.shape).astype(np.float32)
    dr = dict(edge_keep=0.8, state_keep=1.0, seed=77)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, 12, dropout=dr)
    got = _run_dropout(A, h0, w, 12, "fp32", dr, dhT)
    assert np.abs(got["hT"] - ref).max() <= FP32_TOL


def _tree_adjacency(b, v, E, seed, zipf=False, first_empty=True):
    """Dependency-tree-shaped graphs (graph_to_adj_mat_bd, chem_tensorflow_dense.py:65-83)
    with E labels: most of the 2E channels of a graph are empty, as in the real
    btb data (~30-38 of 92 non-empty).  zipf: label k drawn with
    P ~ 1/k (a few labels dominate a treebank).  first_empty: graph 0 has no
    edge at all."""
    rng = np.random.default_rng(seed)
    A = np.zeros((b, 2 * E, v, v), np.float32)
    pz = 1.0 / np.arange(1, E + 1)
    pz /= pz.sum()
    for g in range(1 if first_empty else 0, b):
        n = int(rng.integers(v // 2, v + 1))
        lab = (lambda: int(rng.choice(E, p=pz)) + 1) if zipf else (lambda: int(rng.integers(1, E + 1)))
        edges = [(int(rng.integers(0, i)), lab(), i) for i in range(1, n)]
        A[g] = O.graph_to_adj_mat_bd(edges, v, E, dtype=np.float32)
    return A


@pytest.mark.parametrize("b,v,h,E,T,precision", [
    (4, 50, 256, 46, 3, "fp32"),     # real-data C = 92, v -> 64: k_prop_fwd / k_prop_bwd
    (3, 120, 256, 46, 2, "fp32"),    # v -> 128, hidden 256: the fused forward
    (4, 30, 128, 13, 2, "fp32"),     # nivre->std label set (C = 26), v -> 32
    (3, 120, 256, 46, 2, "bf16"),
])
def test_empty_channel_skipping_is_bit_identical(b, v, h, E, T, precision):
    """the engine runs MT + AGG only over each graph's
    non-empty channels (k_chan_list); an empty A_c contributes exactly zero, so
    h_T and dL/dh0 (atomic-free chains) must equal the dense channel loop's bit
    for bit.  The weight gradients are summed over graphs / row chunks with fp32
    atomics (k_wgrad256 split-K, k_sum_graphs), whose order varies from run to
    run, so they are held to 1e-6 of each other; the fp32 mode must match the
    oracle."""
    C = 2 * E
    A = _tree_adjacency(b, v, E, seed=b + v)
    assert (A.reshape(b, C, -1).max(-1) > 0).sum(1).max() < C  # some channels really are empty
    rng = np.random.default_rng(v)
    h0 = rng.uniform(-0.2, 0.2, (b, v, h)).astype(np.float32)
    w = O.synthetic_weights(h, C, seed=E)
    dhT = (rng.standard_normal((b, v, h)) * 2.0 ** -10).astype(np.float32)
    skip = _run(A, h0, w, T, precision, dhT=dhT, skip=True)
    dense = _run(A, h0, w, T, precision, dhT=dhT, skip=False)
    for k in ("hT", "h0"):
        assert np.array_equal(skip[k], dense[k]), k
    for k in GRADS[1:]:
        assert _nmax(skip[k], dense[k]) <= 1e-6, (k, _nmax(skip[k], dense[k]))
    if precision == "fp32":
        A64, w64 = A.astype(np.float64), _f64(w)
        ref, caches = O.forward(A64, h0.astype(np.float64), w64, T)
        gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
        assert np.abs(skip["hT"] - ref).max() <= FP32_TOL
        for k in GRADS:
            assert _nmax(skip[k].reshape(gref[k].shape), gref[k]) <= FP32_TOL, k


@pytest.mark.parametrize("v,parity_bias", [(30, False), (30, True), (100, False)])
def test_bf16_within_north_star_on_dependency_trees(v, parity_bias):
    """north_star: bf16 outputs within 1e-2 of the reference.  On the graphs the
    reference trains on (dependency trees, E = 46 labels -> C = 92 channels,
    in-degree ~2 per node) the bf16 mode meets it as written, forward and
    gradients, at T = 5.  (On SURVEY §8d's dense Bernoulli(0.1) synthetic
    adjacency, in-degree ~100, X reaches rms ~2 and the GRU saturates: there
    rounding the WEIGHTS alone to bf16 moves the float64 output by 3.9e-2
    normalised RMS at T = 5 (oracle emulation), so no bf16-weight kernel can be
    within 1e-2; test_forward_bf16_matches_rounding_emulation pins the engine
    to that emulation instead.)"""
    b, h, E, T = 8, 256, 46, 5
    C = 2 * E
    A = _tree_adjacency(b, v, E, seed=v + int(parity_bias), zipf=True, first_empty=False)
    rng = np.random.default_rng(v)
    h0 = rng.uniform(-0.2, 0.2, (b, v, h)).astype(np.float32)
    w = O.synthetic_weights(h, C, seed=3, parity_bias=parity_bias)
    dhT = rng.standard_normal((b, v, h)).astype(np.float32)
    A64, w64 = A.astype(np.float64), _f64(w)
    ref, caches = O.forward(A64, h0.astype(np.float64), w64, T)
    gref = O.backward(A64, dhT.astype(np.float64), caches, w64)
    got = _run(A, h0, w, T, "bf16", dhT=dhT)
    errs = {"hT_nrms": _nrms(got["hT"], ref), "hT_max": float(np.abs(got["hT"] - ref).max())}
    for k in GRADS:
        errs[k] = _nrms(got[k].reshape(gref[k].shape), gref[k])
    print("bf16 on dependency trees:", errs)
    assert errs["hT_nrms"] <= BF16_RMS_TOL and errs["hT_max"] <= BF16_RMS_TOL
    for k in GRADS:
        assert errs[k] <= BF16_RMS_TOL, (k, errs[k])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_forward_16bit_matches_unfused(precision):
    """k_fwd_fused in the single-limb modes (one launch for all T timesteps,
    h in LDS) against the per-timestep k_prop_fwd + k_gru_fwd launches: the
    same rounding points (h, M, X, r*h), so they differ only through fp32
    accumulation order (and the rare 1-ulp flips of a 16-bit operand it
    causes).  One timestep on the dense synthetic data; T = 5 with the
    backward on dependency-tree graphs (the dense synthetic data amplifies a
    flip through the saturated GRU, see test_bf16_within_north_star_...)."""
    b, v, h, C, T = 3, 128, 256, 8, 1
    A, h0, w = _case(b, v, h, C, seed=41)
    fu = _run(A, h0, w, T, precision)["hT"]
    un = _run(A, h0, w, T, precision, unfused=True)["hT"]
    d = np.abs(fu - un)
    assert np.median(d) <= 1e-6 and d.mean() <= 1e-5 and d.max() <= 1e-2, (np.median(d), d.mean(), d.max())
    E, T = 46, 5
    A = _tree_adjacency(b, v, E, seed=5, zipf=True, first_empty=False)
    rng = np.random.default_rng(9)
    h0 = rng.uniform(-0.2, 0.2, (b, v, h)).astype(np.float32)
    w = O.synthetic_weights(h, 2 * E, seed=2)
    dhT = rng.standard_normal((b, v, h)).astype(np.float32)
    fu = _run(A, h0, w, T, precision, dhT=dhT)
    un = _run(A, h0, w, T, precision, dhT=dhT, unfused=True)
    # (bf16's own error vs float64 here is ~4e-3: a half-ulp-scale difference)
    assert _nrms(fu["hT"], un["hT"]) <= 5e-3, _nrms(fu["hT"], un["hT"])
    for k in GRADS:
        assert _nrms(fu[k], un[k]) <= 1e-2, (k, _nrms(fu[k], un[k]))
    inf = _run(A, h0, w, T, precision)   # inference workspace
    assert _nrms(inf["hT"], fu["hT"]) <= 5e-3


@pytest.mark.parametrize("b,v,h,C,T,keep,precision", [
    (8, 128, 256, 8, 3, 1.0, "fp32"),     # k_wgrad256 (256 x 256 tiles), graph-listed dW_c
    (8, 128, 256, 8, 3, 0.9, "fp32"),     # edge dropout: timestep-aligned dW chunks, masked in k_wgrad_reduce
    (3, 64, 256, 4, 2, 0.9, "fp32"),      # N % 128 != 0 at hidden 256: k_wgrad (128 x 128 tiles)
    (6, 64, 128, 4, 3, 1.0, "fp32"),      # hidden 128: k_wgrad
    (8, 128, 256, 8, 2, 1.0, "bf16"),
])
def test_backward_is_deterministic(b, v, h, C, T, keep, precision):
    """The specialised path's backward is bit-reproducible (round 5, VERDICT
    r4 item 4): the weight gradients' K chunks are summed in chunk order
    (k_wgrad_reduce), the GRU and edge biases' per-(timestep, workgroup /
    graph) partials in row order (k_sum_rows) -- no fp32 atomics whose order
    depends on the schedule.  Two engines, same inputs: every gradient equal
    bit for bit."""
    A, h0, w = _case(b, v, h, C, seed=b + v + h)
    dhT = np.random.default_rng(9).standard_normal((b, v, h)).astype(np.float32)
    dr = dict(edge_keep=keep, state_keep=keep, seed=4242)
    r1 = _run_dropout(A, h0, w, T, precision, dr, dhT)
    r2 = _run_dropout(A, h0, w, T, precision, dr, dhT)
    for k in ("hT",) + GRADS:
        assert np.array_equal(r1[k], r2[k]), k
