"""k_prop_bwd's phase b (dh += dM_c W_c^T) in the fp32-parity mode: A_{c+1}'s
LDS-DMA is issued right after S1 from inline asm (the compiler then counts its
vmcnt waits for the W_c^T fragments, vmcnt(3) / vmcnt(2) / vmcnt(2), instead of
draining to 0 at the top of every k-block) and is waited for by hand, vmcnt(0)
after the k loop, before S2 publishes the tile; the last k-block is peeled and
loads no fragment for a block that does not exist; one dword of every 128-byte
line of A_{c+1} is loaded at the top of channel c (an L2 touch, its value
unused).  The dM-image fragments are read from LDS as before: there is NO
read-ahead ring (one was built and measured no gain,
profiles/prop_bwd_phase_b_ab.log).  A stale or half-staged A tile, a fragment
consumed before it landed, or a touch past the tile shows in dL/dh0 and,
through the next step's dM, in every gradient.

Shapes: the smallest at which those paths differ, b = 4, C = 4, T = 2.
fp32-parity at every (V, H), V in {32, 64, 128}, H in {128, 256}: V = 32 is one
row tile per k-block and touches 16 lines with one partial wave, H = 128 is
four k-blocks (start-up and the peeled block are half the loop).  fp16 / bf16
at (32, 128) and (128, 256): their phase b (b_pipeline, compiler-visible DMA)
is exactly as it was.  Dropout (state_keep = edge_keep = 0.9) at (128, 256) and
(32, 128) fp32 against the oracle run with the same masks (the saved keep bits'
lane mapping in the epilogue, the masked W_c^T fragments).

Graphs of every batch: 0 has every channel occupied; 1 has a single edge (one
non-empty channel: the channel loop runs once and nothing is staged or touched
for a next channel); 2 has no edge at all (the channel loop does not run and
dL/dh passes through unchanged: the dispatcher does not treat such a batch
specially, the kernel's channel list is empty for that graph); 3 has every
channel occupied and its dL/dh_T scaled by 2^-6.  Every buffer the step writes
is filled with 0xFF first (the runner of tests/test_gpu_engine_edges.py).

Bars, those of tests/test_gpu_slice_parity.py: every slice (a graph's dL/dh0,
a channel's dW_c and dbeta_c, the blocks of the GRU's gradients) within 1e-3 of
its own maximum against the float64 oracle and within 1.5 x the emulated
operand policy's error + 1e-4; the 16-bit modes at a normalised RMS error of
EE.GRAD_RMS_TOL per slice; what the oracle has at exactly 0 is exactly 0.
Every case runs twice on fresh engines and the runs must agree bit for bit.
The seed is the first whose emulated per-slice error is at most 6e-4 at every
shape and in both dropout cases (test_emulated_policy_within_bar, on the CPU;
as in tests/slice_cases.py).  SEED_NOTE below records the rejected seed.

Measured on an MI355X: the module runs in 3.2 s (32 tests, 8 of them on the
CPU); worst fp32 slice 4.65e-4 (v 32, hidden 256, candidate_kernel[x]; the
emulation has 4.64e-4 there), with dropout 4.34e-4 (v 128, hidden 256,
candidate_kernel[x]; emulated 4.10e-4); the 16-bit modes' worst slices have a
normalised RMS error of 3.96e-3 (fp16, v 128, hidden 256, edge_biases[3]) and
2.70e-2 (bf16, v 128, hidden 256, gates_bias[u]).
"""
import functools

import numpy as np
import pytest

import engine_edge_cases as EC
import ggnn_oracle as O
import slice_cases as SC
import test_gpu_engine_edges as EE

B, C, T = 4, 4, 2
SEED = 1
SEED_NOTE = "seed 0: 6.6e-4 at v 128, hidden 128 (gates_kernel[x,r]); seed 1: 4.6e-4 at most (v 32, hidden 256)"
QUIET = 2.0 ** -6
EMU_BAR = 6e-4
SHAPES = [(v, h) for v in (32, 64, 128) for h in (128, 256)]
BIT16 = [(32, 128), (128, 256)]
DROP = [(128, 256), (32, 128)]
KEEP = 0.9


def _case(v, h, drop):
    k = KEEP if drop else 1.0
    return SC.Case("pb_v%d_h%d%s" % (v, h, "_drop" if drop else ""), B, v, h, C, T, k, k, SEED, "dense", True, False, 1.0, 0)


@functools.lru_cache(maxsize=None)
def _inputs(v, h):
    rng = np.random.default_rng(5200 + 7 * v + h + SEED)
    A = (rng.random((B, C, v, v)) < SC.DENSITY).astype(np.float32)
    for g in (0, 3):                                # every channel occupied
        for c in range(C):
            A[g, c, int(rng.integers(v)), int(rng.integers(v))] = 1.0
    A[1] = 0.0                                      # a single edge
    A[1, 2, int(rng.integers(v)), int(rng.integers(v))] = 1.0
    A[2] = 0.0                                      # no edge at all
    h0 = rng.uniform(-0.2, 0.2, (B, v, h)).astype(np.float32)
    w = O.synthetic_weights(h, C, seed=5200 + SEED)
    dhT = rng.standard_normal((B, v, h)).astype(np.float32)
    dhT[3] *= np.float32(QUIET)
    for x in (A, h0, dhT) + tuple(w.values()):
        x.setflags(write=False)
    return dict(A=A, h0=h0, dhT=dhT, w=w)


@functools.lru_cache(maxsize=None)
def _reference(v, h, drop=False):
    """(gradients of the float64 oracle, of its emulated operand policy), both
    with the case's dropout masks."""
    c, x = _case(v, h, drop), _inputs(v, h)
    A, h0, dhT = (x[k].astype(np.float64) for k in ("A", "h0", "dhT"))
    w = {k: a.astype(np.float64) for k, a in x["w"].items()}
    _, caches = O.forward(A, h0, w, T, dropout=EC.dropout_of(c))
    ref = O.backward(A, dhT, caches, w)
    S = SC.grad_scale(x["dhT"])
    emu = {k: a / S for k, a in O.backward_operand_policy(A, S * dhT, caches, w, *SC.policy(c)).items()}
    return ref, emu


def _run(v, h, precision="fp32", drop=False):
    c, x = _case(v, h, drop), _inputs(v, h)
    eng = EE._engine(c, precision)
    res = EE._step(eng, x["A"], x["h0"], x["w"], T, EC.dropout_of(c), x["dhT"], 0xFF, inference=False)
    EE._check_finite(res, c.name)
    return res


@functools.lru_cache(maxsize=None)
def _gpu(v, h, precision="fp32", drop=False):
    return _run(v, h, precision, drop)


FP32_CASES = [(v, h, False) for v, h in SHAPES] + [(v, h, True) for v, h in DROP]


@pytest.mark.parametrize("v,h,drop", FP32_CASES)
def test_emulated_policy_within_bar(v, h, drop):
    """CPU: the emulated policy alone stays within 6e-4 per slice, so that
    1.5 e + 1e-4 fits the 1e-3 bar; the graph without an edge passes dL/dh_T
    through the GRU alone and the single-edge graph has three empty channels."""
    ref, emu_g = _reference(v, h, drop)
    emu, zero = SC.slice_errors(emu_g, ref)
    worst = max(emu, key=emu.get)
    print("\nv %d h %d drop %s: worst emulated slice %s %.2e" % (v, h, drop, worst, emu[worst]))
    assert emu[worst] <= EMU_BAR, (worst, emu[worst])
    assert not SC.not_exactly_zero(ref, zero)
    assert 1.5 * EMU_BAR + 1e-4 <= SC.SLICE_BAR
    x = _inputs(v, h)
    assert all(x["A"][g, c].any() for g in (0, 3) for c in range(C))
    assert x["A"][1].sum() == 1.0 and not x["A"][2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("v,h,drop", FP32_CASES)
def test_slices_fp32(v, h, drop):
    ref, emu_g = _reference(v, h, drop)
    res = _gpu(v, h, "fp32", drop)
    errs, zero = SC.slice_errors(res, ref)
    emu, zero_e = SC.slice_errors(emu_g, ref)
    assert set(errs) == set(emu) and zero == zero_e
    worst = max(errs, key=errs.get)
    print("\nv %d h %d drop %s: worst slice %s %.2e (emulated %.2e)" % (v, h, drop, worst, errs[worst], emu[worst]))
    bad = SC.not_exactly_zero(res, zero)
    assert not bad, bad
    for n, e in errs.items():
        assert e <= SC.SLICE_BAR, (n, e, emu[n])
        assert e <= 1.5 * emu[n] + 1e-4, (n, e, emu[n])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("v,h", BIT16)
def test_slices_16bit(v, h, precision):
    ref, _ = _reference(v, h)
    res = _gpu(v, h, precision)
    _, zero = SC.slice_errors(res, ref)
    nrms = {}
    for (n, a), (_, r) in zip(SC.slices(res), SC.slices(ref)):
        if n not in zero:
            nrms[n] = float(np.sqrt(np.mean((a - r) ** 2) / np.mean(r ** 2)))
            assert np.any(a != 0.0), n
    worst = max(nrms, key=nrms.get)
    print("\nv %d h %d %s: worst slice %s, normalised RMS %.2e" % (v, h, precision, worst, nrms[worst]))
    bad = SC.not_exactly_zero(res, zero)
    assert not bad, bad
    for n, e in nrms.items():
        assert e <= EE.GRAD_RMS_TOL, (n, e)


@pytest.mark.gpu
@pytest.mark.parametrize("v,h,precision,drop", [(v, h, "fp32", d) for v, h, d in FP32_CASES]
                         + [(v, h, p, False) for v, h in BIT16 for p in ("fp16", "bf16")])
def test_two_runs_same_bits(v, h, precision, drop):
    torch = EE._torch()
    r0, r1 = _gpu(v, h, precision, drop), _run(v, h, precision, drop)
    for k in r0:
        assert torch.equal(torch.from_numpy(r0[k]), torch.from_numpy(r1[k])), k
