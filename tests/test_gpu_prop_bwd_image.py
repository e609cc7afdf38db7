"""k_prop_bwd's dM images at every tile shape: the dM^T rows it stores for the
weight gradient are read back from the 16-bit LDS image (transposing reads),
the fp8 lo image takes its residuals from the pairs packed for that image, and
two j tiles are in flight in phase a.  A wrong lane address in the read-back,
a stale image or a missed store shows in a channel's dW_c; a wrong residual in
dL/dh0.

Cases: every padded graph size V in {32, 64, 128} at hidden {64, 128, 256} in
the fp32-parity mode, and fp16 / bf16 at (128, 256); b = 3, C = 4, T = 2.
(Hidden 64 runs the general path: the specialised kernels exist for hidden
128 / 256 only; the case stays so that a change of that rule is covered.)  Graph 0 has no edge in
channel 3 (its dbeta partials and, where the weight gradient reads every row,
its dM^T rows are zero-filled), graph 1 has a single edge (three empty
channels), graph 2's dL/dh_T is scaled by 2^-6.  Every buffer the step writes
is filled with 0xFF first (the runner of tests/test_gpu_engine_edges.py).

Bars, those of tests/test_gpu_slice_parity.py: every graph's dL/dh0, every
channel's dW_c and dbeta_c and every block of the GRU's gradients within 1e-3
of its own maximum against the float64 oracle and within 1.5 x the emulated
operand policy's error + 1e-4; the 16-bit modes at a normalised RMS error of
5e-2 per slice; what the oracle has at exactly 0 is exactly 0.  The seed is
the first whose emulated per-slice error is at most 6e-4 at every shape (as in
tests/slice_cases.py; seed 0: 7.3e-4 at v 64, hidden 128; seed 1: 5.6e-4 at
most).  A second run on a fresh engine must give the same bits.

Measured on an MI355X: the module runs in 2.8 s (22 tests); worst fp32 slice
5.3e-4 (v 128, hidden 128, gates_kernel[h,u]; the emulation has 5.4e-4 there);
the 16-bit modes' worst slice (edge_weights[3]) has a normalised RMS error of
3.1e-3 (fp16) and 3.0e-2 (bf16)."""
import functools

import numpy as np
import pytest

import ggnn_oracle as O
import slice_cases as SC
import test_gpu_engine_edges as EE

pytestmark = pytest.mark.gpu

B, C, T = 3, 4, 2
SEED = 1
QUIET = 2.0 ** -6
SHAPES = [(v, h) for v in (32, 64, 128) for h in (64, 128, 256)]


def _case(v, h):
    return SC.Case("img_v%d_h%d" % (v, h), B, v, h, C, T, 1.0, 1.0, SEED, "dense", True, False, 1.0, 0)


@functools.lru_cache(maxsize=None)
def _inputs(v, h):
    rng = np.random.default_rng(4100 + 7 * v + h + SEED)
    A = (rng.random((B, C, v, v)) < SC.DENSITY).astype(np.float32)
    A[0, 3] = 0.0                                   # an empty channel
    A[1] = 0.0                                      # a single edge
    A[1, 1, int(rng.integers(v)), int(rng.integers(v))] = 1.0
    h0 = rng.uniform(-0.2, 0.2, (B, v, h)).astype(np.float32)
    w = O.synthetic_weights(h, C, seed=4100 + SEED)
    dhT = rng.standard_normal((B, v, h)).astype(np.float32)
    dhT[2] *= np.float32(QUIET)
    for x in (A, h0, dhT) + tuple(w.values()):
        x.setflags(write=False)
    return dict(A=A, h0=h0, dhT=dhT, w=w)


@functools.lru_cache(maxsize=None)
def _reference(v, h):
    """(gradients of the float64 oracle, of its emulated operand policy)."""
    x = _inputs(v, h)
    A, h0, dhT = (x[k].astype(np.float64) for k in ("A", "h0", "dhT"))
    w = {k: a.astype(np.float64) for k, a in x["w"].items()}
    _, caches = O.forward(A, h0, w, T)
    ref = O.backward(A, dhT, caches, w)
    S = SC.grad_scale(x["dhT"])
    emu = {k: a / S for k, a in O.backward_operand_policy(A, S * dhT, caches, w, *SC.policy(_case(v, h))).items()}
    return ref, emu


def _run(v, h, precision="fp32"):
    c, x = _case(v, h), _inputs(v, h)
    eng = EE._engine(c, precision)
    res = EE._step(eng, x["A"], x["h0"], x["w"], T, None, x["dhT"], 0xFF, inference=False)
    EE._check_finite(res, c.name)
    return res


@functools.lru_cache(maxsize=None)
def _gpu(v, h, precision="fp32"):
    return _run(v, h, precision)


@pytest.mark.parametrize("v,h", SHAPES)
def test_slices_fp32(v, h):
    ref, emu_g = _reference(v, h)
    res = _gpu(v, h)
    errs, zero = SC.slice_errors(res, ref)
    emu, zero_e = SC.slice_errors(emu_g, ref)
    assert set(errs) == set(emu) and zero == zero_e
    worst = max(errs, key=errs.get)
    print("\nv %d h %d: worst slice %s %.2e (emulated %.2e)" % (v, h, worst, errs[worst], emu[worst]))
    bad = SC.not_exactly_zero(res, zero)
    assert not bad, bad
    for n, e in errs.items():
        assert e <= SC.SLICE_BAR, (n, e, emu[n])
        assert e <= 1.5 * emu[n] + 1e-4, (n, e, emu[n])


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_slices_16bit(precision):
    v, h = 128, 256
    ref, _ = _reference(v, h)
    res = _gpu(v, h, precision)
    _, zero = SC.slice_errors(res, ref)
    nrms = {}
    for (n, a), (_, r) in zip(SC.slices(res), SC.slices(ref)):
        if n not in zero:
            nrms[n] = float(np.sqrt(np.mean((a - r) ** 2) / np.mean(r ** 2)))
            assert np.any(a != 0.0), n
    worst = max(nrms, key=nrms.get)
    print("\n%s: worst slice %s, normalised RMS %.2e" % (precision, worst, nrms[worst]))
    bad = SC.not_exactly_zero(res, zero)
    assert not bad, bad
    for n, e in nrms.items():
        assert e <= EE.GRAD_RMS_TOL, (n, e)


@pytest.mark.parametrize("v,h,precision", [(v, h, "fp32") for v, h in SHAPES] + [(128, 256, "fp16"), (128, 256, "bf16")])
def test_two_runs_same_bits(v, h, precision):
    torch = EE._torch()
    r0, r1 = _gpu(v, h, precision), _run(v, h, precision)
    for k in r0:
        assert torch.equal(torch.from_numpy(r0[k]), torch.from_numpy(r1[k])), k
