"""Where the general path's product kernels write: the exact [M, N] output of
ggnn_dbg_gemm and ggnn_dbg_gemm_ex (k_gemm, k_gemm_ring, k_gemm_ks with 1 / 2 /
4 column blocks) with A, B and D exact regions of a guard arena
(tests/guard_arena.py), on shapes ragged against the 32- / 64- / 128-row tiles,
the 128-column tiles and the 32-wide K slices, in the fp32-parity and bf16
modes.  Per case the call runs under pattern guards, NaN guards and on plain
allocations: no guard byte changes, A and B stay as they were, D is
bit-identical across the three runs (a 16-byte load over a ragged tail may
read a guard, but no such value may reach D) and within
test_gpu_generic.py's bars of the float64 product.
"""
import ctypes

import numpy as np
import pytest

import guard_arena as GA
import guard_cases as GC
from test_gpu_engine_edges import _torch

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-6, "bf16": 1e-2}       # test_gpu_generic.py: relative to the accumulated magnitude


@pytest.fixture(scope="module")
def operands():
    cache = {}

    def get(M, N, K):
        if (M, N, K) not in cache:
            rng = np.random.default_rng(M * 7 + N * 3 + K)
            A = rng.standard_normal((M, K)).astype(np.float32)
            B = rng.standard_normal((K, N)).astype(np.float32)
            ref = A.astype(np.float64) @ B.astype(np.float64)
            scale = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
            cache[(M, N, K)] = (A, B, ref, scale)
        return cache[(M, N, K)]
    return get


def _call(mem, A, Bop, M, N, K, precision, kernel, b_layout):
    torch = _torch()
    from ggnn_amd import _lib
    a = mem.tensor("A", A.shape, torch.float32, A)
    b = mem.tensor("B", Bop.shape, torch.float32, Bop)
    mem.snapshot("A")
    mem.snapshot("B")
    d = mem.tensor("D", (M, N), torch.float32)
    dims = _lib.dims(1, 1, 64, 1, 1, True, precision)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    if kernel is None:
        _lib.check(_lib.load().ggnn_dbg_gemm(ctypes.byref(dims), M, N, K, P(a), P(b), P(d), s), "ggnn_dbg_gemm")
    else:
        _lib.check(_lib.load().ggnn_dbg_gemm_ex(ctypes.byref(dims), M, N, K, P(a), 0, P(b), b_layout, P(d), kernel, s),
                   "ggnn_dbg_gemm_ex")
    return {"D": d}


def _check(D, ref, scale, K, precision):
    bound = TOL[precision] * scale + K * 2.0 ** -24     # (the f16 lo limb's subnormal floor, test_gpu_generic.py)
    assert np.all(np.abs(D - ref) <= bound), float(np.max(np.abs(D - ref) / bound))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K,kernel,b_layout", GC.GEMM_CASES)
def test_gemm_ex_writes_inside_d(operands, M, N, K, kernel, b_layout, precision):
    A, B, ref, scale = operands(M, N, K)
    Bop = B if b_layout == 0 else np.ascontiguousarray(B.T)
    res = GA.run_guarded(lambda mem: _call(mem, A, Bop, M, N, K, precision, kernel, b_layout),
                         _torch().device("cuda", 0), 8 << 20)
    _check(res["D"], ref, scale, K, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", GC.GEMM_SHAPES)
def test_gemm_writes_inside_d(operands, M, N, K, precision):
    """ggnn_dbg_gemm: the library's own kernel choice for the shape."""
    A, B, ref, scale = operands(M, N, K)
    res = GA.run_guarded(lambda mem: _call(mem, A, B, M, N, K, precision, None, 0), _torch().device("cuda", 0),
                         8 << 20)
    _check(res["D"], ref, scale, K, precision)


@pytest.mark.parametrize("M,N,K,kernel,b_layout", [(M, N, K, k, bl) for (M, N, K) in GC.GEMM_SHAPES
                                                   for k in (2, 3) for bl in (0, 1)
                                                   if not GC.gemm_admits(k, M, N, K, bl)])
def test_unaligned_shapes_are_refused_not_launched(operands, M, N, K, kernel, b_layout):
    """The shapes the case table leaves out for the ring and k_gemm_ks are the
    ones the library itself refuses before any launch: the table drops nothing
    that could run."""
    torch = _torch()
    from ggnn_amd import _lib
    A, B, _, _ = operands(M, N, K)
    Bop = B if b_layout == 0 else np.ascontiguousarray(B.T)
    mem = GA.Arena(torch.device("cuda", 0), capacity=8 << 20)
    with pytest.raises(_lib.GGNNError):
        _call(mem, A, Bop, M, N, K, "fp32", kernel, b_layout)
    torch.cuda.synchronize()
    mem.check()


def test_checker_sees_device_writes():
    GA.device_self_test(_torch().device("cuda", 0))
