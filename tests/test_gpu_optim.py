"""Edge shapes of the fused clip + Adam step (k_opt_sqnorm, k_opt_adam in
csrc/k_optim.h) through ``ClipAdam`` against the float64 oracle
``O.adam_step``: three steps per case, grad_scale != 1.

Both kernels take 16-byte pieces when the arrays allow it and single elements
otherwise; a launch has min(256, ceil(max n / 1024)) blocks of 1024 threads per
tensor, so one pass covers 1,048,576 elements in pieces of four and 262,144 one
by one.  The cases reach: the one-by-one path through a misaligned gradient or
a misaligned parameter (a FlatGradients view behind a 150- or 46-element bias
sits 8 bytes off), the tail after the pieces (n % 4 != 0), n below one piece, a
second pass of either path, 16 tensors in one call with most blocks idle, the
squared-norm override on both sides of the clip, norms just either side of the
clip, gradients small enough that epsilon matters, stale scratch, and the
device step count.

Bar: 1e-6 absolute on parameters of magnitude 0.1 (the bar of
test_clip_adam_matches_tf1_semantics); bit equality where stated.
"""
import collections

import numpy as np
import pytest

import ggnn_oracle as O

pytestmark = pytest.mark.gpu

LR, CLIP, GSCALE, TOL = 0.003, 1.0, 0.5, 1e-6
# the betas as the float32 values the C ABI carries (same inputs on both sides): v's factor 1 - beta2 is
# 1.3e-5 (relative) away from 0.001 at float32(0.999)
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))
PAD = 4                       # sentinel floats either side of a parameter (keeps its alignment)
SENTINEL = 12345.0
N_VEC2 = 1048576 + 4099 + 3   # one full pass of float4 pieces, a second trip, then a 2-element tail
N_SCALAR2 = 300001            # one full pass element by element (262,144), then a second trip


Run = collections.namedtuple("Run", "got ref opt p0 ref_m ref_v")
STEP_MUL = (1.0, 2.5, 0.6)    # the gradient norm changes from step to step (see _check)


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a machine without a HIP device")
    return torch


def _place(torch, x, off):
    """x as a contiguous 1-D device tensor starting `off` elements into a flat
    buffer with PAD sentinels either side (off = 1: 4 bytes off a 16-byte
    boundary).  Returns (view, buffer)."""
    dev = torch.device("cuda", 0)
    buf = torch.full((PAD + off + x.size + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[PAD + off:PAD + off + x.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x, np.float32).reshape(-1)).to(dev))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * off) % 16
    return view, buf


def _grad(rng, n, norm):
    """n float32 values whose norm after grad_scale is `norm` (to float32 rounding)."""
    g = rng.standard_normal(n)
    return (g * (norm / GSCALE / np.sqrt(np.sum(g * g)))).astype(np.float32)


def _run(torch, specs, steps=3, use_step_dev=False, nan_scratch=False, seed=0):
    """specs: list of dict(n, p_off, g_off, norm | lo/hi, sq) -- one tensor
    each.  norm: the gradient's norm after grad_scale at step 1 (times
    STEP_MUL at the later steps); (lo, hi): instead,
    entries of magnitude in [lo, hi] (the epsilon regime); sq: squared-norm
    override (before grad_scale) or None.  Runs `steps` steps on the GPU and in
    the oracle; returns a Run."""
    from ggnn_amd.optim import ClipAdam
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda", 0)
    p0 = [(rng.standard_normal(s["n"]) * 0.1).astype(np.float32) for s in specs]
    placed = [_place(torch, x, s.get("p_off", 0)) for x, s in zip(p0, specs)]
    params = [p for p, _ in placed]
    opt = ClipAdam(params, learning_rate=LR, clamp_gradient_norm=CLIP)
    ref_p = [x.astype(np.float64) for x in p0]
    ref_m = [np.zeros_like(x) for x in ref_p]
    ref_v = [np.zeros_like(x) for x in ref_p]
    sqn = [s.get("sq") for s in specs]
    sq_t = [None if q is None else torch.tensor([q], dtype=torch.float32, device=dev) for q in sqn]
    sq_ref = [None if q is None else float(np.float32(q)) for q in sqn]
    step_dev = torch.zeros(1, dtype=torch.int64, device=dev) if use_step_dev else None
    for t in range(1, steps + 1):
        grads = []
        for s in specs:
            if "lo" in s:
                g = np.exp(rng.uniform(np.log(s["lo"]), np.log(s["hi"]), s["n"])) * rng.choice([-1.0, 1.0], s["n"])
                grads.append(g.astype(np.float32))
            else:
                grads.append(_grad(rng, s["n"], s["norm"] * STEP_MUL[(t - 1) % 3]))
        g_t = [_place(torch, g, s.get("g_off", 0))[0] for g, s in zip(grads, specs)]
        if nan_scratch:
            opt._scratch.fill_(float("nan"))
        if use_step_dev:
            step_dev.fill_(t)
            opt.step(g_t, grad_scale=GSCALE, sqnorms=sq_t, step_dev=step_dev)
        else:
            opt.step(g_t, grad_scale=GSCALE, sqnorms=sq_t)
        O.adam_step(ref_p, grads, ref_m, ref_v, t, lr=LR, beta1=B1, beta2=B2, clip_norm=CLIP, grad_scale=GSCALE,
                    sqnorms=sq_ref)
    torch.cuda.synchronize()
    for (p, buf), s in zip(placed, specs):   # nothing written outside a parameter
        lo = PAD + s.get("p_off", 0)
        assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + s["n"]:] == SENTINEL).all())
    return Run(got=[p.cpu().numpy() for p in params], ref=ref_p, opt=opt, p0=p0, ref_m=ref_m, ref_v=ref_v)


def _check(run):
    """Parameters at the 1e-6 bar.  The moments too, at 1e-5 of their largest
    entry (the project's gradient bar; fp32 arithmetic lands near 1e-7): m is
    linear and v quadratic in the clip factor, which the parameters hardly see
    while that factor stays the same from step to step (Adam's step is
    invariant to a constant gradient scale, up to epsilon)."""
    for i, (a, r) in enumerate(zip(run.got, run.ref)):
        err = float(np.abs(a - r).max())
        assert err <= TOL, "tensor %d (n = %d): max error %.3e" % (i, a.size, err)
    for name, got, ref in (("m", run.opt.m, run.ref_m), ("v", run.opt.v, run.ref_v)):
        for i, (a, r) in enumerate(zip(got, ref)):
            err = float(np.abs(a.cpu().numpy() - r).max() / np.abs(r).max())
            assert err <= 1e-5, "%s of tensor %d (n = %d): normalised error %.3e" % (name, i, r.size, err)


SMALL_NS = (1, 2, 3, 5, 1023, 1025)


@pytest.mark.parametrize("p_off,g_off", [
    (0, 1),   # g misaligned only: k_opt_sqnorm and k_opt_adam both element by element
    (1, 0),   # p misaligned only: k_opt_sqnorm in float4 pieces + tail, k_opt_adam element by element
    (0, 0),   # both aligned: float4 pieces, then the n % 4 tail (n = 1, 2, 3: the tail alone)
])
def test_adam_alignment_and_tails(p_off, g_off):
    torch = _torch()
    # n = 1, 2, 3: below one float4 piece; 5, 1025: one-element tail; 1023: three-element tail;
    # norms on both sides of the clip
    specs = [dict(n=n, p_off=p_off, g_off=g_off, norm=(0.3 if i % 2 else 2.0)) for i, n in enumerate(SMALL_NS)]
    run = _run(torch, specs, seed=1 + 2 * p_off + g_off)
    _check(run)


@pytest.mark.parametrize("n,off", [
    (N_VEC2, 0),      # aligned, n = 1,048,576 + 4102: second float4 trip of both kernels, then a 2-element tail
    (N_SCALAR2, 1),   # misaligned, n = 300,001: second element-by-element trip of both kernels
])
def test_adam_second_trip_and_device_step(n, off):
    """A tensor larger than one pass of the 256 x 1024 grid; the same steps with
    the step count read from device memory (ggnn_adam_step_dev) give the same
    bits."""
    torch = _torch()
    specs = [dict(n=n, p_off=off, g_off=off, norm=3.0)]
    run = _run(torch, specs, seed=7)
    _check(run)
    dev = _run(torch, specs, seed=7, use_step_dev=True)
    assert dev.opt.t == 0 and run.opt.t == 3      # (the caller keeps the count under step_dev)
    assert np.array_equal(dev.got[0], run.got[0])


def test_adam_device_step_small_misaligned():
    """The misaligned small tensors through ggnn_adam_step_dev: the bits of the host-step run."""
    torch = _torch()
    specs = [dict(n=n, p_off=1, g_off=1, norm=(0.3 if i % 2 else 2.0)) for i, n in enumerate(SMALL_NS)]
    run = _run(torch, specs, seed=3)
    _check(run)
    dev = _run(torch, specs, seed=3, use_step_dev=True)
    for a, b in zip(dev.got, run.got):
        assert np.array_equal(a, b)


def _sixteen():
    # GGNN_OPT_MAXT = 16 tensors in one call: the large tensor sets the grid (256 blocks per tensor
    # row), so all but one block of the n = 1 rows are idle; alignments, overrides and norms mixed
    specs = [dict(n=1, norm=0.2), dict(n=N_VEC2, norm=3.0), dict(n=1, p_off=1, norm=5.0),
             dict(n=1, g_off=1, norm=0.5, sq=36.0), dict(n=2, norm=2.0), dict(n=3, p_off=1, g_off=1, norm=0.1),
             dict(n=5, norm=1.5, sq=1.0), dict(n=1023, g_off=1, norm=0.9), dict(n=1025, p_off=1, norm=4.0),
             dict(n=1, norm=1.0), dict(n=150, g_off=1, norm=0.4), dict(n=46, p_off=1, g_off=1, norm=2.5),
             dict(n=1, norm=3.0), dict(n=7, lo=1e-9, hi=1e-7), dict(n=1, norm=0.01), dict(n=4, norm=1.2)]
    assert len(specs) == 16
    return specs


def test_adam_sixteen_tensors_one_call():
    torch = _torch()
    run = _run(torch, _sixteen(), seed=11)
    _check(run)


def test_adam_sqnorm_override_both_sides_of_clip():
    """The squared-norm override (the IndexedSlices norm of an embedding) on
    some tensors, None on others.  grad_scale^2 * override decides the clip,
    whatever the tensor's own norm: an override above the clip on a small
    gradient, below it on a large one, and just either side of it."""
    torch = _torch()
    c2 = (CLIP / GSCALE) ** 2                 # the override value whose scaled norm is the clip
    specs = [dict(n=1025, norm=0.2, sq=25.0 * c2),          # own norm below the clip, override above: clipped by 5
             dict(n=1023, g_off=1, norm=5.0, sq=0.04 * c2),  # own norm above the clip, override below: not clipped
             dict(n=600, norm=2.0),                          # no override, clipped by its own norm
             dict(n=37, p_off=1, norm=0.5),                  # no override, unclipped
             dict(n=64, norm=0.7, sq=1.002 * c2),            # override just above the clip
             dict(n=64, norm=0.7, sq=0.998 * c2)]            # override just below the clip
    run = _run(torch, specs, seed=13)
    _check(run)


@pytest.mark.parametrize("norm", [0.999, 1.001])   # just below / just above clamp_gradient_norm = 1
@pytest.mark.parametrize("off", [0, 1])
def test_adam_norm_next_to_the_clip(norm, off):
    torch = _torch()
    specs = [dict(n=4099, p_off=off, g_off=off, norm=norm * CLIP), dict(n=3, norm=norm * CLIP)]
    run = _run(torch, specs, seed=17)
    _check(run)


@pytest.mark.parametrize("off", [0, 1])
def test_adam_epsilon_regime(off):
    """Gradient entries of 1e-9 .. 1e-7 (unclipped): sqrt(v) is 3e-11 .. 3e-9
    after the first step, comparable with epsilon = 1e-8, and the update is
    lr_t * m / (sqrt(v) + eps) with the reference's uncorrected epsilon outside
    the root.  An epsilon inside the root (sqrt(v + 1e-8) ~ 1e-4) or a
    bias-corrected one changes the step by ~lr * 0.3, about 1e-4 to 1e-3."""
    torch = _torch()
    specs = [dict(n=1027, p_off=off, g_off=off, lo=1e-9 / GSCALE, hi=1e-7 / GSCALE), dict(n=260, norm=2.0)]
    run = _run(torch, specs, seed=19)
    _check(run)
    assert np.abs(run.ref[0] - run.p0[0]).max() > 1e-4      # the steps themselves are far above the bar


def test_adam_scratch_is_stored_not_accumulated():
    """k_opt_sqnorm stores one partial per block and k_opt_adam reads only
    those: NaN-filled scratch before every step leaves the bits unchanged."""
    torch = _torch()
    specs = [dict(n=N_SCALAR2, p_off=1, g_off=1, norm=3.0), dict(n=1, norm=0.3), dict(n=1025, norm=2.0),
             dict(n=5, g_off=1, norm=0.2, sq=30.0)]
    clean = _run(torch, specs, seed=23)
    _check(clean)
    dirty = _run(torch, specs, seed=23, nan_scratch=True)
    for a, b in zip(dirty.got, clean.got):
        assert np.array_equal(a, b)
