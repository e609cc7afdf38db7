"""Guard bands around caller buffers: where do the kernels write?

`Arena` is one uint8 tensor from which named regions of an exact byte count
are carved.  Every byte outside a region's exact extent is guard: the slack
between a region's last byte and the next 256-byte boundary, at least `guard`
bytes before the first region and after every region, and 1 MiB at the end.
`check()` compares every guard byte with the copy saved at construction, on
the device, one `torch.equal` per gap.

Every region starts at an address that is a multiple of 256: the alignment
ggnn_api.hip's pack_layout uses and below the caching allocator's 512, so no
kernel's 16-byte-alignment branch takes another path than on a plain
allocation.  The default guard, 64 KiB, is one 128 x 128 fp32 tile, the
largest unit any kernel stores: a misplaced tile is caught whole.

Nothing here imports a GPU at module level; CPU and CUDA tensors work alike
(tests/test_guard_arena.py proves on CPU tensors that the checker can fail).
"""
import numpy as np

ALIGN = 256
TAIL = 1 << 20
FILLS = ("pattern", "nan")


def _up(x, a=ALIGN):
    return (x + a - 1) // a * a


def capacity_for(sizes, guard=65536):
    """The capacity that holds regions of these byte counts, in this order."""
    off = _up(guard)
    for n in sizes:
        off = _up(off + int(n) + guard)
    return off


class GuardError(AssertionError):
    """A guard byte changed.  region: the nearest region's name; side: "after"
    (offsets count from the region's end: end + 0 is 0) or "before" (offsets
    count from its start: start - 1 is -1); first / last: the first and last
    touched offsets; count: the number of touched bytes in that gap."""

    def __init__(self, region, side, first, last, count):
        self.region, self.side, self.first, self.last, self.count = region, side, first, last, count
        rel = "end" if side == "after" else "start"
        super().__init__("guard touched %s region %r: %d byte(s), offsets %+d .. %+d from its %s"
                         % (side, region, count, first, last, rel))


class Arena:
    def __init__(self, device, guard=65536, fill="pattern", capacity=32 << 20):
        """capacity: the bytes available to regions and their guards (the
        1 MiB tail comes on top); capacity_for() sizes it for a known list."""
        import torch
        if fill not in FILLS:
            raise ValueError("fill must be one of %s" % (FILLS,))
        self.device = torch.device(device)
        self.guard = int(guard)
        self.fill = fill
        self.capacity = _up(int(capacity))
        self.total = self.capacity + TAIL
        raw = torch.empty(self.total + ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % ALIGN
        self.buf = raw[skew:skew + self.total]
        assert self.buf.data_ptr() % ALIGN == 0
        if fill == "pattern":       # byte k = (k * 131 + 89) & 0xFF: period 256
            k = torch.arange(ALIGN, dtype=torch.int64, device=self.device)
            period = ((k * 131 + 89) & 0xFF).to(torch.uint8)
            self.buf.copy_(period.repeat(self.total // ALIGN))
        else:                       # NaN as fp32, f16 and bf16; -1 as int32
            self.buf.fill_(0xFF)
        self._saved = self.buf.clone()
        self._regions = []          # (name, start, end), ascending
        self._by_name = {}
        self._snaps = {}
        self._next = _up(self.guard)

    # ------------------------------------------------------------- carving
    def region(self, name, nbytes):
        """A uint8 view of exactly nbytes (0 allowed) at a 256-byte boundary."""
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError("negative size for region %r" % name)
        if name in self._by_name:
            raise ValueError("region %r exists" % name)
        start, end = self._next, self._next + nbytes
        if end + self.guard > self.capacity:
            raise MemoryError("arena capacity %d too small for region %r of %d bytes at %d"
                              % (self.capacity, name, nbytes, start))
        self._next = _up(end + self.guard)
        self._regions.append((name, start, end))
        self._by_name[name] = (start, end)
        return self.buf[start:end]

    def tensor(self, name, shape, dtype, init=None):
        """A typed view of a new region, optionally initialised from a numpy array."""
        import torch
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        item = torch.empty((), dtype=dtype).element_size()
        t = self.region(name, n * item).view(dtype).view(shape)
        if init is not None:
            src = torch.from_numpy(np.array(init, order="C"))
            if tuple(src.shape) != shape or src.dtype != dtype:
                raise ValueError("init of %r: %s %s, region %s %s" % (name, tuple(src.shape), src.dtype, shape, dtype))
            t.copy_(src)
        return t

    def extent(self, name):
        """(start, end) of a region in arena offsets."""
        return self._by_name[name]

    def names(self):
        return [r[0] for r in self._regions]

    # ------------------------------------------------------------ checking
    def gaps(self):
        """[(a, b, before, after)]: the guard intervals [a, b) with the
        regions (name, start, end) on either side (None at the arena's ends)."""
        out, pos, prev = [], 0, None
        for r in self._regions:
            out.append((pos, r[1], prev, r))
            pos, prev = r[2], r
        out.append((pos, self.total, prev, None))
        return [g for g in out if g[1] > g[0]]

    def check(self):
        """Raise GuardError for the first gap whose bytes differ from the saved copy."""
        import torch
        for a, b, prev, nxt in self.gaps():
            if torch.equal(self.buf[a:b], self._saved[a:b]):
                continue
            hit = (self.buf[a:b] != self._saved[a:b]).nonzero().flatten()
            first, last, count = a + int(hit[0]), a + int(hit[-1]), int(hit.numel())
            if prev is None and nxt is None:        # an arena without regions is all guard
                raise GuardError(None, "after", first, last, count)
            if nxt is None or (prev is not None and first - prev[2] <= nxt[1] - 1 - first):
                raise GuardError(prev[0], "after", first - prev[2], last - prev[2], count)
            raise GuardError(nxt[0], "before", first - nxt[1], last - nxt[1], count)

    def snapshot(self, name):
        """Remember a read-only input's bytes."""
        a, b = self._by_name[name]
        self._snaps[name] = self.buf[a:b].clone()

    def unchanged(self, name):
        """Whether the region still holds its snapshot."""
        import torch
        a, b = self._by_name[name]
        return torch.equal(self.buf[a:b], self._snaps[name])

    def snapshots(self):
        return list(self._snaps)


class Plain:
    """Arena's carving interface over plain torch.empty allocations: the same
    test body runs on what the bindings' callers allocate today."""
    fill = None

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self._t, self._snaps = {}, {}

    def region(self, name, nbytes):
        import torch
        if name in self._t:
            raise ValueError("region %r exists" % name)
        self._t[name] = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._t[name]

    tensor = Arena.tensor

    def check(self):
        pass

    def snapshot(self, name):
        self._snaps[name] = self._t[name].clone()

    def unchanged(self, name):
        import torch
        return torch.equal(self._t[name], self._snaps[name])

    def snapshots(self):
        return list(self._snaps)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_guarded(run, device, capacity=32 << 20, guard=65536):
    """run(mem) makes every buffer of a call sequence from ``mem`` (Arena or
    Plain: inputs through tensor(..., init) + snapshot(), outputs and
    workspaces as exact regions), launches it and returns {name: output
    tensor or None}.  It runs three times: pattern guards, NaN guards, plain
    allocations.  After each run and one synchronize: (a) no guard byte
    changed and (d) every snapshot is unchanged.  Then (c) the pattern run's outputs equal the plain run's bit
    for bit, and (b) the NaN run's equal the pattern run's bit for bit and are
    finite where the plain run's are.  Returns the pattern run's outputs as
    numpy arrays."""
    import torch
    device = torch.device(device)
    res = {}
    for kind in ("pattern", "nan", "plain"):
        mem = Plain(device) if kind == "plain" else Arena(device, guard, kind, capacity)
        out = run(mem)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        mem.check()
        for name in mem.snapshots():
            assert mem.unchanged(name), "%s guards: read-only input %r was written" % (kind, name)
        res[kind] = {k: None if t is None else t.cpu().numpy().copy() for k, t in out.items()}
    pat, nan, plain = res["pattern"], res["nan"], res["plain"]
    assert set(pat) == set(nan) == set(plain)
    for k, a in pat.items():
        if a is None:
            assert nan[k] is None and plain[k] is None, k
            continue
        assert a.shape == plain[k].shape and np.array_equal(_bits(a), _bits(plain[k])), \
            "%s: differs between guarded and plain buffers" % k
        assert np.array_equal(_bits(nan[k]), _bits(a)), "%s: depends on the bytes outside its buffers" % k
        if a.dtype.kind == "f":
            assert np.isfinite(nan[k][np.isfinite(plain[k])]).all(), k
    return pat


def device_self_test(device):
    """(f): the checker sees a write made on this device: one byte stored by
    torch into a guard the test owns is reported with its place."""
    a = Arena(device, guard=4096, capacity=1 << 16)
    r = a.region("r", 100)
    a.region("s", 5)
    a.check()
    r.fill_(7)
    a.check()
    start, end = a.extent("r")
    a.buf[end + 3] ^= 0x55
    try:
        a.check()
    except GuardError as e:
        assert (e.region, e.side, e.first, e.last, e.count) == ("r", "after", 3, 3, 1), str(e)
    else:
        raise AssertionError("a device write into a guard went unreported")
