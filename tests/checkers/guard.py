"""Guard bands around device buffers: the only way a kernel's out-of-bounds store is ever seen.

The wrappers allocate outputs with ``torch.empty`` / ``torch.zeros`` and scratch through
``ops._workspace`` (a cache that only grows).  A store past the end of either lands in the caching
allocator's rounding slack, in a neighbouring tensor or in the tail of a workspace a larger call
left behind: no fault, no changed value.  Here every buffer is one ``uint8`` allocation

    [ front guard | payload | back guard ]        all 0xFF bytes (NaN in float32 and bf16, and not
                                                  the canonical NaN arithmetic produces)

with the payload 256-byte aligned, the back guard starting at the payload's last byte + 1 and
each guard ``max(64 KiB, payload bytes)`` capped at 1 MiB, so a store that is off by a whole row
or tile stride still lands inside it.  ``Guarded.check()`` asserts every guard byte is still 0xFF.
A strided payload (rows of ``width`` elements at stride ``ld > width``, or any shape / stride
pair) treats the bytes between the rows as guard too.

``guarded_allocations()`` makes the package's own wrappers allocate such buffers: every module of
``rgbd_amd`` reaches torch through its module-global ``torch``, which is swapped for a proxy whose
six factories (empty, zeros, empty_like, zeros_like, full, ones) return guarded payloads for GPU
requests, and ``ops._ws_cache`` is swapped for an empty dict so that every workspace is new and
exactly the size the wrapper asked for.  Not for use around graph capture (``check`` reads back).

The same classes run on CPU tensors (tests/test_guard_harness.py proves they report overruns).
"""
import contextlib
import sys

import torch

FILL = 0xFF
GUARD_MIN, GUARD_MAX = 64 * 1024, 1024 * 1024
ALIGN = 256


def guard_bytes(payload_bytes):
    return min(max(GUARD_MIN, int(payload_bytes)), GUARD_MAX)


def _prod(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Guarded:
    """One guarded allocation.  ``payload``: the tensor handed out (``shape`` of ``dtype``,
    contiguous unless ``strides`` — in elements — is given).  ``base``: the whole uint8 buffer."""

    def __init__(self, shape, dtype, device, zero=False, tag="", strides=None):
        shape = tuple(int(s) for s in shape)
        isz = torch.empty((), dtype=dtype).element_size()
        if strides is None:
            extent = _prod(shape)
        else:
            strides = tuple(int(s) for s in strides)
            assert len(strides) == len(shape) and all(s >= 0 for s in strides)
            extent = 0 if _prod(shape) == 0 else 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        self.nbytes = extent * isz  # first to last payload byte, stride gaps included
        self.tag, self.dtype, self.shape = tag, dtype, shape
        g = guard_bytes(self.nbytes)
        self.base = torch.full((g + ALIGN + self.nbytes + g,), FILL, dtype=torch.uint8, device=device)
        self.off = g + (-(self.base.data_ptr() + g)) % ALIGN  # payload offset: 256-byte aligned address
        self.end = self.off + self.nbytes                     # back guard: the very next byte
        # the payload shares the storage without being a view of ``base`` to autograd (an autograd
        # Function may return it, and callers may write into it in place)
        contig = tuple(_prod(shape[i + 1:]) for i in range(len(shape)))
        self.payload = torch.empty((0,), dtype=dtype, device=device).set_(
            self.base.untyped_storage(), self.off // isz, shape, contig if strides is None or not extent else strides)
        if strides is None:
            self.owned = None
        else:
            # byte mask of the payload proper; everything else between off and end is gap = guard
            self.owned = torch.zeros((self.nbytes,), dtype=torch.bool, device=device)
            if extent:
                self.owned.as_strided(shape + (isz,), tuple(s * isz for s in strides) + (1,)).fill_(True)
        if zero:
            self.payload.zero_()
        assert self.payload.data_ptr() % ALIGN == 0 or extent == 0

    def touched(self):
        """Device tensor: the number of guard bytes that are no longer 0xFF (no host sync)."""
        b = self.base
        n = (b[:self.off] != FILL).sum() + (b[self.end:] != FILL).sum()
        if self.owned is not None:
            n = n + ((b[self.off:self.end] != FILL) & ~self.owned).sum()
        return n

    def report(self):
        """None when clean, else a description of the touched guard bytes."""
        b = self.base
        bad = b != FILL
        if self.owned is None:
            bad[self.off:self.end] = False
        else:
            bad[self.off:self.end] &= ~self.owned
        idx = bad.nonzero().flatten()
        if idx.numel() == 0:
            return None
        rel = idx.cpu() - self.off  # byte offsets relative to the payload's first byte
        parts = []
        for side, sel in (("front guard", rel < 0), ("stride gap", (rel >= 0) & (rel < self.nbytes)),
                          ("back guard", rel >= self.nbytes)):
            r = rel[sel]
            if r.numel():
                parts.append(f"{side}: {r.numel()} bytes touched, payload-relative offsets {int(r.min())}..{int(r.max())}")
        return (f"guarded buffer '{self.tag}' {self.shape} {self.dtype} ({self.nbytes} payload bytes): "
                + "; ".join(parts))

    def check(self):
        msg = self.report()
        assert msg is None, msg


def strided(rows, width, ld, dtype, device, zero=False, tag=""):
    """Rows of ``width`` elements at stride ``ld`` > width: the gap columns are guard."""
    assert ld >= width
    return Guarded((rows, width), dtype, device, zero=zero, tag=tag, strides=(ld, 1))


class Pool:
    """The buffers handed out in one sweep; ``check_all`` synchronises and checks every one."""

    def __init__(self):
        self.bufs = []
        self.passed_through = 0  # GPU requests the proxy could not guard (layouts it does not model)

    def new(self, shape, dtype, device, zero=False, tag="", strides=None):
        g = Guarded(shape, dtype, device, zero=zero, tag=tag, strides=strides)
        self.bufs.append(g)
        return g

    def place(self, t, tag="input"):
        """A copy of ``t`` (same shape, strides kept when it is not contiguous) between NaN guards:
        a kernel that reads past an input's end and lets the value reach its output changes it."""
        st = None if t.is_contiguous() else t.stride()
        g = self.new(t.shape, t.dtype, t.device, tag=tag, strides=st)
        g.payload.copy_(t)
        return g.payload

    def check_all(self):
        """Number of buffers checked; raises AssertionError naming every touched buffer."""
        if not self.bufs:
            return 0
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        by_dev = {}
        for g in self.bufs:
            by_dev.setdefault(g.base.device, []).append(g)
        msgs = []
        for gs in by_dev.values():
            counts = torch.stack([g.touched() for g in gs])
            if int(counts.sum()):
                for g, c in zip(gs, counts.tolist()):
                    if c:
                        msgs.append(g.report())
        assert not msgs, f"{len(msgs)} of {len(self.bufs)} guarded buffers touched:\n" + "\n".join(msgs)
        return len(self.bufs)


def _is_gpu(device):
    if device is None:
        return False
    return torch.device(device).type == "cuda"


class TorchProxy:
    """Stands in for the ``torch`` module global of the package's modules: every attribute is
    torch's, except that the six factories return guarded payloads for GPU requests."""

    def __init__(self, pool):
        object.__setattr__(self, "_pool", pool)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _tag(self, what):
        f = sys._getframe(1)
        while f.f_back is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        return f"{what} at {f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno}"

    @staticmethod
    def _shape(args, kw):
        if "size" in kw:
            return tuple(kw.pop("size"))
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            return tuple(args[0])
        return tuple(args)

    def _new(self, what, shape, kw, zero=False, fill=None):
        kw = dict(kw)
        dev = kw.pop("device", None)
        dtype = kw.pop("dtype", None)
        if dtype is None:
            dtype = torch.get_default_dtype() if fill is None or isinstance(fill, float) else (
                torch.bool if isinstance(fill, bool) else torch.int64)
        kw.pop("requires_grad", None)
        mf = kw.pop("memory_format", torch.contiguous_format)
        if kw or mf != torch.contiguous_format:
            return None
        g = self._pool.new(shape, dtype, torch.device(dev), zero=zero, tag=self._tag(what))
        if fill is not None:
            g.payload.fill_(fill)
        return g.payload

    def _factory(self, what, args, kw, zero=False):
        if not _is_gpu(kw.get("device")) or kw.get("pin_memory"):
            return getattr(torch, what)(*args, **kw)
        k = dict(kw)
        shape = self._shape(args, k)
        out = self._new(what, shape, k, zero=zero, fill=1 if what == "ones" else None)
        if out is None:
            self._pool.passed_through += 1
            return getattr(torch, what)(*args, **kw)
        return out

    def empty(self, *args, **kw):
        return self._factory("empty", args, kw)

    def zeros(self, *args, **kw):
        return self._factory("zeros", args, kw, zero=True)

    def ones(self, *args, **kw):
        return self._factory("ones", args, kw)

    def full(self, size, fill_value=None, **kw):
        if fill_value is None:
            fill_value = kw.pop("fill_value")
        if not _is_gpu(kw.get("device")) or kw.get("pin_memory") or isinstance(fill_value, torch.Tensor):
            return torch.full(size, fill_value, **kw)
        out = self._new("full", tuple(size), kw, fill=fill_value)
        if out is None:
            self._pool.passed_through += 1
            return torch.full(size, fill_value, **kw)
        return out

    def _like(self, what, t, kw, zero):
        dev = kw.get("device", t.device)
        if not _is_gpu(dev) or kw.get("pin_memory"):
            return getattr(torch, what)(t, **kw)
        probe = torch.empty_like(t, **{**kw, "device": "meta"})  # the layout torch would choose
        extent = 0 if probe.numel() == 0 else 1 + sum((n - 1) * s for n, s in zip(probe.shape, probe.stride()))
        if extent != probe.numel():  # not dense: nothing in the package asks for this
            self._pool.passed_through += 1
            return getattr(torch, what)(t, **kw)
        st = None if probe.is_contiguous() else probe.stride()
        g = self._pool.new(probe.shape, probe.dtype, torch.device(dev), zero=zero, tag=self._tag(what), strides=st)
        return g.payload

    def empty_like(self, t, **kw):
        return self._like("empty_like", t, kw, False)

    def zeros_like(self, t, **kw):
        return self._like("zeros_like", t, kw, True)


class Sweep(Pool):
    """What ``guarded_allocations()`` yields: the pool, plus the workspaces the wrappers made."""

    def workspaces(self):
        return dict(self._ws)


@contextlib.contextmanager
def guarded_allocations():
    """Inside: the wrappers of every loaded ``rgbd_amd`` module allocate guarded buffers and every
    ``ops._workspace`` is new and guarded.  Yields a ``Sweep``; call its ``check_all()`` (before
    or after leaving)."""
    import importlib
    import pathlib
    import rgbd_amd
    from rgbd_amd import ops
    for src in sorted(pathlib.Path(rgbd_amd.__path__[0]).glob("*.py")):  # a module imported lazily inside
        if src.stem != "__init__":                                        # the context would keep torch itself
            importlib.import_module(f"rgbd_amd.{src.stem}")
    sweep = Sweep()
    proxy = TorchProxy(sweep)
    swapped = []
    for name, mod in list(sys.modules.items()):
        if (name == "rgbd_amd" or name.startswith("rgbd_amd.")) and mod is not None \
                and mod.__dict__.get("torch") is torch:
            mod.torch = proxy
            swapped.append(mod)
    saved_cache, saved_zeroed = ops._ws_cache, ops._ws_zeroed
    ops._ws_cache, ops._ws_zeroed = {}, set()
    sweep._ws = ops._ws_cache
    try:
        yield sweep
    finally:
        # the guarded workspaces retire as _workspace retires a buffer it replaces: never freed
        # (a launch still queued, or a plan built inside, may hold their addresses)
        ops._ws_retired.extend(ops._ws_cache.values())
        sweep._ws = dict(ops._ws_cache)
        ops._ws_cache, ops._ws_zeroed = saved_cache, saved_zeroed
        for mod in swapped:
            mod.torch = torch
