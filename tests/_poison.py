"""TEST-ONLY: poisoned allocations.  Every byte of device memory the package uses comes from torch.empty / empty_like / empty_strided / Tensor.new_empty,
and many kernel contracts (include/stllm_hip.h: "Memory regions") rest on nobody reading what was never written.  In a fresh test process such memory
holds zeros or recycled finite activations, so a stale read is invisible.  `poisoned_allocations()` makes it deterministic: while the context is active

  * every tensor handed out by one of the four names has ALL its bytes set to 0xFF before the caller sees it — a NaN in fp64 / fp32 / fp16 / bf16,
    -1 in the signed integers, 255 in uint8 (so one fill serves the uint8 workspaces that kernels reinterpret as floats);
  * persistent scratch is re-filled with 0xFF on EVERY hand-out, on the current stream (ordered in front of the launch that uses it):
    hip.split_workspace (hip._split_ws, the only cached torch.empty buffer of the package: hip._colws allocates afresh per call and is caught as an
    allocation; hip.gemm_workspace is torch.zeros and its flags are defined to be zero: left alone; the pinned h2d ring is written by the host right
    before every copy that reads it and its slots may be in flight: left alone);
  * the rows a KVCache forgets by truncate() — "simply overwritten by the next extend / decode_step" — are re-filled as well: they are undefined again.

The context counts what it poisoned (`allocations`, `refills`, `bytes`); a test asserts `count > 0` for its path, so that a path which stops going
through the patched names fails instead of passing vacuously.  Everything is restored on exit, also after an exception.  Nothing here touches
conftest.py, the pytest settings or Python's start-up: a test imports this module and enters the context itself.

`compare(a, b, p)` is the comparison rule of the poisoned runs: A == B bit for bit (run-to-run determinism), P == A bit for bit, P finite."""
import contextlib

import torch

PATCHED = ("empty", "empty_like", "empty_strided")   # attributes of the torch module; + torch.Tensor.new_empty


class Counts:
    def __init__(self):
        self.allocations = 0
        self.refills = 0
        self.bytes = 0

    @property
    def count(self):
        return self.allocations + self.refills

    def __repr__(self):
        return f"poison(allocations={self.allocations}, refills={self.refills}, bytes={self.bytes})"


def _fill_ff(t, raw_empty, byte=0xFF):
    """0xFF into every byte of t's storage (t owns it: a fresh allocation, or a scratch buffer nobody else holds); on t's device, current stream"""
    if not isinstance(t, torch.Tensor) or t.device.type == "meta" or t.is_sparse or t.layout != torch.strided:
        return 0
    st = t.untyped_storage()
    n = st.nbytes()
    if n == 0:
        return 0
    with torch.no_grad():
        raw_empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,), (1,)).fill_(byte)
    return n


def poison_view_(t):
    """0xFF into the bytes of a (possibly strided) VIEW only: fill_ with the bit pattern reinterpreted per element"""
    if t.numel() == 0:
        return 0
    with torch.no_grad():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
            if t.is_contiguous():
                t.view(torch.uint8).fill_(0xFF)
        elif t.dtype == torch.bool:
            t.fill_(True)
        elif t.dtype == torch.uint8:
            t.fill_(0xFF)
        else:
            t.fill_(-1)
    return t.numel() * t.element_size()


@contextlib.contextmanager
def poisoned_allocations(byte=0xFF):
    """byte: the fill (default 0xFF, the poison).  byte=0 gives what a fresh process usually sees — zeros — deterministically: the "clean" side of the
    positive controls, whose toy functions DO read unwritten memory and would otherwise see whatever block the allocator recycles"""
    c = Counts()
    raw = {n: getattr(torch, n) for n in PATCHED}
    raw_new_empty = torch.Tensor.new_empty
    raw_empty = raw["empty"]

    def wrap(f):
        def g(*a, **k):
            t = f(*a, **k)
            n = _fill_ff(t, raw_empty, byte)
            if n:
                c.allocations += 1
                c.bytes += n
            return t
        g.__name__ = getattr(f, "__name__", "empty")
        g.__wrapped__ = f
        return g

    undo = []

    def patch(obj, name, new):
        old = getattr(obj, name)
        undo.append((obj, name, old))
        setattr(obj, name, new)
        return old
    try:
        for n in PATCHED:
            patch(torch, n, wrap(raw[n]))
        patch(torch.Tensor, "new_empty", wrap(raw_new_empty))
        # persistent scratch of the package (imported lazily: the helper's own tests need torch alone)
        try:
            from stllm_amd import hip
            from stllm_amd.models.llama import KVCache
        except ImportError:
            hip = KVCache = None
        if hip is not None:
            split_workspace = hip.split_workspace

            def poisoned_split_workspace(device, nbytes):
                buf = split_workspace(device, nbytes)
                n = _fill_ff(buf, raw_empty)
                c.refills += 1
                c.bytes += n
                return buf
            patch(hip, "split_workspace", poisoned_split_workspace)
            truncate = KVCache.truncate

            def poisoned_truncate(self, n):
                was = self.lens if self.lens is not None else [self.len] * self.batch
                truncate(self, n)
                now = self.lens if self.lens is not None else [self.len] * self.batch
                for b, (lo, hi) in enumerate(zip(now, was)):
                    if hi > lo:   # positions [lo, hi) of row b are don't-care from here on (local index = position - base_len)
                        for buf in self.qkv:
                            c.bytes += poison_view_(buf[b, lo - self.base_len: hi - self.base_len])
                        c.refills += 1
            patch(KVCache, "truncate", poisoned_truncate)
        yield c
    finally:
        for obj, name, old in reversed(undo):
            setattr(obj, name, old)


def bits_equal(x, y):
    """bit-for-bit: same dtype, shape and bytes (NaN == NaN when the bits agree; +0 != -0)"""
    if isinstance(x, torch.Tensor):
        if not isinstance(y, torch.Tensor) or x.dtype != y.dtype or x.shape != y.shape or x.device != y.device:
            return False
        if x.numel() == 0:
            return True
        return torch.equal(x.contiguous().view(-1).view(torch.uint8), y.contiguous().view(-1).view(torch.uint8))
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(bits_equal(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(bits_equal(a, b) for a, b in zip(x, y))
    if isinstance(x, float):
        return isinstance(y, float) and torch.equal(torch.tensor(x, dtype=torch.float64).view(torch.int64), torch.tensor(y, dtype=torch.float64).view(torch.int64))
    return x == y


def _leaves(x, path=""):
    if isinstance(x, torch.Tensor):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _leaves(v, f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(v, f"{path}[{i}]")
    elif isinstance(x, float):
        yield path, torch.tensor(x)


def first_difference(x, y):
    la, lb = dict(_leaves(x)), dict(_leaves(y))
    for k in la:
        if k not in lb or not bits_equal(la[k], lb[k]):
            return k
    return None if bits_equal(x, y) else "<structure>"


def assert_finite(x, what="P"):
    for path, t in _leaves(x):
        if t.dtype.is_floating_point:
            assert bool(torch.isfinite(t).all()), f"{what}{path}: not finite on a defined output (a read of memory nobody wrote)"


def compare(a, b, p, counts, what=""):
    """the comparison rules of the poisoned runs over the DEFINED outputs (nested tensors / lists / dicts / numbers):
    A == B bit for bit, P == A bit for bit, P finite, poison count > 0"""
    assert counts.count > 0, f"{what}: nothing was poisoned — the path no longer allocates through torch.empty & co, the test would pass vacuously"
    assert bits_equal(a, b), f"{what}: two clean runs differ at {first_difference(a, b)} (run-to-run non-determinism)"
    assert_finite(p, f"{what}: P")
    assert bits_equal(p, a), f"{what}: the poisoned run differs from the clean run at {first_difference(a, p)} (a result depends on unwritten memory)"


# ---- kernel-level: NaN behind a bound, guards around an output --------------------------------------------------------------------------------------
class Guarded:
    """an output [M, N] of `dtype` that sits INSIDE a larger 0xFF-filled buffer: `before` rows in front of it, `after` rows behind it and `pad` more
    columns per row (leading dimension N + pad).  `out` is the view a kernel writes; intact() is true iff every guard byte is still 0xFF."""

    def __init__(self, M, N, dtype, device="cpu", before=2, after=3, pad=8):
        self.M, self.N, self.before = M, N, before
        self.es = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((before + M + after, (N + pad) * self.es), 0xFF, dtype=torch.uint8, device=device)
        self.buf = self.raw.view(dtype)                                  # [before + M + after, N + pad]
        self.out = self.buf[before: before + M, :N]

    def intact(self):
        r, b, M, nb = self.raw, self.before, self.M, self.N * self.es
        return bool((r[:b] == 0xFF).all()) and bool((r[b + M:] == 0xFF).all()) and bool((r[b: b + M, nb:] == 0xFF).all())


def nan_padded(t, pad=8, rows_after=0):
    """a copy of the 2-D tensor t with a leading dimension pad elements larger than its width (and rows_after more rows), everything outside t NaN:
    returns the view [rows, cols] with stride (cols + pad, 1) — what a kernel must read — of a buffer whose other elements it must never read"""
    R, C = t.shape
    buf = torch.full((R + rows_after, C + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:R, :C] = t
    return buf[:R, :C]
