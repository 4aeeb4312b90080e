"""Dirty, guard-banded allocations for the units that take their outputs and scratch arenas from `torch.empty` / `torch.empty_like`.

The contract under test: an output or an arena may hold ANYTHING on entry, and nothing outside it is written.  torch's caching allocator hides a breach of
either half: a block is fresh from the driver or the block an earlier call of the same shape gave back -- often with the right answer still in it.

`dirty(fill, device)` is a context manager.  While it is active `torch.empty` and `torch.empty_like` are replaced as attributes of the `torch` module (the
wrappers call them as `torch.empty(...)`, so they see the replacement) and are put back in a `finally`.  Nothing happens at import time.  An intercepted call
returns the payload of a larger uint8 allocation filled with `fill`:

    [ GUARD bytes | payload, rounded up to 256 bytes | GUARD bytes ]

so the payload starts as `fill` in every byte, and a store before it or behind it -- behind the last ELEMENT, the round-up is guard too -- changes a byte that
`guards_intact()` reads back.  The fills (`FILLS`):

    0x00   what a fresh block usually holds: the run the other two are compared with
    0xFF   NaN at every float width.  NOT enough alone: `z > 0 ? z : 0` and fmaxf turn a NaN operand into 0 or into the other operand
    0x40   3.0039 as float32, 2.125 as float16, 32.50 as float64, 1077952576 as int32: finite, sizeable, and it survives a ReLU or a maximum

`check(...)` is the whole procedure on one call: plain, then under each fill; see its docstring.  tests/test_dirty_alloc_host.py plants the defects on the CPU
and checks that each is reported."""
import contextlib

import torch

GUARD = 4096          # bytes each side; a multiple of 256, so that the payload keeps the alignment of the allocation (the library's arenas ask for 128 bytes)
ROUND = 256
FILLS = (0x00, 0xFF, 0x40)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class DirtyFailure(AssertionError):
    pass


class Dirty:
    """What `dirty` yields: the record of the intercepted allocations."""

    def __init__(self, fill):
        self.fill = int(fill)
        self.blocks = []          # (the whole uint8 allocation, payload bytes, shape, dtype)

    @property
    def count(self):
        return len(self.blocks)

    def touched(self):
        """-> [(block index, shape, dtype)] of the blocks with a guard byte that no longer equals `fill` (one read-back for all of them)."""
        if not self.blocks:
            return []
        ok = torch.stack([(raw[:GUARD] == self.fill).all() & (raw[GUARD + n:] == self.fill).all() for raw, n, _, _ in self.blocks]).tolist()
        return [(i, tuple(b[2]), b[3]) for i, (b, good) in enumerate(zip(self.blocks, ok)) if not good]

    def guards_intact(self):
        return not self.touched()

    def payload_bytes(self, i):
        raw, n, _, _ = self.blocks[i]
        return raw[GUARD:GUARD + n]

    def _allocate(self, shape, dtype, device, full):
        shape = tuple(int(s) for s in shape)
        count = 1
        for s in shape:
            count *= s
        n = count * _itemsize(dtype)
        raw = full((GUARD + (n + ROUND - 1) // ROUND * ROUND + GUARD,), self.fill, dtype=torch.uint8, device=device)
        self.blocks.append((raw, n, shape, dtype))
        return raw[GUARD:GUARD + n].view(dtype).view(shape)


def _itemsize(dtype):
    return torch.tensor([], dtype=dtype).element_size()


def _size_of(args):
    """The size of a `torch.empty` call: one shape tuple / list / torch.Size of ints, or the ints themselves.  -> a tuple, or None for anything else."""
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    if len(args) == 1 and isinstance(args[0], (tuple, list)):
        args = tuple(args[0])
    elif not args:
        return None
    if all(is_int(v) and v >= 0 for v in args):
        return tuple(args)
    return None


@contextlib.contextmanager
def dirty(fill, device):
    """Intercepted: `torch.empty(size, dtype=..., device=...)` with no other keyword, a device of `device`'s type and a size of plain ints, and
    `torch.empty_like(t)` without keywords for a contiguous strided `t` on such a device.  Every other call goes to the real function."""
    kind = torch.device(device).type
    real_empty, real_like, full = torch.empty, torch.empty_like, torch.full
    record = Dirty(fill)

    def empty(*args, **kwargs):
        size = _size_of(args)
        if size is None or "device" not in kwargs or not set(kwargs) <= {"dtype", "device"} or kwargs["device"] is None:
            return real_empty(*args, **kwargs)
        dev = torch.device(kwargs["device"])
        dtype = kwargs.get("dtype")
        if dev.type != kind or not (dtype is None or isinstance(dtype, torch.dtype)):
            return real_empty(*args, **kwargs)
        return record._allocate(size, torch.get_default_dtype() if dtype is None else dtype, dev, full)

    def empty_like(*args, **kwargs):
        if kwargs or len(args) != 1 or not torch.is_tensor(args[0]):
            return real_like(*args, **kwargs)
        t = args[0]
        if t.device.type != kind or t.layout != torch.strided or not t.is_contiguous() or t.is_quantized:
            return real_like(*args, **kwargs)
        return record._allocate(t.shape, t.dtype, t.device, full)

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield record
    finally:
        torch.empty, torch.empty_like = real_empty, real_like


# ---- the procedure ----------------------------------------------------------------------------------------------------------------------------------
def flatten(result, prefix=""):
    """A tensor, None, or tuples / lists / dicts of them -> [(name, tensor or None)] in a fixed order."""
    if result is None or torch.is_tensor(result):
        return [(prefix or "result", result)]
    if isinstance(result, dict):
        return [pair for k in sorted(result, key=str) for pair in flatten(result[k], "%s[%r]" % (prefix, k))]
    if isinstance(result, (tuple, list)):
        return [pair for i, v in enumerate(result) for pair in flatten(v, "%s[%d]" % (prefix, i))]
    raise TypeError("dirty_alloc.flatten: %s holds a %s" % (prefix or "the result", type(result).__name__))


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t.view(_BITS[t.element_size()]) if not t.is_complex() else torch.view_as_real(t).reshape(-1).view(_BITS[t.element_size() // 2])


def _unravel(flat, shape):
    index = []
    for s in reversed(shape):
        index.append(flat % s)
        flat //= s
    return tuple(reversed(index))


def _first_difference(label, what, name, a, b):
    """None when a and b hold the same bits; else the message, with the first differing element's index in the tensor's shape (plane, row, column)."""
    if (a is None) != (b is None):
        return "%s: %s: %s is %s in one run and a tensor in the other" % (label, what, name, None)
    if a is None:
        return None
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s: %s: %s is %s %s in one run, %s %s in the other" % (label, what, name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    x, y = _bits(a), _bits(b)
    if torch.equal(x, y):
        return None
    differ = (x != y).reshape(a.numel(), -1).any(1)
    flat = int(differ.nonzero()[0])
    return "%s: %s: %s %s differs in %d of %d elements, first at %s: %r against %r" % (label, what, name, tuple(a.shape), int(differ.sum()), a.numel(), _unravel(flat, a.shape),
                                                                                     a.detach().reshape(-1)[flat].item(), b.detach().reshape(-1)[flat].item())


def check(label, call, device, min_count, before=None):
    """`call()` -> every tensor the unit returns and every gradient autograd delivers for it (tensors, None, tuples, lists, dicts).  It is run plain, then under
    dirty(0x00), dirty(0xFF) and dirty(0x40) with the same inputs (built OUTSIDE: `call` allocates nothing but through the unit); `before()` runs ahead of each
    of the four (it empties the module-level caches that would hand back an earlier buffer).  Raises DirtyFailure when

      (c) a guard byte of any block was changed (read after the device has finished),
      (d) fewer than `min_count` allocations were intercepted: the outputs plus arenas the wrapper allocates for the call -- a run that intercepted nothing
          proves nothing,
      (b) a value is NaN under 0xFF (or 0x40) where the 0x00 run's is not,
      (a) any tensor differs in any bit between the 0x00 run and the 0xFF or the 0x40 run: the first differing element's index is named,
      (e) the 0x00 run differs from the plain call (the harness itself changed a result).

    Prints the intercepted count per fill and "guards intact".  -> the flattened 0x00 run."""
    kind = torch.device(device).type
    sync = torch.cuda.synchronize if kind == "cuda" else (lambda: None)
    prepare = before if before is not None else (lambda: None)
    prepare()
    plain = flatten(call())
    sync()
    runs, counts = {}, []
    for fill in FILLS:
        prepare()
        with dirty(fill, device) as d:
            runs[fill] = flatten(call())
        sync()
        bad = d.touched()
        if bad:
            raise DirtyFailure("%s: fill 0x%02X: a byte outside the payload was written, around allocation(s) %s of %d" % (label, fill, bad, d.count))
        if d.count < min_count:
            raise DirtyFailure("%s: fill 0x%02X: %d allocations intercepted, the wrapper makes at least %d: the harness does not see them" % (label, fill, d.count, min_count))
        counts.append(d.count)
    print("%-72s intercepted %s allocations (at least %d), guards intact" % (label, "/".join(map(str, counts)), min_count))
    base = runs[FILLS[0]]
    for what, other in [("fill 0x%02X against 0x00" % f, runs[f]) for f in FILLS[1:]] + [("the plain call against the 0x00 run", plain)]:
        if [n for n, _ in other] != [n for n, _ in base]:
            raise DirtyFailure("%s: %s: the results are %s and %s" % (label, what, [n for n, _ in other], [n for n, _ in base]))
        for (name, t), (_, t0) in zip(other, base):
            if t is not None and t0 is not None and t.shape == t0.shape and t.is_floating_point() and t0.is_floating_point():
                fresh = torch.isnan(t) & ~torch.isnan(t0)
                if bool(fresh.any()):
                    raise DirtyFailure("%s: %s: %s %s holds %d NaN the 0x00 run does not, first at %s" % (label, what, name, tuple(t.shape), int(fresh.sum()),
                                                                                                          _unravel(int(fresh.reshape(-1).nonzero()[0]), t.shape)))
            message = _first_difference(label, what, name, t, t0)
            if message:
                raise DirtyFailure(message)
    return base
