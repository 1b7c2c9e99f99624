"""Where a call writes: guard bands around every tensor that a wrapper allocates, and poison in what it leaves undefined.

``guarded_allocations(poison, device_type)`` replaces the Python-level torch factories (``torch.empty``, ``empty_like``, ``zeros``,
``zeros_like``, ``full``, ``ones``, ``Tensor.new_empty``, ``Tensor.new_zeros``, and the two copies through which the wrappers make a
tensor that a kernel then updates in place: ``clone`` and a ``contiguous`` that copies) for requests on ``device_type``; requests for
any other device, and forms the replacements do not understand (``out=``, ``names=``, a sparse layout), go to the original function.  Each
replacement allocates one uint8 buffer

    [ GUARD bytes of 0xA5 | payload | pad to 8 bytes | GUARD bytes of 0xA5 ]

and returns the payload viewed with the requested dtype and shape: contiguous, starting GUARD (a multiple of 256) bytes into the
buffer, so the 8- and 16-byte alignment checks of the C ABI hold as they do for a tensor of the caching allocator.  The trailing
guard begins at the payload size rounded up to 8 bytes -- not at the allocator's 512-byte rounding, which is the slack that hides a
stray write in an ordinary run.  ``empty``-class payloads are filled with the ``poison`` byte (0xFF: NaN in every float format and
-1 in every integer; 0x00: what a fresh process usually sees), so a result that depends on memory the call never defined differs
between two poisons; ``zeros``, ``full``, ``ones`` and copied payloads hold their defined value.

On exit -- by exception too -- the originals are put back and, in CUDA mode, the device is synchronised.  ``allocations`` then
lists every request (byte size, dtype, shape, the tensor, the base buffer) and ``violations()`` every allocation whose guard bytes
changed, with the side and the first and last changed byte offsets, counted from the first payload byte (negative: before it).

GUARD is 64 KiB.  The largest block that one workgroup of a covered kernel writes as a unit is smaller: the 64 x 64 fp64 output tile
of glowk_rpca_gemm (GEMM_TILE in csrc/glowk_rpca_index.h), 32 KiB; then the 64 x 64 fp32 tile of the rows pass of glowk_median_filter
(16 KiB) and the 32 x 32 tiles of the NMF, 2DFT and nearest-neighbour kernels.  So a workgroup that runs off the end of its tensor by a
whole unit still lands inside the guard.  A kernel with a larger unit has to raise GUARD and be named here.

What this cannot see: a write that strays further than GUARD bytes from the payload (a wrong batch stride, say) lands in other
memory and is out of reach of this method; so is memory that the library allocates itself (the flow engine's workspace), and a
tensor made by another torch operator (``stack``, ``to``, arithmetic): the accounting assertion of tests/test_gpu_footprint.py
(every returned tensor is a view of a recorded payload) is what shows that a wrapper's outputs do not come by such a route.

``Guarded`` is the hand-made form for calls through ctypes: a buffer with canary words on each side of the part a call may
write."""
import contextlib
import ctypes

import numpy as np
import torch

GUARD_BYTE = 0xA5
GUARD = 64 * 1024            # bytes on each side; a multiple of 256


class Allocation:
    """One guarded request: ``tensor`` is what the caller got, ``base`` the uint8 buffer around it, ``kind`` the factory."""

    def __init__(self, kind, base, tensor, nbytes):
        self.kind, self.base, self.tensor, self.nbytes = kind, base, tensor, nbytes
        self.dtype, self.shape = tensor.dtype, tuple(tensor.shape)
        self.padded = (nbytes + 7) // 8 * 8          # the trailing guard starts here, counted from the first payload byte

    def payload_bytes(self):
        return self.base[GUARD:GUARD + self.nbytes]

    def holds(self, t):
        """True when ``t`` lies wholly inside this payload's bytes of the same storage (the payload itself or a view of it)."""
        if t.device != self.base.device or t.untyped_storage().data_ptr() != self.base.untyped_storage().data_ptr():
            return False
        if t.numel() == 0:
            return True
        lo = t.storage_offset() * t.element_size()
        hi = lo + (sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
        return GUARD <= lo and hi <= GUARD + self.nbytes

    def __repr__(self):
        return "Allocation(%s, %s, %s, %d bytes)" % (self.kind, self.dtype, self.shape, self.nbytes)


class Violation:
    def __init__(self, allocation, side, first, last, count):
        self.allocation, self.side, self.first, self.last, self.count = allocation, side, first, last, count

    def __repr__(self):
        return "%s guard of %r: %d byte(s) changed, offsets %d .. %d" % (self.side, self.allocation, self.count, self.first, self.last)


class _Record:
    def __init__(self, poison, device_type):
        self.poison, self.device_type, self.allocations = poison, device_type, []

    def violations(self):
        out = []
        for a in self.allocations:
            for side, lo, hi, origin in (("before", 0, GUARD, -GUARD), ("after", GUARD + a.padded, a.base.numel(), a.padded)):
                bad = torch.nonzero(a.base[lo:hi] != GUARD_BYTE).flatten()
                if bad.numel():
                    out.append(Violation(a, side, origin + int(bad[0]), origin + int(bad[-1]), int(bad.numel())))
        return out

    def find(self, t):
        """The allocation whose payload holds ``t``, or None."""
        for a in self.allocations:
            if a.holds(t):
                return a
        return None


_PASS = ("requires_grad", "pin_memory", "layout", "memory_format")


def _size(args):
    if len(args) == 1 and not isinstance(args[0], (int, np.integer)):
        args = tuple(args[0])
    return tuple(int(n) for n in args)


def _fill_dtype(value):
    if isinstance(value, bool):
        return torch.bool
    if isinstance(value, (int, np.integer)):
        return torch.int64
    if isinstance(value, complex):
        return torch.complex128 if torch.get_default_dtype() == torch.float64 else torch.complex64
    return torch.get_default_dtype()


@contextlib.contextmanager
def guarded_allocations(poison, device_type="cuda"):
    """See the module docstring.  Yields the record; read ``allocations`` and ``violations()`` after the block."""
    assert 0 <= poison <= 255
    rec = _Record(poison, device_type)
    names = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones", "clone")
    orig = {n: getattr(torch, n) for n in names}
    orig_new = {n: getattr(torch.Tensor, n) for n in ("new_empty", "new_zeros", "clone", "contiguous")}
    default_device = orig["empty"](0).device

    def ours(device, kw):
        """The resolved device when the request is one of ours, else None."""
        if any(k not in _PASS for k in kw) or kw.get("layout", torch.strided) is not torch.strided or kw.get("pin_memory"):
            return None
        dev = default_device if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        return dev if dev.type == device_type else None

    def make(kind, size, dtype, dev, fill, requires_grad=False):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        n = 1
        for s in size:
            n *= s
        nbytes = n * orig["empty"](0, dtype=dtype).element_size()
        padded = (nbytes + 7) // 8 * 8
        base = orig["full"]((GUARD + padded + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        t = base[GUARD:GUARD + nbytes].view(dtype).view(size)
        if fill is None:
            base[GUARD:GUARD + nbytes] = poison
        else:
            t.fill_(fill)
        rec.allocations.append(Allocation(kind, base, t, nbytes))
        return t.requires_grad_() if requires_grad else t

    def factory(kind, fill):
        def f(*args, dtype=None, device=None, **kw):
            dev = ours(device, kw)
            if dev is None:
                return orig[kind](*args, dtype=dtype, device=device, **kw)
            return make(kind, _size(args), dtype, dev, fill, kw.get("requires_grad", False))
        return f

    def like(kind, fill):
        def f(x, *, dtype=None, device=None, **kw):
            dev = ours(x.device if device is None else device, kw)
            if dev is None:
                return orig[kind](x, dtype=dtype, device=device, **kw)
            return make(kind, tuple(x.shape), x.dtype if dtype is None else dtype, dev, fill, kw.get("requires_grad", False))
        return f

    def full(size, fill_value, *, dtype=None, device=None, **kw):
        dev = ours(device, kw)
        if dev is None or isinstance(fill_value, torch.Tensor):
            return orig["full"](size, fill_value, dtype=dtype, device=device, **kw)
        return make("full", _size((size,)), _fill_dtype(fill_value) if dtype is None else dtype, dev, fill_value, kw.get("requires_grad", False))

    def new(kind, fill):
        def f(self, *args, dtype=None, device=None, **kw):
            dev = ours(self.device if device is None else device, kw)
            if dev is None:
                return orig_new[kind](self, *args, dtype=dtype, device=device, **kw)
            return make(kind, _size(args), self.dtype if dtype is None else dtype, dev, fill, kw.get("requires_grad", False))
        return f

    def copy_of(kind):
        """clone, and contiguous where it copies: the tensor a wrapper hands to a kernel that updates in place."""
        def f(self, *args, **kw):
            plain = not args and all(v in (torch.preserve_format, torch.contiguous_format) for v in kw.values()) and set(kw) <= {"memory_format"}
            if kind == "contiguous" and plain and self.is_contiguous():
                return self
            if not plain or self.device.type != device_type or self.layout is not torch.strided or self.requires_grad or self.is_conj() or self.is_neg():
                return orig_new[kind](self, *args, **kw)
            return make(kind, tuple(self.shape), self.dtype, self.device, None).copy_(self)
        return f

    patched = {"empty": factory("empty", None), "zeros": factory("zeros", 0), "ones": factory("ones", 1), "full": full,
               "empty_like": like("empty_like", None), "zeros_like": like("zeros_like", 0)}
    patched_new = {"new_empty": new("new_empty", None), "new_zeros": new("new_zeros", 0), "clone": copy_of("clone"), "contiguous": copy_of("contiguous")}
    patched["clone"] = lambda x, **kw: patched_new["clone"](x, **kw)
    try:
        for n, f in patched.items():
            setattr(torch, n, f)
        for n, f in patched_new.items():
            setattr(torch.Tensor, n, f)
        yield rec
    finally:
        for n, f in orig.items():
            setattr(torch, n, f)
        for n, f in orig_new.items():
            setattr(torch.Tensor, n, f)
        if device_type == "cuda" and torch.cuda.is_initialized():     # never initialised: nothing was launched
            torch.cuda.synchronize()


# ---- by hand, for calls through ctypes -----------------------------------------------------------------------------------------------
CANARY, GUARD_WORDS = -7.25, 64


class Guarded:
    """A device buffer with GUARD_WORDS canary words on each side of the part a call may write."""

    def __init__(self, shape, dtype, fill, canary=CANARY):
        self.n, self.canary = int(np.prod(shape)), canary
        self.buf = torch.full((self.n + 2 * GUARD_WORDS,), canary, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD_WORDS:GUARD_WORDS + self.n].view(shape)
        self.t.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD_WORDS] == self.canary).all()) and bool((self.buf[GUARD_WORDS + self.n:] == self.canary).all())
