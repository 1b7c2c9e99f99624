"""tests/footprint.py tested on itself, on the CPU: the guard bands report a stray byte on either side and nothing else, the
payloads have the dtype, shape, contiguity and alignment asked for, defined values survive and undefined ones are poison, and the
torch factories are the originals again afterwards.  The deliberate stray writes go through torch indexing on the recorded base
buffer -- memory the test owns; no kernel is involved."""
import pytest
import torch

from tests.footprint import GUARD, GUARD_BYTE, guarded_allocations

NAMES = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones", "clone")
DTYPES = [torch.float32, torch.float64, torch.complex64, torch.int32, torch.int64]
SHAPES = [(1,), (3,), (7, 5), (2, 3, 5), (0,), (4, 0, 3), ()]


def _originals():
    return [getattr(torch, n) for n in NAMES] + [torch.Tensor.new_empty, torch.Tensor.new_zeros, torch.Tensor.clone, torch.Tensor.contiguous]


def test_clean_run_reports_nothing():
    with guarded_allocations(0xFF, "cpu") as rec:
        a = torch.empty(5, 3)
        b = torch.zeros((4,), dtype=torch.int32)
        a.fill_(1.5)
        b += 7
        a[-1, -1] = 2.0                                      # the last payload element is not guard
    assert len(rec.allocations) == 2 and rec.violations() == []
    assert rec.find(a) is rec.allocations[0] and rec.find(b[1:3]) is rec.allocations[1] and rec.find(torch.empty(3)) is None


@pytest.mark.parametrize("nbytes_shape,dtype", [((5,), torch.float32), ((3,), torch.float64), ((7,), torch.uint8), ((0,), torch.float32)])
def test_one_byte_past_and_before_the_payload(nbytes_shape, dtype):
    """20-, 24-, 7- and 0-byte payloads: the trailing guard starts at 24, 24, 8 and 0 bytes from the payload's first byte."""
    for side in ("after", "before"):
        with guarded_allocations(0x00, "cpu") as rec:
            t = torch.empty(nbytes_shape, dtype=dtype)
            other = torch.empty(9)
        a = rec.allocations[0]
        assert a.nbytes == t.numel() * t.element_size() and a.padded == (a.nbytes + 7) // 8 * 8
        at = GUARD + a.padded if side == "after" else GUARD - 1
        a.base[at] = 0
        v = rec.violations()
        assert len(v) == 1 and v[0].allocation is a and v[0].side == side and v[0].count == 1
        assert v[0].first == v[0].last == (a.padded if side == "after" else -1)
        assert rec.find(other) is rec.allocations[1]
        a.base[at] = GUARD_BYTE
        assert rec.violations() == []


def test_first_and_last_changed_offsets():
    with guarded_allocations(0xFF, "cpu") as rec:
        torch.empty(4, dtype=torch.float64)
        torch.zeros(2)
    a, b = rec.allocations
    a.base[GUARD + 32 + 8:GUARD + 32 + 24] = 1                # 16 bytes, one fp64 past the end
    a.base[-1] = 2                                           # and the last guard byte
    b.base[0] = 3                                            # the first guard byte
    b.base[GUARD - 4:GUARD] = 0                              # the fp32 before the payload
    v = rec.violations()
    assert [(x.allocation, x.side, x.first, x.last, x.count) for x in v] == [(a, "after", 40, 32 + GUARD - 1, 17), (b, "before", -GUARD, -1, 5)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_payload_layout(shape, dtype):
    src, other = torch.ones(shape, dtype=dtype), torch.ones(shape, dtype=torch.uint8)
    with guarded_allocations(0xFF, "cpu") as rec:
        made = [torch.empty(shape, dtype=dtype), torch.empty(*shape, dtype=dtype) if shape else torch.empty((), dtype=dtype),
                torch.zeros(shape, dtype=dtype), torch.ones(shape, dtype=dtype), torch.full(shape, 3, dtype=dtype), torch.empty_like(src),
                torch.zeros_like(src), torch.empty_like(other, dtype=dtype), src.new_empty(shape), src.new_zeros(shape),
                torch.empty(shape, dtype=dtype, device="cpu"), torch.empty(torch.Size(shape), dtype=dtype, device=torch.device("cpu"))]
    assert len(rec.allocations) == len(made)
    n = src.numel()
    for t, a in zip(made, rec.allocations):
        assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and a.tensor is t
        assert a.dtype == dtype and a.shape == shape and a.nbytes == n * src.element_size()
        assert a.base.dtype == torch.uint8 and a.base.numel() == 2 * GUARD + a.padded
        start = t.storage_offset() * t.element_size()        # bytes from the buffer start (a tensor of no elements has no data_ptr)
        assert start % 256 == 0 and start == GUARD and t.untyped_storage().data_ptr() == a.base.untyped_storage().data_ptr()
        if n:
            assert t.data_ptr() == a.base.data_ptr() + GUARD and t.data_ptr() % 16 == 0   # the 8- and 16-byte checks of the ABI
        assert bool((a.base[:GUARD] == GUARD_BYTE).all()) and bool((a.base[GUARD + a.padded:] == GUARD_BYTE).all())
    assert rec.violations() == []


@pytest.mark.parametrize("poison", [0xFF, 0x00, 0x5A])
def test_defined_values_and_poison(poison):
    x = torch.arange(6, dtype=torch.float32)
    with guarded_allocations(poison, "cpu") as rec:
        e, el, ne = torch.empty(7, dtype=torch.float64), torch.empty_like(x), x.new_empty((2, 2), dtype=torch.int32)
        z, zl, nz = torch.zeros(3, 2), torch.zeros_like(x), x.new_zeros(5)
        o, f, fi, fb = torch.ones(4, dtype=torch.int64), torch.full((2, 3), 2.5), torch.full((3,), 7), torch.full((2,), -1.0, dtype=torch.float64)
    for a in rec.allocations[:3]:
        assert bool((a.payload_bytes() == poison).all())
    if poison == 0xFF:
        assert bool(torch.isnan(e).all()) and bool(torch.isnan(el).all()) and bool((ne == -1).all())
    if poison == 0x00:
        assert bool((e == 0).all()) and bool((el == 0).all()) and bool((ne == 0).all())
    for t in (z, zl, nz):
        assert bool((t == 0).all())
    assert bool((o == 1).all()) and o.dtype == torch.int64
    assert bool((f == 2.5).all()) and f.dtype == torch.float32
    assert bool((fi == 7).all()) and fi.dtype == torch.int64
    assert bool((fb == -1).all()) and fb.dtype == torch.float64
    assert [a.kind for a in rec.allocations] == ["empty", "empty_like", "new_empty", "zeros", "zeros_like", "new_zeros", "ones", "full", "full", "full"]
    assert rec.violations() == []


def test_originals_are_back_after_exit_and_after_an_exception():
    before = _originals()
    with guarded_allocations(0xFF, "cpu"):
        assert all(a is not b for a, b in zip(_originals(), before))
    assert all(a is b for a, b in zip(_originals(), before))
    with pytest.raises(ZeroDivisionError):
        with guarded_allocations(0xFF, "cpu") as rec:
            torch.empty(3)
            1 / 0
    assert all(a is b for a, b in zip(_originals(), before))
    assert len(rec.allocations) == 1 and rec.violations() == []     # the record survives the exception
    t = torch.empty(3)
    assert t.untyped_storage().nbytes() == 12                 # an ordinary tensor again


def test_other_devices_and_forms_reach_the_originals():
    with guarded_allocations(0xFF, "cuda") as rec:             # the mode the GPU tests use; a CPU request is not its business
        cpu = [torch.empty(3), torch.zeros(2, 2, device="cpu"), torch.full((2,), 1.0), torch.ones(3), torch.empty_like(torch.ones(2)),
               torch.ones(2).new_empty(4), torch.ones(2).new_zeros(4)]
    assert rec.allocations == []
    for t in cpu:
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
    with guarded_allocations(0xFF, "cpu") as rec:
        meta = torch.empty(5, device="meta")
        out = torch.ones(3)
        n0 = len(rec.allocations)
        torch.zeros(3, out=out)                              # out=: the caller's memory, not an allocation
        assert len(rec.allocations) == n0 and bool((out == 0).all())
    assert meta.device.type == "meta" and len(rec.allocations) == 1


def test_clone_and_a_copying_contiguous_are_guarded_copies():
    x = torch.arange(24, dtype=torch.float64).reshape(4, 6)
    with guarded_allocations(0xFF, "cpu") as rec:
        same = x.contiguous()                                # already contiguous: the tensor itself, no allocation
        c, t, f = x.clone(), x.t().contiguous(), torch.clone(x[:, 1:3])
    assert same is x and [a.kind for a in rec.allocations] == ["clone", "contiguous", "clone"]
    for got, want, a in zip((c, t, f), (x, x.t(), x[:, 1:3]), rec.allocations):
        assert torch.equal(got, want) and got.is_contiguous() and got.dtype == want.dtype and rec.find(got) is a
        assert got.storage_offset() * got.element_size() == GUARD and a.nbytes == want.numel() * 8
    assert rec.violations() == []
    g = torch.ones(3, requires_grad=True)
    with guarded_allocations(0xFF, "cpu") as rec:
        h = g.clone()                                        # autograd's clone is not an allocation of a wrapper's
    assert rec.allocations == [] and h.grad_fn is not None
