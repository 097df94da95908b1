"""tests/_poison.py on the CPU: the poisoned torch.empty / torch.empty_like give the layouts
of the real calls for every call signature the package uses, hold the specified fills, and
their margins catch a write one element before or past an allocation."""
import pytest
import torch

from tests import _poison as P

CL = torch.channels_last_3d
DEV = "cpu"
_X_CL = torch.zeros((2, 8, 3, 4, 5), dtype=torch.bfloat16).contiguous(memory_format=CL)
_X_PLAIN = torch.zeros((3, 7), dtype=torch.float32)
_X_T = torch.zeros((4, 6), dtype=torch.float64).t()          # dense, not contiguous

# every way multimodal_alzheimer_amd/ calls the two functions (args, kwargs)
EMPTY_CALLS = [
    (((2, 8, 3, 4, 5),), dict(dtype=torch.bfloat16, device=DEV, memory_format=CL)),
    (((2, 8, 3, 4, 5),), dict(dtype=torch.float32, device=DEV, memory_format=CL)),
    (((5, 2, 16),), dict(dtype=torch.float32, device=DEV)),
    (((2, 5, 2, 16),), dict(dtype=torch.float32, device=DEV)),
    ((37,), dict(dtype=torch.bfloat16, device=DEV)),                  # one int size
    ((torch.Size([3, 1, 4, 5, 6]),), dict(dtype=torch.float64, device=DEV)),
    ((2, 3, 4), dict(dtype=torch.float64, device=DEV)),               # positional sizes
    (((),), dict(dtype=torch.float64, device=DEV)),                   # 0-d (the losses)
    ((0,), dict(dtype=torch.bfloat16, device=DEV)),                   # empty workspace
    ((13,), dict(dtype=torch.uint8, device=DEV)),
    (((2, 3, 4, 5, 8),), dict(dtype=torch.uint8, device=DEV)),        # argmax buffers
    ((7,), dict(dtype=torch.int32, device=DEV)),
    ((7,), dict(dtype=torch.int64, device=DEV)),
    (((4, 9),), dict(dtype=torch.float64, device=torch.device(DEV))),
    ((6,), dict(device=DEV)),                                         # default dtype
    ((6,), dict(dtype=torch.float32, device=DEV, requires_grad=True)),
]
LIKE_CALLS = [
    (_X_CL, {}), (_X_PLAIN, {}), (_X_T, {}),
    (_X_CL, dict(dtype=torch.float32)),
    (_X_CL, dict(dtype=torch.uint8)),
    (_X_PLAIN, dict(dtype=torch.float64)),
    (_X_CL, dict(memory_format=torch.contiguous_format)),
    (_X_CL[:, ::2], {}),                                              # not dense
    (torch.zeros((), dtype=torch.float64), {}),
    (torch.zeros(5, dtype=torch.int64), {}),
]


def _same_layout(got, ref):
    assert got.shape == ref.shape and got.stride() == ref.stride()
    assert got.dtype == ref.dtype and got.device == ref.device
    assert got.requires_grad == ref.requires_grad
    assert got.data_ptr() % 16 == 0
    assert not got._is_view()


@pytest.mark.parametrize("fill", ["A", "B"])
def test_layout_agrees_with_the_real_calls(fill):
    with P.poisoned(fill, "cpu") as p:
        assert torch.empty is not P._REAL_EMPTY
        for args, kw in EMPTY_CALLS:
            _same_layout(torch.empty(*args, **kw), P._REAL_EMPTY(*args, **kw))
        for x, kw in LIKE_CALLS:
            _same_layout(torch.empty_like(x, **kw), P._REAL_EMPTY_LIKE(x, **kw))
        assert len(p.records) == len(EMPTY_CALLS) + len(LIKE_CALLS)
        # 512 bytes on either side of the data, inside one uint8 buffer
        t = torch.empty((3, 5), dtype=torch.float32, device=DEV)
        buf, nbytes = p.records[-1][:2]
        assert buf.dtype == torch.uint8 and nbytes == 60 and buf.numel() == 60 + 2 * 512
        assert t.data_ptr() == buf.data_ptr() + 512
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        p.check()


def test_fills():
    floats = (torch.bfloat16, torch.float16, torch.float32, torch.float64)
    ints = (torch.uint8, torch.int32, torch.int64)
    with P.poisoned("A", "cpu") as p:
        for dt in floats:
            t = torch.empty((3, 5), dtype=dt, device=DEV)
            assert t.isnan().all()
            assert (p.records[-1][0] == 255).all()                 # margins too
        for dt in ints:
            t = torch.empty((3, 5), dtype=dt, device=DEV)
            assert (t == 1).all()
            assert (p.records[-1][0].view(dt) == 1).all()
        assert torch.empty_like(_X_CL).isnan().all()
        assert (torch.empty_like(_X_CL, dtype=torch.uint8) == 1).all()
    with P.poisoned("B", "cpu") as p:
        for dt in floats + ints:
            t = torch.empty((3, 5), dtype=dt, device=DEV)
            assert (t == 0).all() and (p.records[-1][0] == 0).all()
        assert (torch.empty_like(_X_CL) == 0).all()
        # guarded inputs: the values of the source, NaN margins under both fills
        src = torch.arange(24, dtype=torch.float32).reshape(1, 2, 3, 2, 2).contiguous(
            memory_format=CL)
        g = P.guarded(src)
        assert torch.equal(g, src) and g.stride() == src.stride() and g.data_ptr() % 16 == 0
        buf, nbytes = p.records[-1][:2]
        assert nbytes == 96 and (buf[:512] == 255).all() and (buf[512 + 96:] == 255).all()
        gi = P.guarded(torch.arange(5))
        assert torch.equal(gi, torch.arange(5)) and (p.records[-1][0][:512] == 0).all()
        p.check()
    alias = P.guarded(src.requires_grad_(True))                    # no block: a detached alias
    assert alias.data_ptr() == src.data_ptr() and not alias.requires_grad


def test_pass_through():
    dst = P._REAL_EMPTY(4)
    with P.poisoned("A", "cpu") as p:
        assert torch.empty(4, out=dst) is dst
        m = torch.empty((2, 3), device="meta")
        assert m.device.type == "meta"
        assert torch.empty_like(_X_PLAIN, device="meta").device.type == "meta"
        assert not p.records
    with P.poisoned("A", "cuda") as p:                             # CPU calls are not its own
        t = torch.empty((2, 3), dtype=torch.float32, device=DEV)
        u = torch.empty_like(_X_PLAIN)
        assert t.shape == (2, 3) and u.shape == _X_PLAIN.shape and not p.records
        assert P.guarded(_X_PLAIN).data_ptr() == _X_PLAIN.data_ptr()


def _raw(t, first, count):
    """``count`` elements of t's storage from element offset ``first`` (may leave t)"""
    return P._REAL_EMPTY(0, dtype=t.dtype).set_(t.untyped_storage(),
                                                t.storage_offset() + first, (count,), (1,))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.float64, torch.uint8,
                                   torch.int64])
@pytest.mark.parametrize("fill", ["A", "B"])
def test_margins(dtype, fill):
    n = 2 * 8 * 3 * 4 * 5
    with P.poisoned(fill, "cpu") as p:
        keep = torch.empty((11,), dtype=dtype, device=DEV)
        t = torch.empty((2, 8, 3, 4, 5), dtype=dtype, device=DEV, memory_format=CL)
        g = P.guarded(torch.ones(9, dtype=dtype))
        t.fill_(3)
        keep.fill_(4)
        _raw(t, 0, n).fill_(5)                     # first to last element: in bounds
        g.fill_(6)
        p.check()
        _raw(t, n, 1).fill_(7)                     # one element past the end
        with pytest.raises(AssertionError, match=r"margin after empty \(2, 8, 3, 4, 5\)") as e:
            p.check()
        assert str(dtype) in str(e.value) and "test_poison_helper_cpu.py" in str(e.value)
        assert "margin before" not in str(e.value)
    with P.poisoned(fill, "cpu") as p:
        t = torch.empty((6, 5), dtype=dtype, device=DEV)
        _raw(t, -1, 1).fill_(7)                    # one element before the start
        with pytest.raises(AssertionError, match=r"margin before empty \(6, 5\)"):
            p.check()
    with P.poisoned(fill, "cpu") as p:
        g = P.guarded(torch.ones(9, dtype=dtype))
        _raw(g, 9, 1).fill_(7)
        with pytest.raises(AssertionError, match=r"margin after guarded input \(9,\)"):
            p.check()


def test_restored_after_an_exception():
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned("A", "cpu"):
            assert torch.empty is not P._REAL_EMPTY
            with P.poisoned("B", "cpu"):
                pass
            assert torch.empty is not P._REAL_EMPTY                # the outer block's again
            raise RuntimeError("boom")
    assert torch.empty is P._REAL_EMPTY and torch.empty_like is P._REAL_EMPTY_LIKE
    assert not P._ACTIVE


def test_autograd_adopts_a_poisoned_gradient_in_place():
    """a gradient tensor from the poisoned allocator becomes .grad itself (not a copy), which
    the deferred weight-gradient reductions rely on"""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, w):
            return w.sum()

        @staticmethod
        def backward(ctx, g):
            dw = torch.empty((4, 3), dtype=torch.float32, device=DEV)
            dw.fill_(2.0)
            Fn.ptr = dw.data_ptr()
            return dw

    w = torch.zeros(4, 3, requires_grad=True)
    with P.poisoned("A", "cpu") as p:
        Fn.apply(w).backward()
        p.check()
    assert w.grad.data_ptr() == Fn.ptr and (w.grad == 2).all()
