"""A poisoned allocator with guard bands for the tests.

``poisoned(fill)`` replaces ``torch.empty`` and ``torch.empty_like`` for the length of a
``with`` block.  Every tensor they hand out for the chosen device type has the shape, dtype
and strides of the real call, but lives inside a larger uint8 buffer with MARGIN bytes before
and after it, and the interior and both margins are filled before the tensor is returned:

  fill "A": float dtypes all-ones bytes (a NaN in bf16 / fp16 / fp32 / fp64), integers 1
  fill "B": float dtypes zero bytes, integers 0

A kernel that leaves part of an output, a partial-sum row or a workspace tail unwritten, or
that reads memory it was not given, then gives different (or non-finite) results under the
two fills; one that stores outside its output changes a margin, which ``check()`` reports with
the allocation's shape, dtype and call site.  Integer buffers (window indices, selection
masks, sample orders) only ever hold 0 or 1, so a kernel that wrongly reads one before
writing it shows as an A/B mismatch and not as a wild address.

``guarded(t)`` places a test-made operand in the same kind of buffer (float margins NaN under
both fills: a read past the operand that reaches a result shows as NaN).

The project's Python resolves ``torch.empty`` at call time, so nothing in it changes."""
import contextlib
import os
import sys

import torch

MARGIN = 512                  # bytes before and after every allocation (keeps 16-B alignment)
_REAL_EMPTY = torch.empty
_REAL_EMPTY_LIKE = torch.empty_like
_HERE = os.path.abspath(__file__)
_ACTIVE = []                  # innermost poisoned() last


def _is_float(dtype):
    return dtype.is_floating_point or dtype.is_complex


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    while f is not None and f.f_code.co_filename.endswith("contextlib.py"):
        f = f.f_back
    return ("?", 0) if f is None else (f.f_code.co_filename, f.f_lineno)


def _span(shape, stride):
    """elements between the first and one past the last addressed element"""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, stride))


class Poison:
    def __init__(self, fill, device_type="cuda"):
        if fill not in ("A", "B"):
            raise ValueError("fill is 'A' (NaN / 1) or 'B' (zero bytes / 0)")
        self.fill = fill
        self.device_type = device_type
        self.records = []         # (buffer, data bytes, front / back patterns, description)
        self._patterns = {}

    # ------------------------------------------------------------------ allocation
    def _pattern(self, dtype, device, nan):
        """MARGIN bytes of the margin fill of ``dtype``"""
        key = (dtype, str(device), nan)
        p = self._patterns.get(key)
        if p is None:
            p = _REAL_EMPTY(MARGIN, dtype=torch.uint8, device=device)
            if _is_float(dtype):
                p.fill_(255 if nan else 0)
            else:
                p.view(dtype).fill_(1 if self.fill == "A" else 0)
            self._patterns[key] = p
        return p

    def _place(self, shape, stride, dtype, device, site, what, src=None):
        isz = dtype.itemsize
        nbytes = _span(shape, stride) * isz
        buf = _REAL_EMPTY(MARGIN + nbytes + MARGIN, dtype=torch.uint8, device=device)
        # margins of a guarded float operand are NaN under both fills
        pat = self._pattern(dtype, device, self.fill == "A" or src is not None)
        buf[:MARGIN].copy_(pat)
        buf[MARGIN + nbytes:].copy_(pat)
        if nbytes:
            if _is_float(dtype):
                buf[MARGIN:MARGIN + nbytes].fill_(255 if self.fill == "A" else 0)
            else:
                buf[MARGIN:MARGIN + nbytes].view(dtype).fill_(1 if self.fill == "A" else 0)
        t = _REAL_EMPTY(0, dtype=dtype, device=device)
        # set_ on the buffer's storage: not an autograd view, so AccumulateGrad still adopts
        # such a tensor as .grad in place
        t.set_(buf.untyped_storage(), MARGIN // isz, tuple(shape), tuple(stride))
        if src is not None:
            t.copy_(src)
        assert t.data_ptr() % 16 == 0
        self.records.append((buf, nbytes, pat,
                             f"{what} {tuple(shape)} {dtype} at {site[0]}:{site[1]}"))
        return t

    def _mine(self, device):
        return torch.device(device).type == self.device_type

    def empty(self, *args, **kwargs):
        if kwargs.get("out") is not None or kwargs.get("pin_memory"):
            return _REAL_EMPTY(*args, **kwargs)
        device = kwargs.get("device")
        if device is None:
            device = torch.get_default_device()
        if not self._mine(device) or kwargs.get("layout", torch.strided) != torch.strided:
            return _REAL_EMPTY(*args, **kwargs)
        meta = _REAL_EMPTY(*args, **{**kwargs, "device": "meta", "requires_grad": False})
        t = self._place(meta.shape, meta.stride(), meta.dtype, torch.device(device),
                        _call_site(), "empty")
        return t.requires_grad_(True) if kwargs.get("requires_grad") else t

    def empty_like(self, inp, **kwargs):
        device = kwargs.get("device")
        if device is None:
            device = inp.device
        if kwargs.get("pin_memory") or not self._mine(device) or \
                kwargs.get("layout", inp.layout) != torch.strided or inp.layout != torch.strided:
            return _REAL_EMPTY_LIKE(inp, **kwargs)
        # (preserve_format, a memory_format= or a dtype= override resolve as in the real call)
        meta = _REAL_EMPTY_LIKE(inp.detach(),
                                **{**kwargs, "device": "meta", "requires_grad": False})
        t = self._place(meta.shape, meta.stride(), meta.dtype, torch.device(device),
                        _call_site(), "empty_like")
        return t.requires_grad_(True) if kwargs.get("requires_grad") else t

    def guarded(self, t):
        """a copy of ``t`` (same sizes, strides where dense) between two margins"""
        src = t.detach()
        if not self._mine(t.device):
            return src
        if _span(src.shape, src.stride()) != src.numel() or 0 in src.stride():
            src = src.contiguous()
        return self._place(src.shape, src.stride(), src.dtype, src.device, _call_site(),
                           "guarded input", src=src)

    # ------------------------------------------------------------------ the check
    def check(self):
        """synchronise, then assert that every byte of every margin still holds its fill"""
        if self.device_type == "cuda" and torch.cuda.is_available():
            torch.cuda.synchronize()
        if not self.records:
            return
        flags = []
        for buf, nbytes, pat, _ in self.records:
            flags.append(((buf[:MARGIN] != pat).any(), (buf[MARGIN + nbytes:] != pat).any()))
        bad = torch.stack([torch.stack(f) for f in flags]).cpu()
        msgs = []
        for (buf, nbytes, pat, desc), (front, back) in zip(self.records, bad.tolist()):
            for hit, name, band in ((front, "before", buf[:MARGIN]),
                                    (back, "after", buf[MARGIN + nbytes:])):
                if hit:
                    idx = (band != pat).nonzero().flatten().cpu()
                    off = (int(idx[0]) - MARGIN, int(idx[-1]) - MARGIN + 1) if name == "before" \
                        else (int(idx[0]), int(idx[-1]) + 1)
                    msgs.append(f"margin {name} {desc} changed: {idx.numel()} byte(s), offsets "
                                f"{off[0]}..{off[1]} relative to the allocation's "
                                f"{'start' if name == 'before' else 'end'}")
        assert not msgs, "out-of-bounds writes:\n  " + "\n  ".join(msgs)


@contextlib.contextmanager
def poisoned(fill, device_type="cuda"):
    p = Poison(fill, device_type)
    prev = (torch.empty, torch.empty_like)
    _ACTIVE.append(p)
    torch.empty, torch.empty_like = p.empty, p.empty_like
    try:
        yield p
    finally:
        torch.empty, torch.empty_like = prev
        _ACTIVE.remove(p)


def guarded(t):
    """``t`` in a margined buffer of the innermost active ``poisoned`` block; outside one a
    detached alias of ``t``, so one input builder serves the plain and the poisoned runs and
    ``requires_grad_()`` on the result never reaches the shared operand"""
    return _ACTIVE[-1].guarded(t) if _ACTIVE else t.detach()
