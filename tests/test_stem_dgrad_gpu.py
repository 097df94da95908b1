"""The input gradient of a Cin = 1 conv at kernel level: the dedicated stem kernel
(mmad_conv3d_dgrad_raw) and the generic route (weight Ci padded to 8 + mmad_conv3d_dgrad +
mmad_take_channel) against torch.nn.grad.conv3d_input in float64 on the same operands.

Bars.  dX of the stem kernel is accumulated in fp32 and stored in fp32 / f64 without a bf16
re-rounding, so it takes the project's float64 bar for fp32-accumulated gradients
(test_lattice5_gpu.py's dW bar): per element |err| <= 1e-3 |ref| + 1e-4 mag, mag = the same
transposed conv on |dY|, |W|.  The generic route in bf16 stores a bf16 dX (the conv bar:
2^-7 |ref| + 1e-3 max|ref| of an fp32 reference); in fp32 compute it takes the float64 bar."""
import pytest
import torch

from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import volume_ops as V

pytestmark = pytest.mark.gpu
DEV = "cuda"

STEM_SHAPES = [
    (2, 1, 16, 16, 16),     # batch stride
    (1, 1, 9, 11, 13),      # all extents odd, smaller than two windows
    (1, 1, 3, 5, 4),        # grid smaller than the 4-tap window
    (1, 1, 19, 23, 21),     # MNI-like parities
    (1, 1, 6, 6, 160),      # wo = 80: two column chunks
    (1, 1, 37, 50, 64),     # several work items per sample, partial row groups
]
_CACHE = {}


def _operands(shape, co=64, k=7, stride=2, pad=3, seed=0):
    """(desc, bf16-representable fp32 weight, bf16-representable dY (n, co, do, ho, wo) fp32,
    float64 reference dX, float64 magnitude), computed once per geometry on the CPU"""
    key = (shape, co, k, stride, pad)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1000 + seed + sum(shape) + co + k)
        d = V.conv_desc(shape, (co, 1, k, k, k), (stride,) * 3, (pad,) * 3, (1, 1, 1))
        w = (torch.randn((co, 1, k, k, k), generator=gen) * 0.1).bfloat16().float()
        dy = torch.randn((shape[0], co, d.do_, d.ho, d.wo), generator=gen).bfloat16().float()
        ref = torch.nn.grad.conv3d_input(shape, w.double(), dy.double(), stride=stride,
                                         padding=pad)
        mag = torch.nn.grad.conv3d_input(shape, w.double().abs(), dy.double().abs(),
                                         stride=stride, padding=pad)
        _CACHE[key] = (d, w, dy, ref, mag)
    return _CACHE[key]


def _assert_f64_bar(got, ref, mag, what):
    err = (got.double().cpu() - ref).abs()
    lim = 1e-3 * ref.abs() + 1e-4 * mag
    worst = (err - lim).max().item()
    print(f"{what}: max|err| {err.max().item():.3e}, max|ref| {ref.abs().max().item():.3e}, "
          f"worst err - bound {worst:.3e}")
    assert ref.abs().sum() > 0
    assert worst <= 0, f"{what}: {worst:.3e} over the bound"


def _assert_bf16_bar(got, ref, what):
    err = (got.double().cpu() - ref).abs()
    lim = 2.0 ** -7 * ref.abs() + 1e-3 * ref.abs().max()
    worst = (err - lim).max().item()
    print(f"{what}: max|err| {err.max().item():.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert ref.abs().sum() > 0
    assert worst <= 0, f"{what}: {worst:.3e} over the bound"


def _gy(dy, cdtype):
    return dy.to(DEV).to(cdtype).contiguous(memory_format=torch.channels_last_3d)


def _launch_stem(d, gy, w, out_dtype):
    """dX inside a sentinel-filled buffer: (dx view, buffer, margin)"""
    lib = L.load()
    numel = d.n * d.di * d.hi * d.wi
    margin = 256
    buf = torch.full((numel + 2 * margin,), -777.0, dtype=out_dtype, device=DEV)
    dx = buf[margin:margin + numel]
    ws = torch.empty(lib.mmad_stem_dgrad_ws_bytes(d), dtype=torch.uint8, device=DEV)
    L.call("mmad_conv3d_dgrad_raw", d, L.BF16, L.ptr(gy), L.ptr(w), L.dtype_code(out_dtype),
           L.ptr(dx), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return dx.view(d.n, 1, d.di, d.hi, d.wi), buf, margin


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_dgrad_matches_float64(shape, out_dtype):
    d, w, dy, ref, mag = _operands(shape)
    assert L.load().mmad_stem_dgrad_ok(d, L.BF16, L.dtype_code(out_dtype)) == 1
    gy, wd = _gy(dy, torch.bfloat16), w.to(DEV)
    dx, buf, margin = _launch_stem(d, gy, wd, out_dtype)
    assert (buf[:margin] == -777.0).all() and (buf[-margin:] == -777.0).all()
    assert torch.isfinite(dx).all()
    _assert_f64_bar(dx, ref, mag, f"stem_dgrad {shape} {out_dtype}")
    again, buf2, _ = _launch_stem(d, gy, wd, out_dtype)
    assert torch.equal(buf, buf2)              # deterministic, margins included


def test_default_route_is_the_stem_kernel():
    shape = (1, 1, 9, 11, 13)
    d, w, dy, ref, mag = _operands(shape)
    gy, wd = _gy(dy, torch.bfloat16), w.to(DEV)
    a = V.raw_input_grad(d, gy, wd, torch.float64)
    b = V.raw_input_grad(d, gy, wd, torch.float64, route="stem")
    assert a.dtype == torch.float64 and tuple(a.shape) == shape
    assert torch.equal(a, b)
    _assert_f64_bar(a, ref, mag, "raw_input_grad default route")


GENERIC = [
    ((2, 1, 16, 16, 16), 64, 7, 2, 3),      # the stem through the generic route
    ((1, 1, 9, 11, 13), 64, 7, 2, 3),
    ((2, 1, 12, 12, 12), 8, 5, 1, 2),       # Small_PET_CNN conv 1: k5 'same', co 8
    ((2, 1, 12, 12, 12), 16, 7, 1, 3),      # k7 'same', co 16
]


@pytest.mark.parametrize("cdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape,co,k,stride,pad", GENERIC)
def test_generic_route(shape, co, k, stride, pad, cdtype):
    d, w, dy, ref, mag = _operands(shape, co, k, stride, pad)
    gy, wd = _gy(dy, cdtype), w.to(DEV)
    for out_dtype in (torch.float64, torch.float32):
        dx = V.raw_input_grad(d, gy, wd, out_dtype, route="generic")
        torch.cuda.synchronize()
        assert dx.dtype == out_dtype and tuple(dx.shape) == shape
        what = f"generic {shape} co {co} k {k} {cdtype} -> {out_dtype}"
        if cdtype == torch.bfloat16:
            _assert_bf16_bar(dx, ref, what)
        else:
            _assert_f64_bar(dx, ref, mag, what)
