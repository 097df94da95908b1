"""Host side of the stem input gradient (mmad_conv3d_dgrad_raw): where the kernel applies,
its workspace query and its operand checks.  Nothing is launched here (no GPU needed)."""
import os

import pytest

from multimodal_alzheimer_amd import _lib
from multimodal_alzheimer_amd.volume_ops import conv_desc

STEM_W = (64, 1, 7, 7, 7)


def stem_desc(shape, wshape=STEM_W, stride=2, pad=3):
    return conv_desc(shape, wshape, (stride,) * 3, (pad,) * 3, (1, 1, 1))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from multimodal_alzheimer_amd import _build
        _build.build()
    return _lib.load()


@pytest.mark.parametrize("shape", [(8, 1, 128, 128, 128), (2, 1, 160, 160, 160),
                                   (2, 1, 91, 109, 91)])
@pytest.mark.parametrize("out_dtype", [_lib.F32, _lib.F64])
def test_stem_geometry_is_covered(lib, shape, out_dtype):
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape), _lib.BF16, out_dtype) == 1


def test_other_geometries_are_declined(lib):
    shape = (2, 1, 32, 32, 32)
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape), _lib.BF16, _lib.F64) == 1
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape, (64, 1, 3, 3, 3), 2, 1), _lib.BF16,
                                  _lib.F64) == 0                       # 3^3 conv
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape, stride=1), _lib.BF16, _lib.F64) == 0
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape, (32, 1, 7, 7, 7)), _lib.BF16, _lib.F64) == 0
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape), _lib.F32, _lib.F64) == 0
    assert lib.mmad_stem_dgrad_ok(stem_desc(shape), _lib.BF16, _lib.BF16) == 0
    assert lib.mmad_stem_dgrad_ok(None, _lib.BF16, _lib.F64) == 0


def test_workspace_query(lib):
    for shape in ((8, 1, 128, 128, 128), (1, 1, 9, 11, 13)):
        n = lib.mmad_stem_dgrad_ws_bytes(stem_desc(shape))
        assert n > 0 and n % 16 == 0


def test_bad_operands_are_rejected_without_launching(lib):
    d = stem_desc((2, 1, 16, 16, 16))
    f = lib.mmad_conv3d_dgrad_raw
    # the pointer values are never dereferenced here
    assert f(d, _lib.BF16, None, 0x2000, _lib.F64, 0x3000, 0x4000, None) == 1003
    assert f(d, _lib.BF16, 0x1000, None, _lib.F64, 0x3000, 0x4000, None) == 1003
    assert f(d, _lib.BF16, 0x1000, 0x2000, _lib.F64, None, 0x4000, None) == 1003
    assert f(d, _lib.BF16, 0x1000, 0x2000, _lib.F64, 0x3000, None, None) == 1003
    assert f(d, _lib.BF16, 0x1008, 0x2000, _lib.F64, 0x3000, 0x4000, None) == 1001
    assert f(d, _lib.BF16, 0x1000, 0x2004, _lib.F64, 0x3000, 0x4000, None) == 1001
    assert f(d, _lib.BF16, 0x1000, 0x2000, _lib.F32, 0x3004, 0x4000, None) == 1001
    assert f(d, _lib.BF16, 0x1000, 0x2000, _lib.F64, 0x3000, 0x4002, None) == 1001
    assert f(d, 7, 0x1000, 0x2000, _lib.F64, 0x3000, 0x4000, None) == 1002
    assert f(d, _lib.BF16, 0x1000, 0x2000, _lib.BF16, 0x3000, 0x4000, None) == 1002
    # a geometry (or compute dtype) the kernel does not cover is refused, not launched
    assert f(d, _lib.F32, 0x1000, 0x2000, _lib.F64, 0x3000, 0x4000, None) == 1004
    d3 = stem_desc((2, 1, 16, 16, 16), (64, 1, 3, 3, 3), 2, 1)
    assert f(d3, _lib.BF16, 0x1000, 0x2000, _lib.F64, 0x3000, 0x4000, None) == 1004
    g = lib.mmad_take_channel
    assert g(_lib.BF16, 64, 8, 0, None, _lib.F64, 0x3000, None) == 1003
    assert g(_lib.BF16, 64, 8, 0, 0x1004, _lib.F64, 0x3000, None) == 1001
    assert g(_lib.BF16, 64, 8, 8, 0x1000, _lib.F64, 0x3000, None) == 1001
    assert g(_lib.F64, 64, 8, 0, 0x1000, _lib.F64, 0x3000, None) == 1002
