"""Host-side pin of the conv routing (no GPU, nothing is launched): the shape queries Python
sizes its buffers from reproduce tests/golden/conv_routes.json exactly, under the default
kernel-variant setting and under every run-time override, and a fused dgrad + BN-sum call is
refused wherever the kernel that would run the conv has no such epilogue."""
import importlib.util
import json
import os

import pytest

from multimodal_alzheimer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location(
        "make_conv_routes_golden", os.path.join(GOLDEN, "make_conv_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from multimodal_alzheimer_amd import _build
        _build.build()
    return _lib.load()


def test_routes_match_snapshot(lib):
    maker = _maker()
    with open(os.path.join(GOLDEN, "conv_routes.json")) as f:
        want = json.load(f)
    assert tuple(want["fields"]) == maker.FIELDS
    got = maker.snapshot(lib)
    assert sorted(got) == sorted(want["routes"])
    for label, rows in want["routes"].items():
        assert got[label] == rows, f"setting {label}"
    # the table is complete and the snapshot sees the routes: both dtypes of every case, and
    # overrides that move entries
    assert len(want["routes"]["default"]) == 2 * len(maker.cases())
    assert sum(1 for label, rows in want["routes"].items() if label != "default" and rows) >= 9


REFUSED = [
    # (variant, conv arguments): forced onto a kernel without the BN-sum epilogue
    ("patchz", ((8, 64, 32, 32, 32), (64, 64, 3, 3, 3), (1,) * 3, (1,) * 3, (1,) * 3)),
    ("lattice", ((2, 512, 23, 28, 23), (512, 512, 3, 3, 3), (1,) * 3, (4,) * 3, (4,) * 3)),
    ("lattice5", ((1, 512, 20, 20, 20), (512, 512, 3, 3, 3), (1,) * 3, (4,) * 3, (4,) * 3)),
]


@pytest.mark.parametrize("variant,args", REFUSED, ids=[r[0] for r in REFUSED])
def test_bnsum_refused_where_the_kernel_has_no_such_epilogue(lib, variant, args):
    """the z-walking patch conv, the ragged residue-class conv and the 5d^3 one write no
    BN-backward sums: the row query says -1 and the call returns MMAD_EUNSUPPORTED instead of
    launching a kernel that would leave the partial buffer unwritten (fake aligned pointers,
    never dereferenced)"""
    from multimodal_alzheimer_amd.volume_ops import conv_desc
    d = conv_desc(*args)
    prev = lib.mmad_set_kernel_variant(variant.encode(), 2)
    try:
        assert lib.mmad_conv3d_dgrad_bnsum_rows(d, _lib.BF16) == -1
        ptrs = [0x1000 * (i + 1) for i in range(9)]
        assert lib.mmad_conv3d_dgrad_bnsum(d, _lib.BF16, *ptrs, None) == _lib.EUNSUPPORTED
    finally:
        lib.mmad_set_kernel_variant(variant.encode(), prev)
