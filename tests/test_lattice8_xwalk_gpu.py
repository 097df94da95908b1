"""lattice8.hip's x-walk form (the exact 16^3 grid's y-pair fragments walked along x,
mmad_set_kernel_variant("lattice8_xwalk", 1)) against the x-pair form it replaces (0), which
the ragged grids still run.

Per output element both forms add the same 32-channel MFMAs in the same (chunk, kz, ky, kx)
order -- they differ in which all-zero padding products they execute -- and the BN partial
rows are added in the same order, so everything is compared with torch.equal:

  * forward with BN partial rows (output and both rows), forward with bias + residual +
    ReLU, the input gradient (mmad_conv3d_dgrad) and the input gradient with the BN-sum
    epilogue (output and its partial rows), on random normal bf16 operands;
  * the new form against an fp32 torch conv3d of the bf16-rounded operands, at
    test_kernels_gpu.test_conv3d_fwd_bwd's bf16 bounds (1.2e-2 forward, 2e-2 dX);
  * a ragged 12 x 14 x 12 grid gives the same bits with the variant on and off.

Shapes (kernel input channels Cs, output channels Nd), "lattice8" forced to 2: at batch 1
every tile is 32 channels wide (one 16-column MFMA tile per wave: 64-channel tiles are
taken only when they give every CU a block), 8 z-planes = 8 tiles a column tile with both
z-edge kinds; Cs 64 is two 32-channel chunks (both ring slots), Cs 128 four; Nd 64 at batch
1 is two column tiles.  The 64-channel tiles (two MFMA column tiles per wave) need 256 of
them: batch 32 at Cs 64, Nd 64.

Cs 32 (one chunk) cannot reach the kernel: the packed weight rows are padded to a multiple
of 64 (27 * 32 = 864 -> 896), and lattice8's ok() wants them unpadded, so such a conv runs
the implicit GEMM whatever the variant says.  The case stays as a check of exactly that:
not routed, and the same bits with the variant on and off."""
import functools

import pytest
import torch
import torch.nn.functional as F

from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import volume_ops as V
from tests._variants import variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last_3d
BF = torch.bfloat16

# name: (batch, Cs, Nd)
CASES = {
    "cs64_nd64": (1, 64, 64),
    "cs64_nd32": (1, 64, 32),
    "cs128_nd32": (1, 128, 32),
    "cs64_nd64_wide": (32, 64, 64),
}
GRID = (16, 16, 16)


def _vol(g, n, c, grid=GRID):
    return torch.randn((n, c) + grid, generator=g, device=DEV).to(BF).contiguous(memory_format=CL)


def _launches(n, cs, nd, grid, seed, routed=True):
    """every launch of one shape under the current variant -> dict of outputs
    (routed = False: a shape the kernel does not take; no BN-sum epilogue then)"""
    lib = L.load()
    dt = L.dtype_code(BF)
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    # forward: Cs -> Nd
    x = _vol(g, n, cs, grid)
    w = torch.randn((nd, cs, 3, 3, 3), generator=g, device=DEV) * (3.0 / (cs * 27)) ** 0.5
    bias = torch.randn(nd, generator=g, device=DEV)
    res = _vol(g, n, nd, grid)
    d = V.conv_desc((n, cs) + grid, tuple(w.shape), (1,) * 3, (2,) * 3, (2,) * 3)
    planes = (grid[0] + 1) // 2
    rows = lib.mmad_conv3d_stats_rows(d, dt)
    assert (rows == n * planes) == routed, "route to the residue-class kernel"
    wp = V.pack_weight(d, dt, w, BF, False)
    y = torch.empty_like(res)
    stats = torch.empty((rows, 2, nd), device=DEV)
    L.call("mmad_conv3d_fwd", d, dt, L.ptr(x), L.ptr(wp), None, L.ptr(y), L.ptr(stats),
           L.stream())
    y2 = torch.empty_like(res)
    L.call("mmad_conv3d_fwd_ex", d, dt, L.ptr(x), L.ptr(wp), L.ptr(bias), L.ptr(res), 1,
           L.ptr(y2), None, L.stream())
    # input gradient of a conv Nd -> Cs: the kernel again reads Cs channels and writes Nd
    gy = _vol(g, n, cs, grid)
    wb = torch.randn((cs, nd, 3, 3, 3), generator=g, device=DEV) * (3.0 / (cs * 27)) ** 0.5
    db = V.conv_desc((n, nd) + grid, tuple(wb.shape), (1,) * 3, (2,) * 3, (2,) * 3)
    wpt = V.pack_weight(db, dt, wb, BF, True)
    dx = torch.empty_like(res)
    L.call("mmad_conv3d_dgrad", db, dt, L.ptr(gy), L.ptr(wpt), L.ptr(dx), L.stream())
    out.update(x=x, w=w, y=y, stats=stats, y_epi=y2, gy=gy, wb=wb, dx=dx)
    if not routed:
        torch.cuda.synchronize()
        return out
    brows = lib.mmad_conv3d_dgrad_bnsum_rows(db, dt)
    assert brows == n * planes, "dgrad not routed to the residue-class kernel"
    yb = _vol(g, n, nd, grid)
    sc = torch.rand(nd, generator=g, device=DEV) + 0.5
    sh = torch.randn(nd, generator=g, device=DEV) * 0.3
    mu = torch.randn(nd, generator=g, device=DEV) * 0.1
    ist = torch.rand(nd, generator=g, device=DEV) + 0.5
    dx2 = torch.empty_like(res)
    parts = torch.empty((brows, 2, nd), device=DEV)
    L.call("mmad_conv3d_dgrad_bnsum", db, dt, L.ptr(gy), L.ptr(wpt), L.ptr(dx2), L.ptr(yb),
           L.ptr(sc), L.ptr(sh), L.ptr(mu), L.ptr(ist), L.ptr(parts), L.stream())
    torch.cuda.synchronize()
    out.update(dx_bn=dx2, parts=parts)
    return out


def _on_off(n, cs, nd, grid, seed, routed):
    """the launches of one shape with the variant off (x-pair form), then on (x-walk)"""
    with variants(lattice8=2, lattice8_xwalk=0) as prev:
        assert prev["lattice8_xwalk"] in (0, 1), "unknown variant name"
        off = _launches(n, cs, nd, grid, seed, routed)
        with variants(lattice8_xwalk=1):
            on = _launches(n, cs, nd, grid, seed, routed)
    return off, on


@functools.lru_cache(maxsize=None)
def _both(name):
    """(x-pair form, x-walk form) outputs of one case, computed once"""
    n, cs, nd = CASES[name]
    return _on_off(n, cs, nd, GRID, 11, True)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_bn_rows_keep_their_bits(name):
    old, new = _both(name)
    assert torch.equal(old["x"], new["x"]) and torch.equal(old["w"], new["w"])
    assert torch.isfinite(new["y"].float()).all() and new["y"].float().abs().max() > 0.5
    assert torch.equal(new["y"], old["y"])
    assert torch.equal(new["stats"][:, 0], old["stats"][:, 0])
    assert torch.equal(new["stats"][:, 1], old["stats"][:, 1])


@pytest.mark.parametrize("name", list(CASES))
def test_forward_bias_residual_relu_keeps_its_bits(name):
    old, new = _both(name)
    assert (new["y_epi"] == 0).any() and (new["y_epi"] > 0).any()
    assert torch.equal(new["y_epi"], old["y_epi"])


@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_keeps_its_bits(name):
    old, new = _both(name)
    assert new["dx"].float().abs().max() > 0.5
    assert torch.equal(new["dx"], old["dx"])


@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_bnsum_keeps_its_bits(name):
    old, new = _both(name)
    assert torch.equal(new["dx_bn"], new["dx"])
    assert torch.equal(new["dx_bn"], old["dx_bn"])
    assert torch.equal(new["parts"], old["parts"])


def _close(got, ref, rtol, what):
    err = (got.double() - ref.double()).abs().max().item()
    scale = ref.double().abs().max().item() + 1e-12
    print(f"{what}: max|err| {err:.3e}, bound {rtol:.1e} * {scale:.3e}")
    assert err <= rtol * scale, f"{what}: max|err| {err:.3e} > {rtol:.1e} * {scale:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_new_form_against_fp32_conv3d(name):
    _, new = _both(name)
    ref = F.conv3d(new["x"].float(), new["w"].to(BF).float(), None, 1, 2, 2)
    _close(new["y"], ref, 1.2e-2, "y")
    # dX of y = conv(x, wb): conv_transpose of gy by the same weights
    refdx = F.conv_transpose3d(new["gy"].float(), new["wb"].to(BF).float(), None, 1, 2,
                               dilation=2)
    _close(new["dx"], refdx, 2e-2, "dx")


def test_ragged_grid_stays_on_the_x_pair_form():
    off, on = _on_off(1, 64, 64, (12, 14, 12), 12, True)
    for k in ("y", "stats", "y_epi", "dx", "dx_bn", "parts"):
        assert torch.equal(on[k], off[k]), k


def test_one_chunk_convs_are_not_the_kernels():
    off, on = _on_off(1, 32, 32, GRID, 13, False)
    for k in ("y", "stats", "y_epi", "dx"):
        assert torch.equal(on[k], off[k]), k
