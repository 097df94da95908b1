"""The z-walking layer1 conv (csrc/patchz.hip) runs its 27 taps in nine 3-tap stages with one
barrier each, over a 6-slot plane ring and a 3-slot weight-stage ring whose DMA waits are
counted by hand.  These are the smallest grids that reach every path of that loop:

  1 x 8 x 8 x 8     two boxes: the first (prologue planes, no predecessor) and the last (no
                    planes or weights issued past the segment's end) only
  1 x 12 x 8 x 8    three boxes: a middle box, and the ring base 0 -> 4 -> 2
  2 x 28 x 16 x 8   seven boxes (more than one period of the ring base), two y columns that
                    share a halo, two samples
  1 x 12 x 8 x 8, 128 output channels: two channel tiles per column

Each is one z segment (asserted by the stats row count).  Per case: forward and input gradient
are bit-identical to the per-box patch conv (variant 0: same K order per output element) and
within one bf16 rounding of an fp32 conv of the same bf16 operands (|err| <= 2^-7 |ref| + 1e-3
max|ref|); the BN partial-sum totals agree to fp32 rounding (1e-5 sum|y| + 1e-6; the rows
group different boxes); and two consecutive runs give the same bits -- a miscounted DMA wait
is a race, not a fault, and shows up there.  Plus the eval epilogue (residual + ReLU)."""
import pytest
import torch

from multimodal_alzheimer_amd import volume_ops as V
from tests._variants import variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last_3d
BF = torch.bfloat16

# (N, D, H, W, output channels)
CASES = [(1, 8, 8, 8, 64), (1, 12, 8, 8, 64), (2, 28, 16, 8, 64), (1, 12, 8, 8, 128)]
IDS = ["two_boxes", "three_boxes", "seven_boxes_two_columns", "two_channel_tiles"]


def _conv(x, w, gy=None):
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    y, stats = V.conv3d(xg, wg, None, (1,) * 3, (1,) * 3, (1,) * 3, BF, want_stats=True)
    if gy is None:
        g = torch.Generator(device=DEV).manual_seed(19)
        gy = (torch.rand(y.shape, generator=g, device=DEV) * 2 - 1).to(BF) \
            .contiguous(memory_format=CL)
    y.backward(gy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "stats": stats.detach().clone(), "dx": xg.grad, "dw": wg.grad,
            "gy": gy}


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def runs(request):
    """variant 0 once, variant 2 twice, the fp32 conv once; shared by the tests below"""
    from tests.test_fullsize_gpu import _ref_conv
    n, d, h, wd, co = request.param
    g = torch.Generator(device=DEV).manual_seed(d * 100 + h + n + co)
    x = (torch.rand((n, 64, d, h, wd), generator=g, device=DEV) * 2 - 1).to(BF) \
        .contiguous(memory_format=CL)
    w = (torch.rand((co, 64, 3, 3, 3), generator=g, device=DEV) * 2 - 1) * (3.0 / (64 * 27)) ** 0.5
    with variants(patchz=0):
        ref = _conv(x, w)
        with variants(patchz=2):
            got = _conv(x, w, ref["gy"])
            again = _conv(x, w, ref["gy"])
    xr = x.float().requires_grad_(True)
    wr = w.to(BF).float().requires_grad_(True)
    yr = _ref_conv(xr, wr, 1, 1, 1)
    yr.backward(ref["gy"].float())
    return {"shape": request.param, "ref": ref, "got": got, "again": again,
            "y32": yr.detach(), "dx32": xr.grad}


def _close(got, ref, name, rel=2 ** -7, absf=1e-3):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bound = rel * ref.abs() + absf * ref.abs().max()
    bad = int((err > bound).sum())
    assert bad == 0, f"{name}: {bad} beyond bound, max|err| {err.max().item():.3e}"


def test_routed_to_one_segment_of_4x8x8_boxes(runs):
    n, d, h, wd, _ = runs["shape"]
    assert runs["got"]["stats"].shape[0] == n * (d // 4) * (h // 8) * (wd // 8), \
        "not routed to the z-walking kernel"
    assert runs["ref"]["stats"].shape[0] == n * (d // 2) * (h // 8) * (wd // 8), \
        "variant 0 is not the per-box patch conv"


def test_bit_identical_to_patch_conv(runs):
    got, ref = runs["got"], runs["ref"]
    assert torch.equal(got["y"], ref["y"]), "forward differs"
    assert torch.equal(got["dx"], ref["dx"]), "input gradient differs"
    assert torch.equal(got["dw"], ref["dw"]), "weight gradient differs (same wgrad kernel)"


def test_within_bf16_rounding_of_fp32(runs):
    _close(runs["got"]["y"], runs["y32"], "forward vs fp32")
    _close(runs["got"]["dx"], runs["dx32"], "input gradient vs fp32")


def test_bn_partial_sum_totals(runs):
    y = runs["ref"]["y"].float()
    mag = torch.stack((y.abs().sum(dim=(0, 2, 3, 4)), (y * y).sum(dim=(0, 2, 3, 4))))
    got, ref = runs["got"]["stats"].sum(0), runs["ref"]["stats"].sum(0)
    assert ((got - ref).abs() <= 1e-5 * mag + 1e-6).all(), "BN partial-sum totals differ"


def test_two_runs_same_bits(runs):
    got, again = runs["got"], runs["again"]
    assert torch.equal(got["y"], again["y"]), "forward: two runs differ"
    assert torch.equal(got["dx"], again["dx"]), "input gradient: two runs differ"
    assert torch.equal(got["stats"], again["stats"]), "BN partial sums: two runs differ"


def test_eval_epilogue_residual_relu():
    from multimodal_alzheimer_amd import layers as Lyr
    torch.manual_seed(7)
    conv = Lyr.Conv3d(64, 64, 3, padding=1, bias=False).to(DEV)
    conv.compute_dtype = BF
    bn = torch.nn.BatchNorm3d(64).to(DEV).eval()
    with torch.no_grad():
        bn.running_var.uniform_(0.5, 2.0)
        bn.bias.uniform_(-0.3, 0.3)
    g = torch.Generator(device=DEV).manual_seed(8)
    shape = (1, 64, 12, 8, 8)
    x = (torch.rand(shape, generator=g, device=DEV) * 2 - 1).to(BF).contiguous(memory_format=CL)
    res = (torch.rand(shape, generator=g, device=DEV) * 2 - 1).to(BF).contiguous(memory_format=CL)
    with variants(patchz=0), torch.no_grad():
        ref = V.conv_bn_act_eval(x, conv, bn, relu=True, res=res)
        with variants(patchz=2):
            got = V.conv_bn_act_eval(x, conv, bn, relu=True, res=res)
            again = V.conv_bn_act_eval(x, conv, bn, relu=True, res=res)
        torch.cuda.synchronize()
    assert (ref > 0).any() and (ref == 0).any(), "the ReLU clips nothing or everything"
    assert torch.equal(got, ref)
    assert torch.equal(again, got)
