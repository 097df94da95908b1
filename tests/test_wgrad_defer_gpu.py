"""Deferred weight-gradient slab reductions (volume_ops.deferred_wgrad_reduce ->
mmad_conv3d_wgrad_deferred + mmad_wgrad_reduce_batch): every conv route of the benched
config-2 step, at its real geometry (batch 2), gives a dW bit-identical to the immediate
reduction -- the batched launch runs the same per-element sums in the same order -- and
several convs' reductions share one launch."""
import pytest
import torch

from multimodal_alzheimer_amd import _lib
from multimodal_alzheimer_amd import volume_ops as V
from tests._variants import variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last_3d
BF = torch.bfloat16

# (name, x shape, w shape, stride, padding, dilation): the routes of the ResNet-10 step
ROUTES = [
    ("layer4_conv2_lattice", (2, 512, 16, 16, 16), (512, 512, 3, 3, 3), 1, 4, 4),
    ("layer3_conv_pwgrad_lat", (2, 256, 16, 16, 16), (256, 256, 3, 3, 3), 1, 2, 2),
    ("layer2_conv2_pwgrad_w16", (2, 128, 16, 16, 16), (128, 128, 3, 3, 3), 1, 1, 1),
    ("layer1_pwgrad", (2, 64, 32, 32, 32), (64, 64, 3, 3, 3), 1, 1, 1),
    ("layer2_conv1_s2_generic", (2, 64, 32, 32, 32), (128, 64, 3, 3, 3), 2, 1, 1),
    ("layer4_downsample_wide", (2, 256, 16, 16, 16), (512, 256, 1, 1, 1), 1, 0, 1),
    ("layer3_downsample_wide", (2, 128, 16, 16, 16), (256, 128, 1, 1, 1), 1, 0, 1),
    ("layer2_downsample_s2", (2, 64, 32, 32, 32), (128, 64, 1, 1, 1), 2, 0, 1),
]


def _operands(xs, ws, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.rand(xs, generator=g, device=DEV) * 2 - 1).to(BF).contiguous(memory_format=CL)
    w = (torch.rand(ws, generator=g, device=DEV) * 2 - 1) * (3.0 / (ws[1] * ws[2] ** 3)) ** 0.5
    return x, w


def _wgrad(x, w, s, p, d, gy=None, defer=False):
    wg = w.clone().requires_grad_(True)
    y = V.conv3d(x, wg, None, (s,) * 3, (p,) * 3, (d,) * 3, BF)
    if gy is None:
        g = torch.Generator(device=DEV).manual_seed(5)
        gy = (torch.rand(y.shape, generator=g, device=DEV) * 2 - 1).to(BF) \
            .contiguous(memory_format=CL)
    with V.deferred_wgrad_reduce(defer):
        y.backward(gy)
        queued = len(V._WGRAD_DEFER["jobs"])
    torch.cuda.synchronize()
    return wg.grad, gy, queued


@pytest.mark.parametrize("name,xs,ws,s,p,d", ROUTES, ids=[r[0] for r in ROUTES])
def test_deferred_reduce_bit_identical(name, xs, ws, s, p, d):
    x, w = _operands(xs, ws, hash(name) % 1000)
    ref, gy, _ = _wgrad(x, w, s, p, d)
    got, _, queued = _wgrad(x, w, s, p, d, gy, defer=True)
    assert queued <= 1
    assert torch.equal(got, ref), f"{name}: max |diff| {(got - ref).abs().max().item():.3e}"


def test_many_convs_one_batch():
    """all routes queued, then one flush: each dW equals its immediate reduction"""
    refs, gys, xs_ws = [], [], []
    for i, (name, xs, ws, s, p, d) in enumerate(ROUTES):
        x, w = _operands(xs, ws, 100 + i)
        r, gy, _ = _wgrad(x, w, s, p, d)
        refs.append(r)
        gys.append(gy)
        xs_ws.append((x, w))
    wgs = []
    with V.deferred_wgrad_reduce(True):
        for (x, w), gy, (name, _, _, s, p, d) in zip(xs_ws, gys, ROUTES):
            wg = w.clone().requires_grad_(True)
            V.conv3d(x, wg, None, (s,) * 3, (p,) * 3, (d,) * 3, BF).backward(gy)
            wgs.append(wg)
        n = len(V._WGRAD_DEFER["jobs"])
    torch.cuda.synchronize()
    assert n >= 6, "expected most routes to queue a reduction"
    for (name, *_), wg, r in zip(ROUTES, wgs, refs):
        assert torch.equal(wg.grad, r), name


def test_reduce_batch_rejects_bad_jobs():
    lib = _lib.load()
    job = _lib.WgradJob()
    job.kind, job.gx, job.gy, job.gz = 1, 1, 1, 1       # ws / dw left NULL
    assert lib.mmad_wgrad_reduce_batch(1, job, None) == 1003
    assert lib.mmad_wgrad_reduce_batch(0, None, None) == 0


@pytest.mark.parametrize("xs,co,s", [((2, 256, 16, 16, 16), 512, 1), ((2, 128, 16, 16, 16), 256, 1),
                                     ((2, 64, 32, 32, 32), 128, 2), ((1, 256, 8, 12, 10), 128, 1),
                                     ((3, 64, 9, 8, 7), 128, 2)],
                         ids=["layer4_ds", "layer3_ds", "layer2_ds_s2", "ragged", "ragged_s2"])
def test_pointwise_wgrad_vs_float64(xs, co, s):
    """the 1x1x1 weight gradient (pointwise.hip pw_wgrad_kernel + wide slab reduction)
    against a float64 sum over the same bf16 operands: within 1e-3 |ref| + 1e-4 sum|gY||X|"""
    x, w = _operands(xs, (co, xs[1], 1, 1, 1), 7)
    got, gy, _ = _wgrad(x, w, s, 0, 1)
    xd = x.double()[:, :, ::s, ::s, ::s]
    gd = gy.double()
    ref = torch.einsum("nczyx,nkzyx->ck", gd, xd)
    mag = torch.einsum("nczyx,nkzyx->ck", gd.abs(), xd.abs())
    err = (got.double().reshape(ref.shape) - ref).abs()
    assert (err <= 1e-3 * ref.abs() + 1e-4 * mag).all(), f"max err {err.max().item():.3e}"


@pytest.mark.parametrize("xs,co", [((2, 64, 32, 32, 32), 128), ((2, 64, 15, 16, 16), 128),
                                   ((1, 128, 16, 16, 16), 256), ((3, 64, 10, 32, 31), 128)],
                         ids=["layer2_conv1", "odd_depth", "wide_ci", "rows16_ragged"])
def test_stride2_3cube_wgrad_vs_float64(xs, co):
    """the stride-2 3^3 weight gradient (pw_wgrad_kernel's 3-tap form + transposing slab
    reduction; layer2.0.conv1) against torch's float64 weight gradient of the same bf16
    operands: within 1e-3 |ref| + 1e-4 sum |gY| |X|"""
    x, w = _operands(xs, (co, xs[1], 3, 3, 3), 11)
    got, gy, _ = _wgrad(x, w, 2, 1, 1)
    xd, gd = x.double(), gy.double()
    ref = torch.nn.grad.conv3d_weight(xd, w.shape, gd, 2, 1, 1)
    mag = torch.nn.grad.conv3d_weight(xd.abs(), w.shape, gd.abs(), 2, 1, 1)
    err = (got.double() - ref).abs()
    assert (err <= 1e-3 * ref.abs() + 1e-4 * mag).all(), f"max err {err.max().item():.3e}"


def test_deferred_stem_reduce_bit_identical():
    """the MedicalNet stem's weight gradient straight from the raw f64 volume (7^3 / 2, the
    bench's 128^3 at batch 2): its two-level slab sum deferred into the batched launch is
    bit-identical to the immediate one"""
    from multimodal_alzheimer_amd import layers as Lyr
    torch.manual_seed(5)
    conv = Lyr.Conv3d(1, 64, 7, stride=2, padding=3, bias=False).to(DEV)
    conv.compute_dtype = BF
    g = torch.Generator(device=DEV).manual_seed(6)
    vol = torch.rand((2, 1, 128, 128, 128), generator=g, device=DEV, dtype=torch.float64)
    grads = []
    for defer in (False, True):
        conv.weight.grad = None
        y = conv(vol)
        gy = (torch.rand(y.shape, generator=torch.Generator(device=DEV).manual_seed(7),
                         device=DEV) * 2 - 1).to(BF).contiguous(memory_format=CL)
        with V.deferred_wgrad_reduce(defer):
            y.backward(gy)
            queued = len(V._WGRAD_DEFER["jobs"])
        torch.cuda.synchronize()
        assert queued == (1 if defer else 0)
        grads.append(conv.weight.grad.clone())
    assert torch.equal(grads[0], grads[1])



@pytest.mark.parametrize("xs,co", [((2, 64, 32, 32, 32), 128), ((3, 64, 10, 32, 31), 128),
                                   ((1, 64, 6, 4, 32), 128), ((1, 64, 9, 31, 32), 128)],
                         ids=["layer2_conv1", "rows16_ragged", "two_rows", "odd_height"])
def test_stride2_3cube_wgrad_dedup_bit_identical(xs, co):
    """16-wide output rows: the de-duplicated X-row form of the stride-2 3^3 weight gradient
    (pw_wgrad_kernel MODE 4: the even input columns and the 17 odd ones of each output row
    staged once, read by kx = 1 and by kx = 0 / 2 at a one-row offset) gives exactly the
    three-image form's dW (MODE 2): the same voxel pairs summed in the same order."""
    x, w = _operands(xs, (co, xs[1], 3, 3, 3), 13)
    with variants(pw_wg3_dedup=0):
        ref, gy, _ = _wgrad(x, w, 2, 1, 1)
        with variants(pw_wg3_dedup=1):
            got, _, _ = _wgrad(x, w, 2, 1, 1, gy)
    assert torch.equal(got, ref), f"max |diff| {(got - ref).abs().max().item():.3e}"


def test_hooked_weight_is_not_deferred():
    """a tensor hook on the weight reads dW during the backward, before any flush: such a
    weight keeps the immediate reduction (bit-identical dW, the hook sees the final dW)"""
    name, xs, ws, s, p, d = ROUTES[0]
    x, w = _operands(xs, ws, 21)
    ref, gy, _ = _wgrad(x, w, s, p, d)
    wg = w.clone().requires_grad_(True)
    seen = []
    wg.register_hook(lambda g: seen.append(g.clone()))
    y = V.conv3d(x, wg, None, (s,) * 3, (p,) * 3, (d,) * 3, BF)
    with V.deferred_wgrad_reduce(True):
        y.backward(gy)
        queued = len(V._WGRAD_DEFER["jobs"])
    torch.cuda.synchronize()
    assert queued == 0
    assert torch.equal(wg.grad, ref) and torch.equal(seen[0], ref)


def test_summed_deferred_gradient_raises():
    """a weight used by two convs gets the SUM of two deferred dWs, computed by autograd
    before the flush: the adoption check refuses it instead of returning garbage"""
    name, xs, ws, s, p, d = ROUTES[0]
    x, w = _operands(xs, ws, 22)
    wg = w.clone().requires_grad_(True)
    y = V.conv3d(x, wg, None, (s,) * 3, (p,) * 3, (d,) * 3, BF)
    y2 = V.conv3d(x, wg, None, (s,) * 3, (p,) * 3, (d,) * 3, BF)
    gy = torch.ones_like(y)
    with pytest.raises(RuntimeError, match="not adopted"):
        with V.deferred_wgrad_reduce(True):
            torch.autograd.backward([y, y2], [gy, gy])
    torch.cuda.synchronize()
    assert not V._WGRAD_DEFER["jobs"] and not V._WGRAD_DEFER["adopt"]

