"""Device augmentation (multimodal_alzheimer_amd.augment) against torch on the CPU in float64:
``F.affine_grid`` + ``F.grid_sample(mode='bilinear', align_corners=False)`` is the oracle of
the resample, the drawn parameters are checked for what they must be (a scaled rotation with
flips, everything inside its range, the right frequencies), and the augmenter is followed
through a captured graph and a model's ``general_step``.

Bar of every comparison with the oracle: max|got - ref| <= 1e-12 * max|ref| (the project's
bar for float64 kernels whose operation order differs from torch's)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib, augment
from multimodal_alzheimer_amd.graph_step import GraphedTrainStep
from tests import _golden as G

pytestmark = pytest.mark.gpu

RTOL = 1e-12
SHAPES = [(2, 9, 11, 13), (3, 16, 16, 16), (1, 5, 7, 67)]


def oracle(x, theta, padding, gain_bias=None):
    """x (B, D, H, W), theta (B, 3, 4), gain_bias (B, 2): CPU float64 tensors."""
    grid = F.affine_grid(theta, (x.shape[0], 1) + tuple(x.shape[1:]), align_corners=False)
    y = F.grid_sample(x[:, None], grid, mode="bilinear", padding_mode=padding,
                      align_corners=False)[:, 0]
    if gain_bias is not None:
        y = gain_bias[:, 0, None, None, None] * y + gain_bias[:, 1, None, None, None]
    return y


def assert_close(got, ref, what=""):
    err = (got.cpu() - ref).abs().max().item()
    bar = RTOL * ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e}, bar {bar:.3e}")
    assert err <= bar, f"{what}: max|err| {err:.3e} > {bar:.3e}"


def rotation(ax, ay, az):
    """Rz Ry Rx over (x, y, z)"""
    def rot(i, j, a):
        r = torch.eye(3, dtype=torch.float64)
        r[i, i] = r[j, j] = math.cos(a)
        r[i, j], r[j, i] = -math.sin(a), math.sin(a)
        return r
    return rot(0, 1, az) @ rot(2, 0, ay) @ rot(1, 2, ax)


def fixed_thetas():
    a = torch.cat([0.9 * rotation(0.1, 0.2, 0.3),
                   torch.tensor([[0.2], [-0.1], [0.15]], dtype=torch.float64)], 1)
    lin = 1.07 * rotation(0.3, 0.1, 0.2)
    lin[:, 0] = -lin[:, 0]                                   # x flip
    b = torch.cat([lin, torch.tensor([[-0.05], [0.2], [0.1]], dtype=torch.float64)], 1)
    return a, b


def volume(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def diag_theta(b, sx=1.0, sy=1.0, sz=1.0, t=(0.0, 0.0, 0.0)):
    th = torch.zeros((b, 3, 4), dtype=torch.float64)
    th[:, 0, 0], th[:, 1, 1], th[:, 2, 2] = sx, sy, sz
    th[:, :, 3] = torch.tensor(t, dtype=torch.float64)
    return th


# ------------------------------------------------------------------ 1. resample vs grid_sample
@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_resample_matches_grid_sample(shape, first, padding):
    x = volume(shape, 11)
    thetas = fixed_thetas()
    theta = torch.stack([thetas[(n + first) % 2] for n in range(shape[0])])
    got = augment.resample(x.cuda(), theta.cuda(), padding)
    assert_close(got, oracle(x, theta, padding), f"{shape} theta{first} {padding}")


# ------------------------------------------------------------------------- 2. out of bounds
def test_translation_past_the_volume():
    x = volume((2, 9, 11, 13), 12)
    theta = diag_theta(2, t=(2.5, 0.0, 0.0))                # 1.25 volumes along x
    theta[1, :, 3] = torch.tensor([0.0, -2.2, 2.1])
    assert oracle(x, theta, "zeros").abs().max().item() == 0.0
    got = augment.resample(x.cuda(), theta.cuda(), "zeros")
    assert torch.count_nonzero(got).item() == 0
    got = augment.resample(x.cuda(), theta.cuda(), "border")
    assert_close(got, oracle(x, theta, "border"), "border, translated out")


@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("lin", [2.0, 0.5])                  # output-to-input: zoom out, zoom in
def test_scale_by_two(lin, padding):
    x = volume((2, 9, 11, 13), 13)
    theta = diag_theta(2, lin, lin, lin)
    got = augment.resample(x.cuda(), theta.cuda(), padding)
    assert_close(got, oracle(x, theta, padding), f"lin {lin} {padding}")


# ----------------------------------------------------------------------------- 3. exact path
FLIPS = [(), (3,), (2,), (1,), (1, 2, 3)]


@pytest.mark.parametrize("dims", FLIPS)
def test_flips_are_bit_exact(dims):
    x = volume((2, 5, 7, 67), 14).cuda()
    sign = [-1.0 if d in dims else 1.0 for d in (3, 2, 1)]   # x = W, y = H, z = D
    theta = diag_theta(2, *sign).cuda()
    flipped = torch.flip(x, dims) if dims else x
    for padding in ("zeros", "border"):
        got = augment.resample(x, theta, padding)
        assert got.data_ptr() != x.data_ptr()
        assert torch.equal(got, flipped)
    gb = torch.tensor([[1.3, -0.2], [0.7, 0.45]], dtype=torch.float64, device="cuda")
    got = augment.resample(x, theta, "zeros", gb)
    assert torch.equal(got, gb[:, 0, None, None, None] * flipped + gb[:, 1, None, None, None])


def test_mixed_batch_takes_the_exact_path_per_sample():
    x = volume((2, 9, 11, 13), 15)
    theta = torch.stack([diag_theta(1, -1.0)[0], fixed_thetas()[0]])
    got = augment.resample(x.cuda(), theta.cuda(), "zeros")
    assert torch.equal(got[0].cpu(), torch.flip(x[0], (2,)))
    assert_close(got[1:], oracle(x[1:], theta[1:], "zeros"), "second sample")


def test_gradient_request_raises():
    x = torch.zeros((1, 4, 4, 4), dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(_lib.MMADError, match="backward"):
        augment.resample(x, diag_theta(1).cuda())


# ---------------------------------------------------------------------------------- 4. draw
B, EXTENT = 4096, (91, 109, 91)                              # (D, H, W)
DRAW_CFG = {"flip_p": 0.5, "rotate_deg": [10.0, 15.0, 20.0], "scale": [0.9, 1.1],
            "translate_vox": [3.0, 4.0, 5.0],
            "gain": {"mri": [0.9, 1.1], "pet1451": [0.8, 1.0]},
            "bias": {"mri": [-0.1, 0.1], "pet1451": [0.0, 0.2]}}
SLACK = 1e-12                                                # rounding of the unit conversions


def voxel_affine(theta, extent=EXTENT):
    """A = N^-1 theta_lin N and t in voxels, over (x, y, z) = (W, H, D)"""
    size = torch.tensor([extent[2], extent[1], extent[0]], dtype=torch.float64)
    a = theta[:, :, :3] * size[None, :, None] / size[None, None, :]
    return a, theta[:, :, 3] * size[None, :] / 2


def in_range_with_centred_mean(v, lo, hi, what):
    assert v.min().item() >= lo - SLACK and v.max().item() <= hi + SLACK, what
    sigma = (hi - lo) / math.sqrt(12 * v.numel())
    assert abs(v.mean().item() - (lo + hi) / 2) <= 5 * sigma, what
    assert v.std().item() > 0.2 * (hi - lo), what            # uniform: 0.289 of the range


@pytest.fixture(scope="module")
def drawn():
    torch.manual_seed(21)
    theta, intensity = augment.draw(DRAW_CFG, B, EXTENT, "cuda", nmod=2)
    assert theta.shape == (B, 3, 4) and intensity.shape == (B, 2, 2)
    return theta.cpu(), intensity.cpu()


def test_draw_is_a_scaled_rotation_with_flips(drawn):
    a, _ = voxel_affine(drawn[0])
    aat = a @ a.transpose(1, 2)
    s2 = aat.diagonal(dim1=1, dim2=2).mean(1)
    eye = torch.eye(3, dtype=torch.float64)
    assert (aat - s2[:, None, None] * eye).abs().max().item() <= 1e-12
    in_range_with_centred_mean(s2.sqrt(), 0.9, 1.1, "scale")
    # angles <= 20 degrees keep the rotation's diagonal positive: the flips are its signs
    flips = a.diagonal(dim1=1, dim2=2).sign()
    assert torch.equal(torch.linalg.det(a).sign(), flips.prod(1))
    freq = (flips < 0).double().mean(0)
    assert (freq - 0.5).abs().max().item() <= 0.04, freq     # 5 sigma, sigma = 0.0078
    # Euler angles of R = A diag(flips) / s = Rz Ry Rx: x = w, y = h, z = d
    r = a * flips[:, None, :] / s2.sqrt()[:, None, None]
    deg = math.pi / 180
    in_range_with_centred_mean(torch.atan2(r[:, 2, 1], r[:, 2, 2]), -20 * deg, 20 * deg, "about w")
    in_range_with_centred_mean(torch.asin(-r[:, 2, 0]), -15 * deg, 15 * deg, "about h")
    in_range_with_centred_mean(torch.atan2(r[:, 1, 0], r[:, 0, 0]), -10 * deg, 10 * deg, "about d")


def test_draw_translation_and_intensity_ranges(drawn):
    theta, intensity = drawn
    _, t = voxel_affine(theta)
    for axis, tmax in ((0, 5.0), (1, 4.0), (2, 3.0)):        # x = w, y = h, z = d
        in_range_with_centred_mean(t[:, axis], -tmax, tmax, f"translation {axis}")
    in_range_with_centred_mean(intensity[:, 0, 0], 0.9, 1.1, "mri gain")
    in_range_with_centred_mean(intensity[:, 0, 1], -0.1, 0.1, "mri bias")
    in_range_with_centred_mean(intensity[:, 1, 0], 0.8, 1.0, "pet gain")
    in_range_with_centred_mean(intensity[:, 1, 1], 0.0, 0.2, "pet bias")
    # the quantities are drawn independently of each other
    c = torch.corrcoef(torch.stack([t[:, 0], t[:, 1], t[:, 2], intensity[:, 0, 0],
                                    intensity[:, 1, 0], intensity[:, 0, 1]]))
    assert (c - torch.eye(6, dtype=torch.float64)).abs().max().item() <= 5 / math.sqrt(B)


def test_flip_probability_zero_and_one_and_axis_order():
    for p, axis in (([1.0, 0.0, 0.0], 2), ([0.0, 1.0, 0.0], 1), ([0.0, 0.0, 1.0], 0)):
        theta, intensity = augment.draw({"flip_p": p}, 256, EXTENT, "cuda")
        theta = theta.cpu()
        want = torch.zeros((256, 3, 4), dtype=torch.float64)  # exactly a flip: the exact path
        want[:, 0, 0] = want[:, 1, 1] = want[:, 2, 2] = 1.0
        want[:, axis, axis] = -1.0                            # p = 1 always, p = 0 never
        assert torch.equal(theta, want)
        assert torch.equal(intensity.cpu(), torch.tensor([1.0, 0.0]).double().expand(256, 1, 2))


def test_draw_follows_the_torch_seed(drawn):
    torch.manual_seed(21)
    theta, intensity = augment.draw(DRAW_CFG, B, EXTENT, "cuda", nmod=2)
    assert torch.equal(theta.cpu(), drawn[0]) and torch.equal(intensity.cpu(), drawn[1])
    theta2, intensity2 = augment.draw(DRAW_CFG, B, EXTENT, "cuda", nmod=2)
    assert not torch.equal(theta2, theta) and not torch.equal(intensity2, intensity)


# ---------------------------------------------------------------------- 5. paired modalities
AUG_CFG = {"flip_p": [0.5, 0.5, 0.5], "rotate_deg": 10.0, "scale": [0.95, 1.05],
           "translate_vox": 1.5, "gain": [0.9, 1.1], "bias": [-0.1, 0.1], "padding": "border"}


def test_paired_modalities_move_together():
    torch.manual_seed(22)
    batch = {"mri": volume((2, 9, 11, 13), 16).cuda(), "pet1451": volume((2, 9, 11, 13), 17).cuda(),
             "label": torch.tensor([0, 1], device="cuda")}
    aug = augment.VolumeAugmenter(**AUG_CFG)
    out = aug(batch)
    assert out["label"] is batch["label"] and set(out) == set(batch)
    theta, intensity = aug.theta.cpu(), aug.intensity.cpu()
    assert not torch.equal(intensity[:, 0], intensity[:, 1])
    for m, k in enumerate(("mri", "pet1451")):
        assert out[k].data_ptr() != batch[k].data_ptr()
        assert_close(out[k], oracle(batch[k].cpu(), theta, "border", intensity[:, m]), k)


# ---------------------------------------------------------------------------- 6. graph replay
def test_graph_replay_draws_fresh_transforms():
    torch.manual_seed(23)
    batch = {"mri": volume((2, 9, 11, 13), 18).cuda(), "label": torch.tensor([0, 1], device="cuda")}
    aug = augment.VolumeAugmenter(**AUG_CFG)
    aug(batch)                                               # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(batch)
    thetas = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        thetas.append(aug.theta.clone())
        again = augment.resample(batch["mri"], aug.theta, "border", aug.intensity[:, 0])
        assert torch.equal(out["mri"], again)
    assert not torch.equal(thetas[0], thetas[1]) and not torch.equal(thetas[1], thetas[2])


# ---------------------------------------------------------------------------- 7. model wiring
def _models():
    torch.manual_seed(24)
    plain = M.Anat_CNN(G.anat_hparams(10, precision="32")).cuda()
    with_key = M.Anat_CNN(G.anat_hparams(10, precision="32", augment=AUG_CFG)).cuda()
    with_key.load_state_dict(plain.state_dict())
    batch = {"mri": volume((2, 32, 32, 32), 19).cuda(), "label": torch.tensor([1, 0], device="cuda")}
    return plain, with_key, batch


def test_general_step_augments_in_train_mode_only():
    plain, with_key, batch = _models()
    with torch.no_grad():
        ref = plain.general_step(batch, 0, "val")
        got = with_key.general_step(batch, 0, "val")
        assert with_key.augmenter.theta is None              # nothing was drawn
        assert torch.equal(got["outputs"], ref["outputs"]) and torch.equal(got["loss"], ref["loss"])
        got = with_key.general_step(batch, 0, "train")
        aug = with_key.augmenter
        x = augment.resample(batch["mri"], aug.theta, "border", aug.intensity[:, 0])
        assert not torch.equal(x, batch["mri"])
        ref = plain.general_step({"mri": x, "label": batch["label"]}, 0, "train")
        assert torch.equal(got["outputs"], ref["outputs"]) and torch.equal(got["loss"], ref["loss"])


def test_graphed_train_step_with_augmentation():
    _, m, batch = _models()
    gs = GraphedTrainStep(m, m.configure_optimizers(), batch, warmup=1)
    thetas = []
    for _ in range(2):
        out = gs()
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        thetas.append(m.augmenter.theta.clone())
    assert not torch.equal(thetas[0], thetas[1])
