"""Elastic deformation of the device augmentation (multimodal_alzheimer_amd.augment) against
torch on the CPU in float64.  The oracle interpolates the control lattice with
``F.grid_sample(align_corners=True, padding_mode='border')`` over the identity grid, adds
``2 u / size`` to ``F.affine_grid``'s grid and samples the volume with ``F.grid_sample``; the
drawn lattices are checked for what they must be, the fold guard is checked on the map that was
actually drawn, and the augmenter is followed through a captured graph and a model's
``general_step``.

Bar of every comparison with the oracle: max|got - ref| <= 1e-12 * max|ref| (the project's
bar for float64 kernels whose operation order differs from torch's)."""
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
CASES = [((2, 9, 11, 13), (3, 4, 5)), ((1, 5, 7, 67), (2, 2, 7)), ((2, 16, 16, 16), (7, 7, 7)),
         ((1, 12, 10, 14), (12, 2, 3))]
BOUNDS = (1.5, 0.8, 2.0)                                     # voxels, components (x, y, z)


def oracle(x, theta, lattice, padding, gain_bias=None):
    """x (B, D, H, W), theta (B, 3, 4), lattice (B, 3, Gd, Gh, Gw), gain_bias (B, 2): CPU
    float64 tensors."""
    grid = oracle_grid(x.shape, theta, lattice)
    y = F.grid_sample(x[:, None], grid, mode="bilinear", padding_mode=padding,
                      align_corners=False)[:, 0]
    if gain_bias is not None:
        y = gain_bias[:, 0, None, None, None] * y + gain_bias[:, 1, None, None, None]
    return y


def oracle_grid(shape, theta, lattice):
    b, d, h, w = shape
    size = (b, 1, d, h, w)
    eye = torch.eye(3, 4, dtype=torch.float64).expand(b, 3, 4).contiguous()
    base = F.affine_grid(eye, size, align_corners=False)
    disp = F.grid_sample(lattice, base, mode="bilinear", padding_mode="border",
                         align_corners=True)
    ext = torch.tensor([w, h, d], dtype=torch.float64)
    return F.affine_grid(theta, size, align_corners=False) + 2.0 * disp.permute(0, 2, 3, 4, 1) / ext


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
    """the two fixed transforms of tests/test_augment_gpu.py"""
    a = torch.cat([0.9 * rotation(0.1, 0.2, 0.3),
                   torch.tensor([[0.2], [-0.1], [0.15]], dtype=torch.float64)], 1)
    lin = 1.07 * rotation(0.3, 0.1, 0.2)
    lin[:, 0] = -lin[:, 0]                                   # x flip
    b = torch.cat([lin, torch.tensor([[-0.05], [0.2], [0.1]], dtype=torch.float64)], 1)
    return a, b


def batch_theta(b, first):
    thetas = fixed_thetas()
    return torch.stack([thetas[(n + first) % 2] for n in range(b)])


def volume(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def random_lattice(b, grid, seed):
    u = torch.rand((b, 3) + tuple(grid), dtype=torch.float64,
                   generator=torch.Generator().manual_seed(seed))
    return (2.0 * u - 1.0) * torch.tensor(BOUNDS, dtype=torch.float64)[None, :, None, None, None]


def strided_gain_bias(b):
    """a (B, 2, 2) tensor whose [:, 1] is the (gain, bias) view, row stride 4"""
    both = torch.tensor([[[9.0, 9.0], [1.3, -0.2]], [[9.0, 9.0], [0.7, 0.45]]],
                        dtype=torch.float64)[:b].contiguous()
    return both


# --------------------------------------------------------------------- 1. resample vs oracle
@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("with_gb", [False, True])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("shape, grid", CASES)
def test_deform_matches_oracle(shape, grid, first, with_gb, padding):
    x, theta = volume(shape, 31), batch_theta(shape[0], first)
    lattice = random_lattice(shape[0], grid, 32)
    both = strided_gain_bias(shape[0]) if with_gb else None
    gb_dev = both.cuda()[:, 1] if with_gb else None
    assert gb_dev is None or gb_dev.stride(0) == 4
    got = augment.resample(x.cuda(), theta.cuda(), padding, gb_dev, lattice=lattice.cuda())
    ref = oracle(x, theta, lattice, padding, both[:, 1] if with_gb else None)
    assert_close(got, ref, f"{shape} {grid} theta{first} gb={with_gb} {padding}")


@pytest.mark.parametrize("padding", ["zeros", "border"])
def test_deform_partly_outside_the_volume(padding):
    shape, grid = CASES[0]
    x, theta = volume(shape, 33), batch_theta(2, 0)
    theta[0, :, 3] += torch.tensor([0.9, 0.0, -0.6])         # almost half a volume along x
    theta[1, :, 3] += torch.tensor([0.0, -1.1, 0.7])
    lattice = random_lattice(2, grid, 34)
    ref = oracle(x, theta, lattice, padding)
    if padding == "zeros":                                   # part of it does sample outside
        assert 0.1 < (ref == 0.0).double().mean().item() < 0.9
    got = augment.resample(x.cuda(), theta.cuda(), padding, lattice=lattice.cuda())
    assert_close(got, ref, f"translated out, {padding}")


# ------------------------------------------------------------------------- 2. zero lattice
@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("first", [0, 1])
def test_zero_lattice_is_the_affine_resample_bit_for_bit(first, padding):
    x, theta = volume((2, 9, 11, 13), 35).cuda(), batch_theta(2, first).cuda()
    gb = strided_gain_bias(2).cuda()[:, 1]
    zero = torch.zeros((2, 3, 3, 4, 5), dtype=torch.float64, device="cuda")
    assert torch.equal(augment.resample(x, theta, padding, gb, lattice=zero),
                       augment.resample(x, theta, padding, gb))
    assert torch.equal(augment.resample(x, theta, padding, lattice=zero),
                       augment.resample(x, theta, padding))


# ---------------------------------------------------------------------------------- 3. draw
EXTENT = (24, 20, 28)
A, B_, C_ = 1.5, 0.75, 2.25


@pytest.mark.parametrize("grid", [7, (2, 5, 12)])
@pytest.mark.parametrize("vox", [(A, 0, 0), (0, B_, 0), (0, 0, C_), (A, B_, C_)])
def test_drawn_lattice(vox, grid):
    cfg = {"elastic_vox": vox, "elastic_grid": grid, "rotate_deg": 10.0, "gain": [0.9, 1.1]}
    torch.manual_seed(41)
    theta, intensity, lattice = augment.draw(cfg, 4, EXTENT, "cuda", nmod=2, return_lattice=True)
    grid3 = (grid,) * 3 if isinstance(grid, int) else grid
    assert lattice.shape == (4, 3) + grid3 and lattice.dtype == torch.float64
    assert lattice.is_contiguous()
    lat = lattice.cpu()
    n = 4 * grid3[0] * grid3[1] * grid3[2]
    for axis, m in enumerate(vox):                           # axis d, h, w <-> component 2, 1, 0
        comp = lat[:, 2 - axis]
        if m == 0:
            assert torch.count_nonzero(comp).item() == 0
            continue
        assert comp.abs().max().item() <= m
        assert abs(comp.mean().item()) <= 5 * m / math.sqrt(3 * n)
        assert comp.max().item() > 0.9 * m and comp.min().item() < -0.9 * m
    assert not torch.equal(lat[0], lat[1]) and not torch.equal(lat[1], lat[2])
    # the same seed, the same lattice; sample 0 does not depend on the batch size
    torch.manual_seed(41)
    _, _, again = augment.draw(cfg, 4, EXTENT, "cuda", nmod=2, return_lattice=True)
    assert torch.equal(again, lattice)
    torch.manual_seed(41)
    _, _, two = augment.draw(cfg, 2, EXTENT, "cuda", nmod=2, return_lattice=True)
    assert torch.equal(two, lattice[:2])
    fresh = augment.draw(cfg, 4, EXTENT, "cuda", nmod=2, return_lattice=True)[2]
    assert not torch.equal(fresh, lattice)
    # theta and intensity are what they are without elastic, under one seed
    off = {k: v for k, v in cfg.items() if not k.startswith("elastic")}
    torch.manual_seed(41)
    theta0, intensity0 = augment.draw(off, 4, EXTENT, "cuda", nmod=2)
    assert torch.equal(theta0, theta) and torch.equal(intensity0, intensity)
    torch.manual_seed(41)
    theta1, intensity1, none = augment.draw(off, 4, EXTENT, "cuda", nmod=2, return_lattice=True)
    assert none is None and torch.equal(theta1, theta) and torch.equal(intensity1, intensity)
    torch.manual_seed(41)
    assert len(augment.draw(cfg, 4, EXTENT, "cuda", nmod=2)) == 2     # the default stays a pair


# ------------------------------------------------------------------------------ 4. fold guard
FOLD_CFG = {"flip_p": 0.5, "rotate_deg": 10.0, "scale": [0.8, 1.1], "elastic_grid": [4, 3, 5]}


def test_fold_free_at_the_cap():
    shape = (2, 24, 20, 28)
    cap = augment.AugmentConfig(**FOLD_CFG).elastic_cap(shape[1:])
    aug = augment.VolumeAugmenter(elastic_vox=0.99 * cap, **FOLD_CFG)
    ext = torch.tensor([28.0, 20.0, 24.0], dtype=torch.float64)            # (W, H, D)
    for seed in range(4):
        torch.manual_seed(50 + seed)
        aug({"mri": volume(shape, 36).cuda()})
        theta, lattice = aug.theta.cpu(), aug.lattice.cpu()
        assert lattice.abs().max().item() > 0.9 * 0.99 * cap
        pos = ((oracle_grid(shape, theta, lattice) + 1.0) * ext - 1.0) / 2  # voxels, (x, y, z)
        core = pos[:, :-1, :-1, :-1]
        jac = torch.stack([pos[:, :-1, :-1, 1:] - core,                     # d pos / d x_out
                           pos[:, :-1, 1:, :-1] - core,                     # d pos / d y_out
                           pos[:, 1:, :-1, :-1] - core], -1)                # d pos / d z_out
        det = torch.linalg.det(jac)
        sign = torch.linalg.det(theta[:, :, :3]).sign()
        assert sign.abs().min().item() == 1.0
        signed = det * sign[:, None, None, None]
        print(f"seed {seed}: smallest signed determinant {signed.min().item():.3f}")
        assert signed.min().item() > 0.0


def test_setting_over_the_cap_raises_before_any_launch():
    shape = (2, 24, 20, 28)
    cap = augment.AugmentConfig(**FOLD_CFG).elastic_cap(shape[1:])
    aug = augment.VolumeAugmenter(elastic_vox=1.001 * cap, **FOLD_CFG)
    state = torch.cuda.get_rng_state()
    with pytest.raises(ValueError, match="fold"):
        aug({"mri": volume(shape, 36).cuda()})
    assert aug.theta is None and aug.lattice is None
    assert torch.equal(torch.cuda.get_rng_state(), state)    # not even the seed was drawn


# ---------------------------------------------------------------------- 5. paired modalities
AUG_CFG = {"flip_p": [0.5, 0.5, 0.5], "rotate_deg": 10.0, "scale": [0.95, 1.05],
           "translate_vox": 1.5, "gain": [0.9, 1.1], "bias": [-0.1, 0.1], "padding": "border",
           "elastic_vox": [0.3, 0.2, 0.25], "elastic_grid": [3, 4, 5]}


def test_paired_modalities_share_theta_and_lattice():
    torch.manual_seed(42)
    batch = {"mri": volume((2, 9, 11, 13), 37).cuda(), "pet1451": volume((2, 9, 11, 13), 38).cuda(),
             "label": torch.tensor([0, 1], device="cuda")}
    aug = augment.VolumeAugmenter(**AUG_CFG)
    out = aug(batch)
    assert out["label"] is batch["label"] and set(out) == set(batch)
    assert aug.lattice.shape == (2, 3, 3, 4, 5)
    theta, intensity, lattice = aug.theta.cpu(), aug.intensity.cpu(), aug.lattice.cpu()
    assert lattice.abs().max().item() > 0.0
    assert not torch.equal(intensity[:, 0], intensity[:, 1])
    for m, k in enumerate(("mri", "pet1451")):
        assert_close(out[k], oracle(batch[k].cpu(), theta, lattice, "border", intensity[:, m]), k)
    # elastic off: no lattice, the affine entry
    plain = augment.VolumeAugmenter(**{k: v for k, v in AUG_CFG.items()
                                       if not k.startswith("elastic")})
    plain(batch)
    assert plain.lattice is None and plain.theta is not None


# ---------------------------------------------------------------------------- 6. graph replay
def test_graph_replay_draws_fresh_lattices():
    torch.manual_seed(43)
    batch = {"mri": volume((2, 9, 11, 13), 39).cuda(), "label": torch.tensor([0, 1], device="cuda")}
    aug = augment.VolumeAugmenter(**AUG_CFG)
    aug(batch)                                               # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = aug(batch)
    lattices = []
    for r in range(2):
        g.replay()
        torch.cuda.synchronize()
        lattices.append(aug.lattice.clone())
        ref = oracle(batch["mri"].cpu(), aug.theta.cpu(), aug.lattice.cpu(), "border",
                     aug.intensity[:, 0].cpu())
        assert_close(out["mri"], ref, f"replay {r}")
    assert not torch.equal(lattices[0], lattices[1])


# ---------------------------------------------------------------------------- 7. model wiring
MODEL_CFG = dict(AUG_CFG, elastic_vox=0.6, elastic_grid=7)


def _models():
    torch.manual_seed(44)
    plain = M.Anat_CNN(G.anat_hparams(10, precision="32")).cuda()
    with_key = M.Anat_CNN(G.anat_hparams(10, precision="32", augment=MODEL_CFG)).cuda()
    with_key.load_state_dict(plain.state_dict())
    batch = {"mri": volume((2, 32, 32, 32), 40).cuda(), "label": torch.tensor([1, 0], device="cuda")}
    return plain, with_key, batch


def test_general_step_deforms_in_train_mode_only():
    plain, with_key, batch = _models()
    with torch.no_grad():
        ref = plain.general_step(batch, 0, "val")
        got = with_key.general_step(batch, 0, "val")
        assert with_key.augmenter.lattice is None            # nothing was drawn
        assert torch.equal(got["outputs"], ref["outputs"]) and torch.equal(got["loss"], ref["loss"])
        got = with_key.general_step(batch, 0, "train")
        aug = with_key.augmenter
        assert aug.lattice.shape == (2, 3, 7, 7, 7) and aug.lattice.abs().max().item() > 0.0
        x = augment.resample(batch["mri"], aug.theta, "border", aug.intensity[:, 0], aug.lattice)
        affine_only = augment.resample(batch["mri"], aug.theta, "border", aug.intensity[:, 0])
        assert not torch.equal(x, affine_only)
        ref = plain.general_step({"mri": x, "label": batch["label"]}, 0, "train")
        assert torch.equal(got["outputs"], ref["outputs"]) and torch.equal(got["loss"], ref["loss"])


def test_graphed_train_step_with_elastic():
    _, m, batch = _models()
    gs = GraphedTrainStep(m, m.configure_optimizers(), batch, warmup=1)
    lattices = []
    for _ in range(2):
        out = gs()
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss"]).all()
        lattices.append(m.augmenter.lattice.clone())
    assert lattices[0].abs().max().item() > 0.0
    assert not torch.equal(lattices[0], lattices[1])


# ---------------------------------------------------------------------------------- 8. errors
def test_bad_lattices_raise():
    x = torch.zeros((2, 4, 5, 6), dtype=torch.float64, device="cuda")
    theta = torch.eye(3, 4, dtype=torch.float64, device="cuda").expand(2, 3, 4).contiguous()
    good = torch.zeros((2, 3, 3, 4, 5), dtype=torch.float64, device="cuda")
    augment.resample(x, theta, lattice=good)
    bad = [
        torch.zeros((1, 3, 3, 4, 5), dtype=torch.float64, device="cuda"),       # batch
        torch.zeros((2, 2, 3, 4, 5), dtype=torch.float64, device="cuda"),       # components
        torch.zeros((2, 3, 4, 5), dtype=torch.float64, device="cuda"),          # rank
        torch.zeros((2, 3, 1, 4, 5), dtype=torch.float64, device="cuda"),       # extent < 2
        torch.zeros((2, 3, 3, 13, 5), dtype=torch.float64, device="cuda"),      # extent > 12
        torch.zeros((2, 3, 3, 4, 5), dtype=torch.float32, device="cuda"),       # dtype
        torch.zeros((2, 3, 3, 4, 5), dtype=torch.float64),                      # device
        torch.zeros((2, 3, 3, 5, 4), dtype=torch.float64, device="cuda").transpose(3, 4),
        torch.zeros((2, 3, 3, 4, 10), dtype=torch.float64, device="cuda")[..., ::2],
    ]
    for lattice in bad:
        with pytest.raises(_lib.MMADError):
            augment.resample(x, theta, lattice=lattice)
    with pytest.raises(_lib.MMADError, match="backward"):
        augment.resample(x, theta, lattice=good.clone().requires_grad_())
