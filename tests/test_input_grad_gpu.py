"""Autograd wiring of the raw-input gradient (volume_ops._Conv3dFn with a (B,1,D,H,W) input
that requires grad) and what explain.saliency leaves behind: nothing."""
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import explain
from multimodal_alzheimer_amd import volume_ops as V
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("cdtype", [torch.bfloat16, torch.float32])
def test_conv3d_raw_input_gets_a_gradient_and_nothing_else_moves(cdtype):
    gen = torch.Generator(device=DEV).manual_seed(11)
    x0 = torch.rand((2, 1, 16, 16, 16), generator=gen, device=DEV, dtype=torch.float64)
    w0 = torch.randn((64, 1, 7, 7, 7), generator=gen, device=DEV) * 0.05
    res = []
    for need in (True, False):
        x = x0.clone().requires_grad_(need)
        w = w0.clone().requires_grad_(True)
        y = V.conv3d(x, w, None, (2, 2, 2), (3, 3, 3), (1, 1, 1), cdtype)
        gy = torch.ones_like(y) * 0.5
        y.backward(gy)
        torch.cuda.synchronize()
        res.append((x, w, y.detach()))
    x, w, y = res[0]
    assert x.grad is not None, "the raw input got no gradient"
    assert x.grad.dtype == torch.float64 and x.grad.shape == x.shape
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    assert res[1][0].grad is None
    assert torch.equal(y, res[1][2])                 # no existing path moved
    assert torch.equal(w.grad, res[1][1].grad)
    # the value: d/dx of sum(0.5 * conv(x, w)) in float64 on the operands the kernels saw
    wr = w0.to(cdtype).double().cpu()
    ref = torch.nn.grad.conv3d_input(x.shape, wr, torch.full(y.shape, 0.5, dtype=torch.float64),
                                     stride=2, padding=3)
    mag = torch.nn.grad.conv3d_input(x.shape, wr.abs(),
                                     torch.full(y.shape, 0.5, dtype=torch.float64), stride=2,
                                     padding=3)
    err = (x.grad.cpu() - ref).abs()
    if cdtype == torch.bfloat16:        # the dedicated kernel: fp32 accumulation, f64 store
        assert L.load().mmad_stem_dgrad_ok(V.conv_desc(x.shape, w.shape, (2,) * 3, (3,) * 3,
                                                       (1,) * 3), L.BF16, L.F64) == 1
    assert (err <= 1e-3 * ref.abs() + 1e-4 * mag).all(), err.max().item()


def test_f32_raw_input_gets_an_f32_gradient():
    gen = torch.Generator(device=DEV).manual_seed(12)
    x = torch.rand((1, 1, 12, 12, 12), generator=gen, device=DEV).requires_grad_(True)
    w = (torch.randn((8, 1, 5, 5, 5), generator=gen, device=DEV) * 0.1).requires_grad_(True)
    b = torch.zeros(8, device=DEV, requires_grad=True)
    y = V.conv3d(x, w, b, (1, 1, 1), (2, 2, 2), (1, 1, 1), torch.float32)
    y.sum().backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    ref = torch.nn.grad.conv3d_input(x.shape, w.detach().double().cpu(),
                                     torch.ones(y.shape, dtype=torch.float64), padding=2)
    assert (x.grad.double().cpu() - ref).abs().max() <= 1e-4 * ref.abs().max()


def _train_step(m, batch):
    for p in m.parameters():
        p.grad = None
    m.train()
    o = m.general_step(batch, 0, "train")
    o["loss"].backward()
    torch.cuda.synchronize()
    return o["loss"].detach().clone(), m.model.conv1.weight.grad.detach().clone()


def test_saliency_leaves_the_model_and_the_training_step_untouched():
    torch.manual_seed(3)
    m = M.Anat_CNN(G.anat_hparams(10, precision="bf16")).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    batch = {"mri": torch.rand((2, 64, 64, 64), generator=gen, device=DEV, dtype=torch.float64),
             "label": torch.tensor([0, 1], device=DEV)}
    # the BN running statistics move with every training step: same state before both steps
    state = {k: v.clone() for k, v in m.state_dict().items()}
    loss0, dw0 = _train_step(m, batch)
    m.load_state_dict(state)
    for p in m.parameters():
        p.grad = None
    frozen = next(iter(m.model.conv_seg.parameters()))
    frozen.requires_grad_(False)                           # a flag saliency must put back
    flags = [p.requires_grad for p in m.parameters()]
    m.train()
    with torch.no_grad():                                  # saliency enables grad itself
        out = explain.saliency(m, batch)
    assert m.training and all(mod.training for mod in m.modules())
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())
    assert out["maps"]["mri"].shape == (2, 64, 64, 64)
    assert out["maps"]["mri"].dtype == torch.float32
    assert out["target"].dtype == torch.int64 and out["score"].dtype == torch.float64
    assert torch.isfinite(out["maps"]["mri"]).all()
    assert not batch["mri"].requires_grad
    frozen.requires_grad_(True)
    m.load_state_dict(state)                               # eval mode moved no buffer anyway
    loss1, dw1 = _train_step(m, batch)
    assert torch.equal(loss0, loss1)
    assert torch.equal(dw0, dw1)


def test_eval_mode_moves_no_running_statistic():
    torch.manual_seed(4)
    m = M.Anat_CNN(G.anat_hparams(10)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(6)
    batch = {"mri": torch.rand((2, 32, 32, 32), generator=gen, device=DEV, dtype=torch.float64),
             "label": torch.tensor([0, 1], device=DEV)}
    state = {k: v.clone() for k, v in m.state_dict().items()}
    explain.saliency(m, batch, method="integrated", steps=2)
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k


def test_channel_stacked_sources_still_raise():
    gen = torch.Generator(device=DEV).manual_seed(7)
    pet = torch.rand((1, 8, 8, 8), generator=gen, device=DEV, dtype=torch.float64,
                     requires_grad=True)
    mri = torch.rand((1, 8, 8, 8), generator=gen, device=DEV, dtype=torch.float64)
    w = torch.randn((8, 2, 3, 3, 3), generator=gen, device=DEV)
    with pytest.raises(L.MMADError, match="channel-stacked"):
        V.conv3d(V.StackedVolumes([pet, mri]), w, None, (1, 1, 1), (1, 1, 1), (1, 1, 1))
    x = torch.stack((pet.detach(), mri), dim=1).requires_grad_(True)
    with pytest.raises(L.MMADError, match="channel-stacked"):
        V.conv3d(x, w, None, (1, 1, 1), (1, 1, 1), (1, 1, 1))
