"""explain.saliency / explain.grad_cam at model level against the CPU oracle run live.

The oracle (oracle/models_ref.py) is plain torch, so torch.autograd.grad w.r.t. its input is
the reference map.  Both sides run in eval mode on the fixture's weights and batch, with the
target class taken as the argmax of the fixture's ``eval_logits``.

Bars
  * fp32 mode: the project's float64 bar (_assert_f64_bar of test_model_parity_gpu.py):
    max|ours - exact| <= max(4 x the oracle's own fp32 error, 1e-2 max|exact|), exact = the
    oracle in float64.
  * bf16 mode: the project's bf16 yardstick (test_fullsize_oracle_gpu.py): the normwise error
    of our map against float64 is at most 2 x the normwise error of the oracle under
    torch.autocast("cpu", dtype=torch.bfloat16), + 0.02.  The yardstick is computed live.
  * Grad-CAM (fp32): the raw layer4-grid map within 1e-2 max|ref| of the same formula on the
    oracle."""
import numpy as np
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import explain
from multimodal_alzheimer_amd import volume_ops as V
from tests import _golden as G
from tests.test_model_parity_gpu import _assert_f64_bar, build_product

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES32 = ["pet_resnet_r10", "small_pet", "anat_pet_fusion", "anat_r10_focal"]
_ORACLE = {}


def _case(name):
    g = G.load(name)
    return g, G.batch_of(name, g), torch.from_numpy(g["eval_logits"].argmax(1))


def _oracle_forward(ref, vols):
    if hasattr(ref, "batch_key"):
        return ref(vols[ref.batch_key].unsqueeze(1))
    return ref(vols["pet1451"].unsqueeze(1), vols["mri"].unsqueeze(1))


def _oracle_model(name, mode):
    g = G.load(name)
    ref = G.build_oracle(name)
    G.load_fixture_weights(ref, g)
    ref = ref.double() if mode == "f64" else ref.float()
    ref.eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


def _oracle_grad(ref, mode, vols, tgt):
    """(d sum_b logit[b, tgt_b] / d volume per used key, logits)"""
    dtype = torch.float64 if mode == "f64" else torch.float32
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in vols.items()}
    if mode == "bf16":
        with torch.autocast("cpu", dtype=torch.bfloat16):
            logits = _oracle_forward(ref, leaves)
    else:
        logits = _oracle_forward(ref, leaves)
    score = logits.double().gather(1, tgt[:, None]).sum()
    keys = list(leaves)
    if not score.requires_grad:
        return {k: np.zeros(tuple(vols[k].shape)) for k in keys}, logits.detach()
    gs = torch.autograd.grad(score, [leaves[k] for k in keys], allow_unused=True)
    return ({k: (np.zeros(tuple(vols[k].shape)) if gr is None else gr.double().numpy())
             for k, gr in zip(keys, gs)}, logits.detach())


def _oracle_maps(name, mode, method="gradient", steps=4):
    key = (name, mode, method)
    if key in _ORACLE:
        return _ORACLE[key]
    g, batch, tgt = _case(name)
    ref = _oracle_model(name, mode)
    vols = {k: batch[k] for k in G.CASES[name][3]}
    if method == "integrated":
        total = {k: 0.0 for k in vols}
        for i in range(steps):
            a = (i + 0.5) / steps
            gr, _ = _oracle_grad(ref, mode, {k: a * v for k, v in vols.items()}, tgt)
            total = {k: total[k] + gr[k] for k in vols}
        maps = {k: vols[k].double().numpy() * total[k] / steps for k in vols}
    else:
        gr, _ = _oracle_grad(ref, mode, vols, tgt)
        maps = {k: gr[k] * vols[k].double().numpy() if method == "grad_x_input" else gr[k]
                for k in vols}
    _ORACLE[key] = maps
    return maps


def _product(name, precision=None):
    g, batch, tgt = _case(name)
    m = build_product(name)
    G.load_fixture_weights(m, g)
    if precision is not None:
        M.layers.set_compute_dtype(m, precision)
    m = m.to(DEV)
    return m, {k: v.to(DEV) for k, v in batch.items()}, tgt.to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_fp32(name, method="gradient", **kw):
    m, batch, tgt = _product(name)
    out = explain.saliency(m, batch, target=tgt, method=method, **kw)
    exact = _oracle_maps(name, "f64", method)
    ref32 = _oracle_maps(name, "f32", method)
    assert sorted(out["maps"]) == sorted(exact)
    assert torch.equal(out["target"], tgt)
    for k in exact:
        ours = _np(out["maps"][k])
        assert ours.shape == exact[k].shape
        print(f"{name}/{k}/{method}: max|exact| {np.abs(exact[k]).max():.3e}, oracle fp32 err "
              f"{np.abs(ref32[k] - exact[k]).max():.3e}, ours {np.abs(ours - exact[k]).max():.3e}")
        assert np.abs(exact[k]).max() > 0
        _assert_f64_bar(f"{name}/{k}/{method}", ours.ravel(), ref32[k].ravel(),
                        exact[k].ravel(), np.abs(exact[k]).max())
    return out


@pytest.mark.parametrize("name", CASES32 + ["anat_r10_mni"])
def test_fp32_gradient_maps_match_the_float64_oracle(name):
    out = _check_fp32(name)
    g = G.load(name)
    sc = np.take_along_axis(g["eval_logits"], g["eval_logits"].argmax(1)[:, None], 1)[:, 0]
    assert np.abs(_np(out["score"]) - sc).max() <= 1e-4        # the north star's logit bar


@pytest.mark.parametrize("method", ["grad_x_input", "integrated"])
def test_fp32_other_methods(method):
    kw = {"steps": 4} if method == "integrated" else {}
    _check_fp32("pet_resnet_r10", method, **kw)


def test_default_target_is_the_eval_argmax():
    m, batch, tgt = _product("pet_resnet_r10")
    a = explain.saliency(m, batch)
    assert torch.equal(a["target"], tgt)
    b = explain.saliency(m, batch, target=int(tgt[0]))
    assert torch.equal(b["target"], torch.full_like(tgt, int(tgt[0])))


def test_relu_zeroed_logit_gives_a_zero_map():
    m, batch, _ = _product("anat_r10_32_live")
    out = explain.saliency(m, batch)
    assert (out["score"] == 0).all()
    assert (out["maps"]["mri"] == 0).all()


@pytest.mark.parametrize("name", CASES32)
def test_bf16_maps_within_the_reference_bf16_error(name):
    m, batch, tgt = _product(name, torch.bfloat16)
    lib = L.load()
    stems = [c for c in m.modules() if isinstance(c, M.layers.Conv3d) and c.in_channels == 1]
    assert stems
    for c in stems:          # the route the backward takes (volume_ops.raw_input_grad)
        shape = (batch["label"].shape[0], 1) + tuple(batch[G.CASES[name][3][0]].shape[1:])
        d = V.conv_desc(shape, tuple(c.weight.shape), c._stride3(), c._pads(), c._dilation3())
        is_stem = tuple(c.weight.shape) == (64, 1, 7, 7, 7)
        assert lib.mmad_stem_dgrad_ok(d, L.BF16, L.F64) == int(is_stem)
    assert V.STEM_DGRAD
    out = explain.saliency(m, batch, target=tgt)
    exact = _oracle_maps(name, "f64")
    ref16 = _oracle_maps(name, "bf16")
    for k in exact:
        ours = _np(out["maps"][k])
        nrm = np.linalg.norm(exact[k])
        e_ours = np.linalg.norm(ours - exact[k]) / nrm
        e_ref = np.linalg.norm(ref16[k] - exact[k]) / nrm
        print(f"{name}/{k}: normwise error ours {e_ours:.3e}, oracle bf16 autocast {e_ref:.3e}")
        assert np.isfinite(ours).all()
        assert e_ours <= 2 * e_ref + 0.02, (e_ours, e_ref)


def _oracle_cam(name, sub):
    g, batch, tgt = _case(name)
    ref = _oracle_model(name, "f64")
    net = ref
    for part in sub.split("."):
        net = getattr(net, part)
    acts = []
    h = net.layer4.register_forward_hook(lambda _m, _i, out: acts.append(out))
    leaves = {k: batch[k].double().clone().requires_grad_(True) for k in G.CASES[name][3]}
    logits = _oracle_forward(ref, leaves)
    h.remove()
    (gr,) = torch.autograd.grad(logits.gather(1, tgt[:, None]).sum(), acts)
    w = gr.mean(dim=(2, 3, 4), keepdim=True)
    return torch.relu((w * acts[0].detach()).sum(dim=1)).numpy()


@pytest.mark.parametrize("name,sub", [("pet_resnet_r10", "model"),
                                      ("anat_pet_fusion", "model_mri.model")])
def test_grad_cam_matches_the_oracle(name, sub):
    m, batch, tgt = _product(name)
    ref = _oracle_cam(name, sub)
    raw = explain.grad_cam(m, batch, target=tgt, upsample=False)
    assert list(raw["maps"]) == [sub]
    ours = _np(raw["maps"][sub])
    assert ours.shape == ref.shape
    print(f"{name}: max|cam| {np.abs(ref).max():.3e}, err {np.abs(ours - ref).max():.3e}")
    assert np.abs(ref).max() > 0
    assert np.abs(ours - ref).max() <= 1e-2 * np.abs(ref).max()
    up = explain.grad_cam(m, batch, target=tgt)
    key = "pet1451" if name == "pet_resnet_r10" else "mri"
    assert tuple(up["maps"][sub].shape) == tuple(batch[key].shape)
    assert (up["maps"][sub] >= 0).all()
    assert all(p.grad is None for p in m.parameters())


def test_grad_cam_needs_a_resnet():
    m, batch, _ = _product("small_pet")
    with pytest.raises(NotImplementedError):
        explain.grad_cam(m, batch)
