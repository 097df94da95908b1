"""Attribution maps: which voxels drove a prediction.

    saliency(model, batch, target=None, method="gradient", steps=8, baseline=None)
    grad_cam(model, batch, target=None, upsample=True)

``model`` is any of the drop-in LightningModule classes (classifiers.py), ``batch`` the dict
its ``general_step`` takes (a missing ``"label"`` is filled with zeros: the loss is computed
but never differentiated).  No reference counterpart: the reference has no attribution code;
the maps are autograd's gradients of the reference's own forward (anat_cnn.py:99-104), so a
plain-torch restatement of a model gives the same maps through ``torch.autograd.grad``.

Both functions

* run the model in ``eval()`` mode (running BN statistics, dropout off: samples are
  independent) and under ``torch.enable_grad()``, also when called inside ``no_grad``;
* switch every parameter's ``requires_grad`` off for the call, so no weight gradient is
  launched, and use ``torch.autograd.grad`` only: no parameter ends up with a ``.grad``;
* call ``model.general_step(batch, 0, "pred")``, so each class's own input plumbing is
  reused, with every volume entry (``"mri"``, ``"pet1451"``) replaced by a detached clone that
  requires grad (a batch carrying a device-normalisation spec is normalised first: the maps
  are w.r.t. the volumes the network sees);
* restore the training flags and ``requires_grad`` flags afterwards, also on an exception.

The score that is differentiated is the model's own output logit of class ``target`` (``None``:
the per-sample argmax of the eval logits; an int; or a (B,) tensor), summed over the batch.
``Anat_CNN`` and the models built on it end in a ReLU: a logit the ReLU has zeroed has a zero
gradient everywhere, so its map is all zeros.  That is faithful, not a failure -- the returned
``"score"`` (the logits that were differentiated) shows it.

The input gradient of the first conv is the ``stem_dgrad`` kernel (MedicalNet stem, bf16) or
the generic Ci-padded route (volume_ops.raw_input_grad).  Channel-stacked early-fusion inputs
(``PET_MRI_EF``) are not covered yet: their first conv raises ``MMADError``.
"""
import torch
import torch.nn.functional as F

from . import medicalnet

VOLUME_KEYS = ("mri", "pet1451")
METHODS = ("gradient", "grad_x_input", "integrated")


class _Frozen:
    """eval mode + every parameter's requires_grad off, restored on exit"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.modes = [(m, m.training) for m in self.model.modules()]
        self.flags = [(p, p.requires_grad) for p in self.model.parameters()]
        self.model.eval()
        for p, _ in self.flags:
            p.requires_grad_(False)
        return self

    def __exit__(self, *exc):
        for p, f in self.flags:
            p.requires_grad_(f)
        for m, t in self.modes:
            m.training = t
        return False


def _prepared(model, batch):
    """(batch as general_step will see it, its volume keys)"""
    batch = dict(model.prepare_batch(dict(batch)))
    keys = [k for k in VOLUME_KEYS if isinstance(batch.get(k), torch.Tensor)]
    if not keys:
        raise ValueError(f"the batch has no volume entry (one of {VOLUME_KEYS})")
    if "label" not in batch:
        v = batch[keys[0]]
        batch["label"] = torch.zeros(v.shape[0], dtype=torch.int64, device=v.device)
    return batch, keys


def _leaves(vols, requires_grad=True):
    return {k: v.detach().clone().requires_grad_(requires_grad) for k, v in vols.items()}


def _logits(model, batch, vols):
    b = dict(batch)
    b.update(vols)
    return model.general_step(b, 0, "pred")["outputs"]


def _target(logits, target):
    n = logits.shape[0]
    if target is None:
        return logits.detach().argmax(dim=1)
    if isinstance(target, int):
        return torch.full((n,), target, dtype=torch.int64, device=logits.device)
    t = torch.as_tensor(target, device=logits.device).to(torch.int64).reshape(-1)
    if t.numel() != n:
        raise ValueError(f"target has {t.numel()} entries for a batch of {n}")
    return t


def _score(logits, tgt):
    return logits.gather(1, tgt[:, None]).squeeze(1)


def _input_grads(score, leaves):
    """d sum(score) / d leaf per volume key (zeros where the score does not depend on it)"""
    keys = list(leaves)
    if not score.requires_grad:
        return {k: torch.zeros_like(leaves[k]) for k in keys}
    grads = torch.autograd.grad(score.sum(), [leaves[k] for k in keys], allow_unused=True)
    return {k: torch.zeros_like(leaves[k]) if g is None else g for k, g in zip(keys, grads)}


def _baselines(baseline, vols):
    out = {}
    for k, v in vols.items():
        b = baseline.get(k) if isinstance(baseline, dict) else baseline
        if b is None:
            out[k] = torch.zeros_like(v)
        else:
            out[k] = torch.as_tensor(b, dtype=v.dtype, device=v.device).expand_as(v).contiguous()
    return out


def saliency(model, batch, target=None, method="gradient", steps=8, baseline=None):
    """Voxel-level attribution of the logit of class ``target`` (module docstring).

    method  "gradient"      d score / d x
            "grad_x_input"  x * d score / d x
            "integrated"    (x - x0) * mean_{k=1..steps} grad(x0 + (k - 1/2) / steps * (x - x0)):
                            integrated gradients by the midpoint rule, one forward / backward
                            per step; x0 = ``baseline`` (a tensor or number broadcast to each
                            volume, or a dict per volume key; None: zeros)

    Returns ``{"maps": {key: (B, D, H, W) float32}, "target": (B,) int64,
    "score": (B,) float64}``: one map per volume entry of the batch, the differentiated class
    and its logit at x."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    if method == "integrated" and steps < 1:
        raise ValueError("integrated gradients need steps >= 1")
    with _Frozen(model), torch.enable_grad():
        batch, keys = _prepared(model, batch)
        vols = {k: batch[k] for k in keys}
        if method == "integrated":
            logits = _logits(model, batch, _leaves(vols, False)).detach()
            tgt = _target(logits, target)
            x0 = _baselines(baseline, vols)
            total = {k: torch.zeros_like(v) for k, v in vols.items()}
            for i in range(steps):
                a = (i + 0.5) / steps
                leaves = _leaves({k: x0[k] + a * (vols[k] - x0[k]) for k in keys})
                g = _input_grads(_score(_logits(model, batch, leaves), tgt), leaves)
                for k in keys:
                    total[k] += g[k]
            maps = {k: (vols[k] - x0[k]) * total[k] / steps for k in keys}
        else:
            leaves = _leaves(vols)
            logits = _logits(model, batch, leaves)
            tgt = _target(logits, target)
            g = _input_grads(_score(logits, tgt), leaves)
            maps = {k: g[k] * vols[k] if method == "grad_x_input" else g[k] for k in keys}
        score = _score(logits.detach(), tgt).to(torch.float64)
    return {"maps": {k: m.detach().to(torch.float32) for k, m in maps.items()},
            "target": tgt, "score": score}


def grad_cam(model, batch, target=None, upsample=True):
    """Grad-CAM at ``layer4`` of every ``medicalnet.ResNet`` under ``model``: channel weights =
    the spatial mean of d score / d A, map = relu(sum_c w_c A_c), trilinearly upsampled to the
    backbone's input grid when ``upsample`` (else the raw layer4-grid map).

    Returns ``{"maps": {module name: (B, D, H, W) float32}, "target": (B,) int64,
    "score": (B,) float64}``.  A model without a ResNet backbone raises NotImplementedError."""
    nets = [(name, m) for name, m in model.named_modules() if isinstance(m, medicalnet.ResNet)]
    if not nets:
        raise NotImplementedError(
            f"grad_cam needs a MedicalNet ResNet backbone; {type(model).__name__} has none")
    acts, sizes, hooks = {}, {}, []
    for name, net in nets:
        hooks.append(net.layer4.register_forward_hook(
            lambda _m, _i, out, name=name: acts.__setitem__(name, out)))
        hooks.append(net.register_forward_pre_hook(
            lambda _m, args, name=name: sizes.__setitem__(name, tuple(args[0].shape[2:]))))
    try:
        with _Frozen(model), torch.enable_grad():
            batch, keys = _prepared(model, batch)
            logits = _logits(model, batch, _leaves({k: batch[k] for k in keys}))
            tgt = _target(logits, target)
            score = _score(logits, tgt)
            names = [n for n, _ in nets if n in acts and acts[n].requires_grad]
            grads = {}
            if score.requires_grad and names:
                gs = torch.autograd.grad(score.sum(), [acts[n] for n in names], allow_unused=True)
                grads = {n: g for n, g in zip(names, gs) if g is not None}
            maps = {}
            for name in acts:
                a = acts[name].detach().to(torch.float32)
                g = grads.get(name)
                g = torch.zeros_like(a) if g is None else g.detach().to(torch.float32)
                w = g.mean(dim=(2, 3, 4), keepdim=True)
                cam = torch.relu((w * a).sum(dim=1))
                if upsample:
                    cam = F.interpolate(cam[:, None], size=sizes[name], mode="trilinear",
                                        align_corners=False)[:, 0]
                maps[name] = cam.contiguous()
            score = score.detach().to(torch.float64)
    finally:
        for h in hooks:
            h.remove()
    return {"maps": maps, "target": tgt, "score": score}
