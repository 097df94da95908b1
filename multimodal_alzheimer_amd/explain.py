"""Attribution maps: which voxels drove a prediction.

    saliency(model, batch, target=None, method="gradient", steps=8, baseline=None)
    grad_cam(model, batch, target=None, upsample=True)
    occlusion(model, batch, target=None, patch=16, stride=None, fill=0.0, score="logit",
              keys=None, windows_per_replay=None, graph=None)

``model`` is any of the drop-in LightningModule classes (classifiers.py), ``batch`` the dict
its ``general_step`` takes (a missing ``"label"`` is filled with zeros: the loss is computed
but never differentiated).  No reference counterpart: the reference has no attribution code;
the maps are autograd's gradients of the reference's own forward (anat_cnn.py:99-104), so a
plain-torch restatement of a model gives the same maps through ``torch.autograd.grad``.

The two gradient-based functions

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
(``PET_MRI_EF``) are not covered by the gradient maps yet: their first conv raises
``MMADError``.

``occlusion`` needs forwards only (eval mode, ``no_grad``), so it has none of these holes: it
covers early fusion, its ``"prob"`` score still moves when the ReLU has clamped the logit, and
it occludes one modality at a time.  It is hundreds of eval forwards per batch, so it replays
one captured forward (``graph_step.GraphedEvalForward``) whose windows are moved and whose
scores are folded on the device (csrc/occlude.hip); see its docstring.
"""
import math

import torch
import torch.nn.functional as F

from . import _lib as L
from . import medicalnet

VOLUME_KEYS = ("mri", "pet1451")
METHODS = ("gradient", "grad_x_input", "integrated")
SCORES = ("logit", "prob")


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


# ------------------------------------------------------------------------------ occlusion
def _triple(name, v):
    """one int or three as an (d, h, w) tuple of ints"""
    if isinstance(v, int) and not isinstance(v, bool):
        return (v, v, v)
    try:
        t = tuple(v)
    except TypeError:
        raise ValueError(f"{name} must be one int or three (d, h, w), got {v!r}") from None
    if len(t) != 3 or any(isinstance(a, bool) or not hasattr(a, "__index__") for a in t):
        raise ValueError(f"{name} must be one int or three (d, h, w), got {v!r}")
    return tuple(a.__index__() for a in t)


def occlusion_windows(size, patch, stride=None):
    """The occluding windows of a volume of extent ``size`` (device-free; csrc/occlude.hip
    restates the rule).  Per axis, with ``1 <= stride <= patch <= size``,
    ``n = max(1, ceil((size - patch) / stride) + 1)`` windows start at
    ``min(i * stride, size - patch)``: every window is full size, the last one is shifted back
    rather than clipped, and every voxel is covered.  Window ``j = (iz * n_h + iy) * n_w + ix``.

    Returns ``{"patch": (3,), "stride": (3,), "starts": (list, list, list)}``."""
    size = _triple("size", size)
    patch = _triple("patch", patch)
    stride = patch if stride is None else _triple("stride", stride)
    starts = []
    for ax, s, p, t in zip("dhw", size, patch, stride):
        if not 1 <= p <= s:
            raise ValueError(f"patch must lie in [1, {s}] along {ax}, got {p}")
        if not 1 <= t <= p:
            raise ValueError(f"stride must lie in [1, patch = {p}] along {ax} (every voxel is "
                             f"covered), got {t}")
        n = max(1, -(-(s - p) // t) + 1)
        starts.append([min(i * t, s - p) for i in range(n)])
    return {"patch": patch, "stride": stride, "starts": tuple(starts)}


def window_count(windows):
    """P = n_d * n_h * n_w"""
    return math.prod(len(s) for s in windows["starts"])


def replay_count(n_windows, windows_per_replay):
    """forwards per occluded key: ceil(P / m)"""
    if n_windows < 1 or windows_per_replay < 1:
        raise ValueError("window counts are positive")
    return -(-n_windows // windows_per_replay)


def _fill_spec(fill, keys):
    """{key: a float or "mean"}"""
    def one(f, where):
        if f == "mean" and isinstance(f, str):
            return f
        if isinstance(f, (int, float)) and not isinstance(f, bool):
            return float(f)
        raise ValueError(f"fill{where} must be a number or 'mean', got {f!r}")
    if isinstance(fill, dict):
        missing = [k for k in keys if k not in fill]
        if missing:
            raise ValueError(f"fill has no entry for {missing}")
        return {k: one(fill[k], f"[{k!r}]") for k in keys}
    return {k: one(fill, "") for k in keys}


def _host_forward(model):
    """whether ``model``'s forward goes through the host (the TabPFN stage-2 / stage-3
    classes): such a forward cannot be captured"""
    from . import classifiers
    host = (classifiers._TabularStage2, classifiers.All_Modalities_Fusion)
    if isinstance(model, host):
        return True
    mods = getattr(model, "_modules", None)
    return mods is not None and any(isinstance(m, host) for m in model.modules())


def _occlusion_plan(model, batch, patch, stride, fill, score, keys, windows_per_replay, graph):
    """Every argument check of :func:`occlusion`, on the batch as given and without a launch.
    Returns ``(keys, windows, fill spec, m, capture)``."""
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    if graph not in (None, True, False):
        raise ValueError("graph must be None, True or False")
    if not isinstance(batch, dict):
        raise ValueError("batch must be the dict general_step takes")
    present = [k for k in VOLUME_KEYS if isinstance(batch.get(k), torch.Tensor)]
    if keys is None:
        keys = present
        if not keys:
            raise ValueError(f"the batch has no volume entry (one of {VOLUME_KEYS})")
    else:
        keys = [keys] if isinstance(keys, str) else list(keys)
        unknown = [k for k in keys if k not in VOLUME_KEYS]
        if unknown:
            raise ValueError(f"keys must come from {VOLUME_KEYS}, got {unknown}")
        missing = [k for k in keys if k not in present]
        if missing:
            raise ValueError(f"the batch has no volume {missing}")
        if not keys or len(set(keys)) != len(keys):
            raise ValueError("keys must name at least one volume, each once")
    shapes = {tuple(batch[k].shape) for k in keys}
    if len(shapes) != 1 or len(next(iter(shapes))) != 4:
        raise ValueError(f"the occluded volumes must share one (B, D, H, W) shape, got "
                         f"{sorted(shapes)}")
    shape = next(iter(shapes))
    windows = occlusion_windows(shape[1:], patch, stride)
    spec = _fill_spec(fill, keys)
    b = shape[0]
    if b < 1:
        raise ValueError("the batch is empty")
    if windows_per_replay is None:
        m = max(1, 8 // b)
    elif isinstance(windows_per_replay, bool) or not isinstance(windows_per_replay, int) or \
            windows_per_replay < 1:
        raise ValueError(f"windows_per_replay must be a positive int, got {windows_per_replay!r}")
    else:
        m = windows_per_replay
    if m * b > 65535:
        raise ValueError(f"windows_per_replay x batch = {m * b} forward rows exceed 65535")
    host = _host_forward(model)
    if graph and host:
        raise ValueError(f"{type(model).__name__}'s forward goes through the host (TabPFN): it "
                         "cannot be captured, use graph=None or graph=False")
    return keys, windows, spec, m, (not host if graph is None else bool(graph))


def _geometry(size, windows):
    return (*size, *windows["patch"], *windows["stride"])


def _check_vols(src, slots):
    L.require_device(src, slots)
    if src.dtype not in (torch.float64, torch.float32) or slots.dtype != src.dtype:
        raise L.MMADError(f"occlusion moves float64 or float32 volumes, got {src.dtype} / "
                          f"{slots.dtype}")
    if src.dim() != 4 or slots.dim() != 4 or slots.shape[1:] != src.shape[1:] or \
            slots.shape[0] % src.shape[0] or not src.is_contiguous() or \
            not slots.is_contiguous():
        raise L.MMADError(f"slots must be contiguous (m * B, D, H, W) over a contiguous "
                          f"(B, D, H, W) source, got {tuple(slots.shape)} / {tuple(src.shape)}")


def occlude_windows(src, slots, fill, cursor, windows):
    """Move the windows of ``slots`` ((m * B, D, H, W), slot i = sample i % B of ``src``) to
    replay position ``cursor`` (a 0-d int64 device tensor, read when the kernel runs): slot i
    gets window ``cursor + i // B`` filled with ``fill[i % B]`` and what window
    ``cursor - m + i // B`` covered outside it restored from ``src``.  In place."""
    _check_vols(src, slots)
    b, m = src.shape[0], slots.shape[0] // src.shape[0]
    L.require_device(fill, cursor)
    if fill.dtype != torch.float64 or fill.shape != (b,) or not fill.is_contiguous():
        raise L.MMADError("fill must be a contiguous (B,) float64 tensor")
    if cursor.dtype != torch.int64 or cursor.numel() != 1:
        raise L.MMADError("the cursor is one int64 on the device")
    L.call("mmad_occlude_windows", L.dtype_code(src.dtype), b, m,
           *_geometry(tuple(src.shape[1:]), windows), L.ptr(src), L.ptr(slots), L.ptr(fill),
           L.ptr(cursor), window_count(windows), L.stream())
    return slots


def occlusion_drop(logits, target, base, cursor, drops, score="logit"):
    """``drops[cursor + i // B, i % B] = base[i % B] - score(logits[i])`` for the rows of
    ``logits`` ((m * B, C) float64) whose window index lies inside ``drops`` ((P, B) float64);
    ``score``: the logit of class ``target[i % B]`` or its softmax probability.  In place."""
    L.require_device(logits, target, base, cursor, drops)
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    p, b = drops.shape
    if logits.dim() != 2 or logits.shape[0] % b or logits.dtype != torch.float64 or \
            not logits.is_contiguous():
        raise L.MMADError(f"logits must be contiguous (m * {b}, C) float64, got {logits.dtype} "
                          f"{tuple(logits.shape)}")
    if drops.dtype != torch.float64 or not drops.is_contiguous() or \
            base.dtype != torch.float64 or base.shape != (b,) or not base.is_contiguous() or \
            target.dtype != torch.int64 or target.shape != (b,) or not target.is_contiguous():
        raise L.MMADError("drops (P, B) / base (B,) are contiguous float64, target (B,) int64")
    if cursor.dtype != torch.int64 or cursor.numel() != 1:
        raise L.MMADError("the cursor is one int64 on the device")
    L.call("mmad_occlusion_drop", SCORES.index(score), b, logits.shape[0] // b, logits.shape[1],
           L.ptr(logits), L.ptr(target), L.ptr(base), L.ptr(cursor), p, L.ptr(drops), L.stream())
    return drops


def occlusion_map(drops, size, windows):
    """(P, B) float64 drops -> (B, D, H, W) float32: each voxel's mean drop over the windows
    that contain it, summed in ascending window index in float64 and rounded once."""
    L.require_device(drops)
    size = tuple(size)
    p, b = drops.shape
    if drops.dtype != torch.float64 or not drops.is_contiguous() or p != window_count(windows):
        raise L.MMADError(f"drops must be contiguous ({window_count(windows)}, B) float64, got "
                          f"{drops.dtype} {tuple(drops.shape)}")
    out = torch.empty((b,) + size, dtype=torch.float32, device=drops.device)
    L.call("mmad_occlusion_map", b, *_geometry(size, windows), L.ptr(drops), p, L.ptr(out),
           L.stream())
    return out


def _tiled(v, b, m):
    """a batch entry for m * B forward rows: row i holds sample i % B"""
    if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == b:
        return v.detach().repeat((m,) + (1,) * (v.dim() - 1)).contiguous()
    if isinstance(v, (list, tuple)) and len(v) == b:
        return type(v)(list(v) * m)
    return v


def occlusion(model, batch, target=None, patch=16, stride=None, fill=0.0, score="logit",
              keys=None, windows_per_replay=None, graph=None):
    """Occlusion sensitivity: how much the score of class ``target`` drops when a box of a
    volume is replaced by ``fill``.  Forwards only, so it covers every drop-in class (early
    fusion included), can score a probability (which still moves when the ReLU has clamped the
    logit) and answers per modality: each of ``keys`` is occluded on its own.

    patch, stride  one int or three (d, h, w); ``1 <= patch <= extent``,
                   ``1 <= stride <= patch`` (default: ``patch``); :func:`occlusion_windows`
    fill           a number, ``"mean"`` (each sample's own mean of that volume) or a dict per key
    score          ``"logit"``: the target class's output logit; ``"prob"``: its softmax
                   probability in float64
    keys           the volume entries to occlude (default: every one of ``("mri", "pet1451")``
                   in the batch); they must share one shape
    windows_per_replay  m windows of all B samples per forward (m * B rows; default
                   ``max(1, 8 // B)``): eval-mode samples are independent, so stacking windows of
                   one patient into one forward batch is exact
    graph          None: the replayed body (move the windows, ``general_step``, score the rows,
                   advance the device cursor) is captured once per key and replayed
                   ``ceil(P / m)`` times, unless the model's forward goes through the host
                   (TabPFN stages); False: the same launches issued from Python (bit-identical);
                   True on a TabPFN stage class raises ``ValueError``

    With ``s0[b]`` the score of the unoccluded batch and window ``j`` of ``P``:
    ``drop[k][j][b] = s0[b] - score(window j of volume k of sample b replaced by fill)`` and
    ``map[k][b][v]`` = the mean of ``drop[k][j][b]`` over the windows that contain voxel ``v``
    (summed in ascending ``j`` in float64, rounded to float32 once).

    Returns ``{"maps": {k: (B, D, H, W) float32}, "drops": {k: (B, n_d, n_h, n_w) float64},
    "target": (B,) int64, "score": (B,) float64 (s0), "windows": {"patch", "stride",
    "starts"}}``.  Wrong arguments raise ``ValueError`` before any launch.  Runs in eval mode
    under ``no_grad``; training flags and ``requires_grad`` are restored afterwards."""
    from .graph_step import GraphedEvalForward
    keys, windows, spec, m, capture = _occlusion_plan(
        model, batch, patch, stride, fill, score, keys, windows_per_replay, graph)
    n_win = window_count(windows)
    with _Frozen(model), torch.no_grad():
        batch, _ = _prepared(model, batch)
        src = {k: batch[k].detach().contiguous() for k in keys}
        b = src[keys[0]].shape[0]
        size = tuple(src[keys[0]].shape[1:])
        dev = src[keys[0]].device
        for k in keys:
            L.require_device(src[k])
            if src[k].dtype not in (torch.float64, torch.float32):
                raise ValueError(f"{k} must be float64 or float32, got {src[k].dtype}")
        with torch.cuda.device(dev):
            static = {k: _tiled(v, b, m) for k, v in batch.items()}
            # the base forward runs on the same m * B rows as every replay (the first B are
            # the batch itself), so an unoccluded slot scores exactly s0
            logits = model.general_step(static, 0, "pred")["outputs"].detach()
            if logits.dim() != 2 or logits.shape[0] != m * b:
                raise ValueError(f"general_step returned outputs of shape {tuple(logits.shape)} "
                                 f"for {m * b} rows")
            logits = logits.to(torch.float64).contiguous()
            tgt = _target(logits[:b], target).contiguous()
            if bool(((tgt < 0) | (tgt >= logits.shape[1])).any()):
                raise ValueError(f"target must lie in [0, {logits.shape[1]})")
            cursor = torch.zeros((), dtype=torch.int64, device=dev)
            zero = torch.zeros(b, dtype=torch.float64, device=dev)
            neg = torch.empty((1, b), dtype=torch.float64, device=dev)
            occlusion_drop(logits[:b].contiguous(), tgt, zero, cursor, neg, score)
            s0 = -neg[0]
            fills = {k: src[k].mean(dim=(1, 2, 3)).to(torch.float64) if spec[k] == "mean"
                     else torch.full((b,), spec[k], dtype=torch.float64, device=dev)
                     for k in keys}
            maps, drops = {}, {}
            for k in keys:
                table = torch.empty((n_win, b), dtype=torch.float64, device=dev)

                def move(st, k=k):
                    occlude_windows(src[k], st[k], fills[k], cursor, windows)

                def fold(out, table=table):
                    occlusion_drop(out, tgt, s0, cursor, table, score)
                    cursor.add_(m)

                step = GraphedEvalForward(model, static, before=move, after=fold,
                                          capture=capture)
                # the warm-up forwards have moved the windows and the cursor
                static[k].copy_(_tiled(src[k], b, m))
                cursor.zero_()
                for _ in range(replay_count(n_win, m)):
                    if capture:
                        step.graph.replay()
                    else:
                        step()
                maps[k] = occlusion_map(table, size, windows)
                drops[k] = table.t().reshape((b,) + tuple(len(s) for s in windows["starts"])) \
                    .contiguous()
                static[k].copy_(_tiled(src[k], b, m))
                del step
    return {"maps": maps, "drops": drops, "target": tgt, "score": s0, "windows": windows}
