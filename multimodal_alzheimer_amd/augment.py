"""Random augmentation of volume batches on device (float64), replayable in a HIP graph.

The reference augments only through CPU transforms handed to the loader (``transform_mri`` /
``transform_pet``, pkg/utils/dataloader.py): one 128^3 float64 resample per sample on a loader
worker.  Here a batch that is already on the device (and, with ``device_normalize=True``,
already normalised there: preprocess.VolumeNormalizer) gets, per sample, one random

* flip per axis, rotation about each axis, isotropic scale and translation, applied as ONE
  trilinear resample (``mmad_affine_resample3d``; a flip-only sample is an exact mirrored
  copy),
* optionally a smooth random (elastic) deformation, folded into that same resample as one more
  term of the sampling position (``mmad_deform_resample3d``): a coarse control lattice of
  displacements per sample (``mmad_elastic_draw``), interpolated trilinearly over the volume
  and shared by the co-registered volumes of a sample, and
* gain and bias per modality (``out = gain * resampled + bias``),

with every parameter drawn on the device (``mmad_augment_draw``) from a seed that is itself a
device tensor (one ``torch.randint``, as head_ops.dropout): reproducible under
``torch.manual_seed``, no host synchronisation, fresh values on every graph replay.

Coordinates are torch's: ``theta`` (B, 3, 4) is the output-to-input map of
``F.affine_grid(theta, size, align_corners=False)`` over normalised (x, y, z) = (W, H, D), and
:func:`resample` computes ``F.grid_sample(x, grid, mode='bilinear', padding_mode=padding,
align_corners=False)``.  The drawn transform is composed in voxel units, so a
rotation stays a rotation on a non-cubic volume.

Three ways in: :func:`resample` (explicit parameters), :func:`draw`, and
:class:`VolumeAugmenter` (a batch dict in, a batch dict out; ``hparams['augment']`` makes every
model's ``general_step`` apply one in ``'train'`` mode).  There is no CPU path and no backward:
the inputs are data.

Elastic semantics: ``lattice`` (B, 3, Gd, Gh, Gw) holds displacements in voxels, components in
the order (x, y, z) = (w, h, d) of ``theta``'s rows; control point ``i`` of an axis with ``G``
points sits at normalised coordinate ``-1 + 2 i / (G - 1)``.  With ``u(p)`` its trilinear
interpolation at an output voxel's normalised centre ``p``, the sampling position is
``theta (p, 1) + 2 u(p) / size`` per component; everything after that is the affine resample's.
:meth:`AugmentConfig.check_elastic` refuses settings under which the composed map could fold.

Out of scope: per-voxel noise (Box-Muller per voxel would make the resample VALU-bound),
gamma, nearest-neighbour interpolation and locked lattice borders.  The batch can come from a
device-resident dataset cache (device_cache.DeviceVolumeCache), whose fetched batch dict the
augmenter takes unchanged.
"""
import math

import torch

from . import _lib as L

VOLUME_KEYS = ("mri", "pet1451")
CONFIG_KEYS = ("flip_p", "rotate_deg", "scale", "translate_vox", "gain", "bias", "padding",
               "elastic_vox", "elastic_grid")
GRID_MIN, GRID_MAX = 2, 12
_PADDING = {"zeros": L.PAD_ZEROS, "border": L.PAD_BORDER}


def _triple(name, v, lo=0.0, hi=math.inf):
    v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(a) for a in v]
    if len(v) != 3:
        raise ValueError(f"{name} takes one value or three (axes d, h, w), got {len(v)}")
    if not all(lo <= a <= hi for a in v):
        raise ValueError(f"{name} must lie in [{lo}, {hi}], got {v}")
    return tuple(v)


def _grid(name, v):
    v = [v] * 3 if isinstance(v, (int, float)) else list(v)
    if len(v) != 3:
        raise ValueError(f"{name} takes one int or three (axes d, h, w), got {len(v)}")
    if not all(isinstance(a, int) and not isinstance(a, bool) and GRID_MIN <= a <= GRID_MAX
               for a in v):
        raise ValueError(f"{name} takes ints in [{GRID_MIN}, {GRID_MAX}], got {v}")
    return tuple(v)


def _range(name, v):
    try:
        lo, hi = (float(a) for a in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} takes a (lo, hi) pair, got {v!r}") from None
    if not lo <= hi:
        raise ValueError(f"{name}: lo must not exceed hi, got ({lo}, {hi})")
    return lo, hi


def _ranges(name, v):
    """one (lo, hi) pair for every modality, or {volume key: (lo, hi)} for all of them"""
    if isinstance(v, dict):
        if set(v) != set(VOLUME_KEYS):
            raise ValueError(f"{name} as a dict needs exactly the keys {VOLUME_KEYS}")
        return {k: _range(f"{name}[{k!r}]", v[k]) for k in VOLUME_KEYS}
    return _range(name, v)


class AugmentConfig:
    """Validated augmentation settings; every default means "off".

    ``flip_p``: flip probability per axis; ``rotate_deg``: maximum absolute angle about each
    axis; ``translate_vox``: maximum absolute shift along each axis, in voxels -- one value
    or three, axes in tensor order (d, h, w).  ``scale``: isotropic zoom range (lo, hi) of the
    output-to-input map (< 1 magnifies).  ``gain`` / ``bias``: (lo, hi), or a dict with one
    pair per volume key.  ``padding``: 'zeros' or 'border'.  ``elastic_vox``: maximum
    absolute displacement of a control point along each axis, in voxels (one value or three,
    (d, h, w)); ``elastic_grid``: control points per axis, one int or three in [2, 12]."""

    def __init__(self, flip_p=0.0, rotate_deg=0.0, scale=(1.0, 1.0), translate_vox=0.0,
                 gain=(1.0, 1.0), bias=(0.0, 0.0), padding="zeros", elastic_vox=0.0,
                 elastic_grid=7):
        self.flip_p = _triple("flip_p", flip_p, 0.0, 1.0)
        self.rotate_deg = _triple("rotate_deg", rotate_deg, 0.0, 180.0)
        self.translate_vox = _triple("translate_vox", translate_vox)
        self.scale = _range("scale", scale)
        if not self.scale[0] > 0.0:
            raise ValueError(f"scale must be positive, got {self.scale}")
        self.gain, self.bias = _ranges("gain", gain), _ranges("bias", bias)
        if padding not in _PADDING:
            raise ValueError(f"padding must be one of {tuple(_PADDING)}, got {padding!r}")
        self.padding = padding
        self.elastic_vox = _triple("elastic_vox", elastic_vox)
        self.elastic_grid = _grid("elastic_grid", elastic_grid)

    @property
    def elastic(self):
        """whether any control-point bound is non-zero"""
        return any(m != 0.0 for m in self.elastic_vox)

    def elastic_cap(self, shape):
        """The isotropic ``elastic_vox`` at which :meth:`check_elastic` starts to refuse
        volumes of extent ``shape`` = (D, H, W): ``scale_lo / (2 sqrt(3 sum_j 1 / s_j^2))``."""
        inv = sum(((g - 1) / float(n)) ** 2 for g, n in zip(self.elastic_grid, shape))
        return self.scale[0] / (2.0 * math.sqrt(3.0 * inv))

    def check_elastic(self, shape):
        """Raise ``ValueError`` if the drawn map could fold volumes of extent ``shape`` =
        (D, H, W).

        Between control points ``s_j = size_j / (G_j - 1)`` voxels apart, bounded by ``m_i``,
        component i of the trilinear displacement changes by at most ``2 m_i`` per ``s_j``
        voxels along axis j, so its Jacobian's Frobenius (hence spectral) norm is at most
        ``beta = 2 sqrt(sum_i m_i^2 sum_j 1 / s_j^2)``.  In voxel units the affine part is
        ``scale * rotation * flips``, every singular value at least ``scale_lo``: the composed
        map stays one-to-one while ``beta < scale_lo``.  (1e-12 of slack keeps the verdict at
        the cap itself independent of rounding.)"""
        shape = tuple(int(n) for n in shape)
        if len(shape) != 3 or min(shape) <= 0:
            raise ValueError(f"shape must be a positive (D, H, W), got {shape}")
        inv = sum(((g - 1) / float(n)) ** 2 for g, n in zip(self.elastic_grid, shape))
        beta = 2.0 * math.sqrt(sum(m * m for m in self.elastic_vox) * inv)
        if not beta < self.scale[0] * (1.0 - 1e-12):
            raise ValueError(
                f"elastic_vox {self.elastic_vox} with elastic_grid {self.elastic_grid} can fold "
                f"a {shape} volume at scale {self.scale[0]}: the displacement's Jacobian norm "
                f"bound {beta:.4g} must stay below the smallest scale; the largest admissible "
                f"isotropic elastic_vox for this shape is below {self.elastic_cap(shape):.4f}")

    @property
    def intensity(self):
        """whether any gain or bias can differ from (1, 0)"""
        def pairs(r):
            return list(r.values()) if isinstance(r, dict) else [r]
        return (any(p != (1.0, 1.0) for p in pairs(self.gain))
                or any(p != (0.0, 0.0) for p in pairs(self.bias)))

    def struct(self, nmod):
        if not 1 <= nmod <= L.AUG_MAX_MOD:
            raise ValueError(f"nmod must lie in [1, {L.AUG_MAX_MOD}]")
        c = L.AugmentCfg()
        c.flip_p[:] = self.flip_p
        c.rot_max[:] = [math.radians(a) for a in self.rotate_deg]
        c.scale_lo, c.scale_hi = self.scale
        c.trans_max[:] = self.translate_vox
        for name, r in (("gain", self.gain), ("bias", self.bias)):
            if isinstance(r, dict):
                if nmod != len(VOLUME_KEYS):
                    raise ValueError(f"per-key {name} ranges need nmod == {len(VOLUME_KEYS)}")
                r = [r[k] for k in VOLUME_KEYS]
            else:
                r = [r] * nmod
            for m, (lo, hi) in enumerate(r):
                getattr(c, name + "_lo")[m], getattr(c, name + "_hi")[m] = lo, hi
        c.nmod = nmod
        return c


def _no_grad(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise L.MMADError("augmentation has no backward: its inputs are data (detach them)")


def resample(x, theta, padding="zeros", gain_bias=None, lattice=None):
    """``gain * F.grid_sample(x[:, None], F.affine_grid(theta, ...), 'bilinear', padding,
    align_corners=False)[:, 0] + bias`` for float64 device volumes ``x`` (B, D, H, W),
    ``theta`` (B, 3, 4) and, optionally, ``gain_bias`` (B, 2) (a view with any row stride
    will do).  A sample whose theta is exactly a flip is mirrored bit-exactly.

    With ``lattice`` (contiguous float64 (B, 3, Gd, Gh, Gw), voxels, extents in [2, 12]) the
    grid gains ``2 u / size``, ``u`` the lattice interpolated trilinearly over the volume (module
    docstring); a zero lattice gives the affine general path's result bit for bit, and no
    sample is mirrored."""
    L.require_device(x, theta, gain_bias, lattice)
    _no_grad(x, theta, gain_bias, lattice)
    if padding not in _PADDING:
        raise ValueError(f"padding must be one of {tuple(_PADDING)}, got {padding!r}")
    if x.ndim != 4 or x.dtype != torch.float64 or not x.is_contiguous():
        raise L.MMADError("volumes must be contiguous float64 (B, D, H, W) tensors")
    b, d, h, w = x.shape
    if theta.shape != (b, 3, 4) or theta.dtype != torch.float64 or not theta.is_contiguous():
        raise L.MMADError(f"theta must be a contiguous float64 ({b}, 3, 4) tensor")
    stride = 0
    if gain_bias is not None:
        if (gain_bias.shape != (b, 2) or gain_bias.dtype != torch.float64
                or gain_bias.stride(1) != 1 or gain_bias.stride(0) < 0):
            raise L.MMADError(f"gain_bias must be a float64 ({b}, 2) tensor with unit inner "
                              "stride")
        stride = gain_bias.stride(0)
    if lattice is not None:
        if (lattice.ndim != 5 or lattice.shape[:2] != (b, 3) or lattice.dtype != torch.float64
                or not lattice.is_contiguous() or lattice.device != x.device
                or not all(GRID_MIN <= g <= GRID_MAX for g in lattice.shape[2:])):
            raise L.MMADError(f"lattice must be a contiguous float64 ({b}, 3, Gd, Gh, Gw) tensor "
                              f"on the volumes' device, extents in [{GRID_MIN}, {GRID_MAX}]")
    out = torch.empty_like(x)
    if lattice is not None:
        L.call("mmad_deform_resample3d", b, d, h, w, L.ptr(x), L.ptr(theta), *lattice.shape[2:],
               L.ptr(lattice), L.ptr(gain_bias), stride, _PADDING[padding], L.ptr(out),
               L.stream())
    else:
        L.call("mmad_affine_resample3d", b, d, h, w, L.ptr(x), L.ptr(theta), L.ptr(gain_bias),
               stride, _PADDING[padding], L.ptr(out), L.stream())
    return out


def draw(cfg, batch_size, shape, device, nmod=1, return_lattice=False):
    """Draw one transform per sample for volumes of extent ``shape`` = (D, H, W): returns
    ``(theta, intensity)``, float64 (B, 3, 4) and (B, nmod, 2) = (gain, bias).  ``cfg``: an
    :class:`AugmentConfig` or its keyword dict.  With ``return_lattice`` the result is
    ``(theta, intensity, lattice)``, the elastic control lattice (B, 3, Gd, Gh, Gw) or ``None``
    when elastic is off; it comes from the same seed, so ``theta`` and ``intensity`` are what
    they are without it."""
    if not isinstance(cfg, AugmentConfig):
        cfg = AugmentConfig(**cfg)
    device = torch.device(device)
    if device.type != "cuda":
        raise L.MMADError(f"augmentation parameters are drawn on HIP devices only (got {device})")
    d, h, w = (int(s) for s in shape)
    c = cfg.struct(nmod)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device)
    theta = torch.empty((batch_size, 3, 4), dtype=torch.float64, device=device)
    intensity = torch.empty((batch_size, nmod, 2), dtype=torch.float64, device=device)
    L.call("mmad_augment_draw", batch_size, d, h, w, c, L.ptr(seed), L.ptr(theta),
           L.ptr(intensity), L.stream())
    if not return_lattice:
        return theta, intensity
    lattice = None
    if cfg.elastic:
        lattice = torch.empty((batch_size, 3) + cfg.elastic_grid, dtype=torch.float64,
                              device=device)
        L.call("mmad_elastic_draw", batch_size, *cfg.elastic_grid, *cfg.elastic_vox, L.ptr(seed),
               L.ptr(lattice), L.stream())
    return theta, intensity, lattice


class VolumeAugmenter:
    """Augment a device batch dict: ``VolumeAugmenter(**cfg)(batch)`` (keys of
    :class:`AugmentConfig`).

    One draw per call.  Every volume key present (:data:`VOLUME_KEYS`) gets the SAME spatial
    transform -- the MRI and PET of one subject are co-registered and must move together --
    and its own gain and bias; every other entry passes through.  ``theta`` / ``intensity``
    hold the last draw (``intensity[:, m]`` belongs to ``VOLUME_KEYS[m]``); inside a captured
    graph they are the graph's buffers, rewritten by each replay.  With elastic on, so does
    ``lattice`` (one per call, shared by every volume key; ``None`` otherwise), and a setting
    that could fold the batch's volumes raises before anything is launched."""

    def __init__(self, **cfg):
        unknown = sorted(set(cfg) - set(CONFIG_KEYS))
        if unknown:
            raise ValueError(f"unknown augmentation settings {unknown}; known: {CONFIG_KEYS}")
        self.cfg = AugmentConfig(**cfg)
        self.theta = self.intensity = self.lattice = None

    def __call__(self, batch):
        vols = [(m, k) for m, k in enumerate(VOLUME_KEYS) if batch.get(k) is not None]
        if not vols:
            return batch
        xs = [batch[k] for _, k in vols]
        L.require_device(*xs)
        if any(x.shape != xs[0].shape for x in xs):
            raise L.MMADError("volumes that share a spatial transform must share a shape")
        if xs[0].ndim != 4:
            raise L.MMADError("volumes must be (B, D, H, W) tensors")
        if self.cfg.elastic:
            self.cfg.check_elastic(xs[0].shape[1:])
        self.theta, self.intensity, self.lattice = draw(
            self.cfg, xs[0].shape[0], xs[0].shape[1:], xs[0].device, nmod=len(VOLUME_KEYS),
            return_lattice=True)
        out = dict(batch)
        for m, k in vols:
            gb = self.intensity[:, m] if self.cfg.intensity else None
            out[k] = resample(batch[k], self.theta, self.cfg.padding, gb, self.lattice)
        return out
