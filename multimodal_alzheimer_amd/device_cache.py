"""A dataset kept in HBM: ``MultiModalDataset``'s volumes stored once, compact but exact, and
every batch assembled on the device from an index -- inside the captured step graph if wanted.

The reference feeds training through a host ``DataLoader``: per sample a NIfTI read and
nibabel's ``get_fdata`` widening to float64 on a worker (pkg/utils/dataloader.py:197-211), per
batch a collate and one host-to-device copy.  At thousands of volumes per second that, not the
GPU, bounds a real run (a 128^3 float64 volume is 16.8 MB).  The data fits on the card many
times over, so here it is loaded once:

* :meth:`DeviceVolumeCache.from_dataset` walks a ``MultiModalDataset(device_normalize=True)``
  (raw volumes; the device normaliser still runs after the fetch) and narrows every scan into a
  store whose dtype loses nothing: the store kernel (csrc/cache.hip) widens each stored voxel
  again and counts the ones that differ from the source in any bit.  ``storage='auto'`` keeps
  float32 when that count is zero over the whole dataset and float64 otherwise; an explicit
  narrower dtype that is not exact raises :class:`CacheInexact` unless ``lossy=True``.  Binary
  brain masks are stored as one bit per voxel.
* :meth:`DeviceVolumeCache.fetch` returns the batch dict that collating ``ds[i]`` for the given
  indices and moving it to the device would give (same keys, dtypes and values), optionally
  centre-padded / cropped to ``out_shape``.
* :meth:`DeviceVolumeCache.feed` returns a :class:`CacheFeed`: the sample order of
  ``data_parallel.shard_indices`` per epoch as a device array plus a device cursor, which the
  fetch kernels read when they run.  ``fetch_into`` + the cursor's increment can be captured,
  so a replayed graph (``graph_step.GraphedTrainStep(feed=...)``) fetches its own next batch
  with no host work and no copy.

Layout (include/mmad.h): slot ``s`` of a store starts at byte ``s * stride``, ``stride`` = the
scan's bytes rounded up to 16; mask bits take ``ceil(vox / 8)`` bytes rounded the same way.
There is no CPU path: the stores live on a HIP device.  The byte accounting, the index
validation and a feed's host-side order need no device.
"""
import torch

from . import _lib as L
from .data_parallel import shard_indices
from .preprocess import NORM_SPEC_KEY

VOLUME_KEYS = ("pet1451", "mri")
MASK_KEY = "mri_mask"
TABULAR_COLS = 9
BATCH_ORDER = ("pet1451", "mri", MASK_KEY, "tabular", "label", NORM_SPEC_KEY)
STORAGE = {"float64": (L.F64, 8, torch.float64), "float32": (L.F32, 4, torch.float32),
           "float16": (L.F16, 2, torch.float16)}
_AUTO_ORDER = ("float32", "float64")
DEFAULT_BUDGET_FRACTION = 0.8
_STAGING_BYTES = 256 << 20          # float64 scans uploaded per chunk of the fill


class CacheInexact(ValueError):
    """The requested storage dtype does not hold the data exactly; ``mismatches`` is the number
    of voxels that would change (``per_key`` splits it by batch key)."""

    def __init__(self, storage, per_key):
        self.storage, self.per_key = storage, dict(per_key)
        self.mismatches = sum(self.per_key.values())
        super().__init__(f"{self.mismatches} voxel(s) do not survive {storage} storage exactly "
                         f"({self.per_key}); use storage='auto' / 'float64', or lossy=True")


class CacheBudgetError(MemoryError):
    """The cache would not fit the byte budget; ``needed`` and ``budget`` are in bytes."""

    def __init__(self, needed, budget, detail):
        self.needed, self.budget = int(needed), int(budget)
        super().__init__(f"the device cache needs {self.needed} bytes ({detail}) but the budget "
                         f"is {self.budget} bytes")


# ------------------------------------------------------------------------ byte accounting
def _round16(nbytes):
    return (int(nbytes) + 15) // 16 * 16


def scan_stride_bytes(vox, storage):
    """bytes between consecutive scans of a value store: the scan rounded up to 16"""
    if storage not in STORAGE:
        raise ValueError(f"storage must be one of {tuple(STORAGE)}, got {storage!r}")
    if vox <= 0:
        raise ValueError("a scan needs at least one voxel")
    return _round16(vox * STORAGE[storage][1])


def mask_stride_bytes(vox):
    """bytes between consecutive bit-packed masks: ceil(vox / 8) rounded up to 16"""
    if vox <= 0:
        raise ValueError("a scan needs at least one voxel")
    return _round16(-(-vox // 8))


def chunk_scans(n, vox):
    """scans uploaded per chunk of the fill (a float64 staging buffer of at most 256 MiB)"""
    return max(1, min(int(n), _STAGING_BYTES // (vox * 8)))


def required_bytes(n, vox, volumes, storage, mask=None, tabular=False):
    """Device bytes of a cache of ``n`` samples: ``volumes`` value stores in ``storage``, a mask
    (``'bits'``, ``'values'`` or None), the label / tabular tables and the fill's staging
    chunk.  Returns ``(total, {part: bytes})``."""
    if n <= 0:
        raise ValueError("a cache needs at least one sample")
    if mask not in (None, "bits", "values"):
        raise ValueError("mask must be None, 'bits' or 'values'")
    parts = {"volumes": n * volumes * scan_stride_bytes(vox, storage), "labels": n * 8}
    if mask is not None:
        parts["mask"] = n * (mask_stride_bytes(vox) if mask == "bits"
                             else scan_stride_bytes(vox, storage))
    if tabular:
        parts["tabular"] = n * TABULAR_COLS * 8
    parts["staging"] = chunk_scans(n, vox) * vox * 8
    return sum(parts.values()), parts


def validate_indices(indices, n):
    """``indices`` (a host sequence of ints or a CPU integer tensor) as a non-empty int64 CPU
    tensor with every entry in [0, n); ``IndexError`` otherwise.  Negative indices are out of
    range (a sampler never produces them)."""
    if torch.is_tensor(indices):
        if indices.device.type != "cpu":
            raise TypeError("indices are validated on the host: pass a CPU tensor or a sequence")
        if indices.dtype.is_floating_point or indices.dtype.is_complex or \
                indices.dtype == torch.bool:
            raise TypeError(f"indices must be integers, got {indices.dtype}")
        idx = indices.to(torch.int64).reshape(-1)
    else:
        vals = []
        for i in indices:
            if isinstance(i, bool) or not hasattr(i, "__index__"):
                raise TypeError(f"indices must be integers, got {type(i).__name__}")
            vals.append(i.__index__())
        idx = torch.tensor(vals, dtype=torch.int64)
    if idx.numel() == 0:
        raise IndexError("an empty index list selects no batch")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n:
        raise IndexError(f"sample index {lo if lo < 0 else hi} is outside [0, {n})")
    return idx


def _shape3(name, shape):
    try:
        s = tuple(int(a) for a in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three positive extents (D, H, W)") from None
    if len(s) != 3 or any(a <= 0 for a in s):
        raise ValueError(f"{name} must be three positive extents (D, H, W), got {shape!r}")
    return s


def _check_args(storage, lossy, budget_bytes):
    if storage != "auto" and storage not in STORAGE:
        raise ValueError(f"storage must be 'auto' or one of {tuple(STORAGE)}, got {storage!r}")
    if lossy and storage == "auto":
        raise ValueError("lossy=True needs an explicit storage dtype ('auto' is always exact)")
    if budget_bytes is not None and budget_bytes <= 0:
        raise ValueError("budget_bytes must be positive")


# ------------------------------------------------------------------------------ sources
class _TensorSource:
    """in-memory float64 arrays, chunked"""

    def __init__(self, arrays, label, spec):
        self.arrays, self.label, self.spec = arrays, label, spec
        self.n = int(label.shape[0])

    def first(self):
        out = {k: v[0] for k, v in self.arrays.items()}
        out["label"] = self.label[0]
        return out

    def chunks(self, size, num_workers=0):
        for s in range(0, self.n, size):
            out = {k: v[s:s + size] for k, v in self.arrays.items()}
            out["label"] = self.label[s:s + size]
            yield out


class _DatasetSource:
    """a MultiModalDataset walked in table order through a DataLoader (its collate)"""

    def __init__(self, ds):
        self.ds, self.n = ds, len(ds)
        self._first = None
        self.spec = None

    def first(self):
        if self._first is None:
            self._first = self.ds[0]
            self.spec = self._first.get(NORM_SPEC_KEY)
        return self._first

    def chunks(self, size, num_workers=0):
        loader = torch.utils.data.DataLoader(self.ds, batch_size=size, shuffle=False,
                                             num_workers=num_workers)
        for batch in loader:
            yield batch


class DeviceVolumeCache:
    """The stores of one dataset on one device; build with :meth:`from_dataset` or
    :meth:`from_tensors`.

    Attributes: ``n`` samples of extent ``in_shape``, fetched at ``out_shape``; ``storage``
    (the volumes' dtype name); ``mask_storage`` (``'bits'``, a dtype name, or None);
    ``nbytes`` (the stores' device bytes) and ``plan`` (the accounting they were checked
    against); ``passes`` (how many times the fill walked the data)."""

    def __init__(self):
        raise TypeError("use DeviceVolumeCache.from_dataset(...) or .from_tensors(...)")

    # ---------------------------------------------------------------------- construction
    @classmethod
    def from_dataset(cls, ds, device, storage="auto", out_shape=None, budget_bytes=None,
                     num_workers=0, lossy=False):
        """Load ``ds`` (a ``MultiModalDataset`` built with ``device_normalize=True``, so that
        ``ds[i]`` holds the raw volumes) into ``device``'s memory.  One walk over the table in
        chunks; a second one only when ``'auto'`` has to widen to float64 or a mask turns out
        not to be binary."""
        _check_args(storage, lossy, budget_bytes)
        if not getattr(ds, "device_normalize", False):
            raise ValueError("build the dataset with device_normalize=True: the cache stores the "
                             "raw volumes and the device normaliser runs after the fetch")
        if getattr(ds, "transform_pet", None) or getattr(ds, "transform_mri", None) or \
                getattr(ds, "transform_tabular", None):
            raise ValueError("a cached dataset is read once: host transforms would be frozen "
                             "(augment on the device, augment.VolumeAugmenter)")
        if len(ds) == 0:
            raise ValueError("the dataset is empty")
        return cls._build(_DatasetSource(ds), device, storage, out_shape, budget_bytes,
                          num_workers, lossy)

    @classmethod
    def from_tensors(cls, label, pet1451=None, mri=None, mri_mask=None, tabular=None, spec=None,
                     device="cuda", storage="auto", out_shape=None, budget_bytes=None,
                     lossy=False):
        """The same from in-memory arrays: volumes and mask float64 ``(N, D, H, W)``, ``tabular``
        ``(N, 9)``, ``label`` ``(N,)`` integers; ``spec`` is the normalisation settings string
        (``preprocess.spec_string``) every fetched batch should carry, or None."""
        _check_args(storage, lossy, budget_bytes)
        arrays = {}
        for k, v in (("pet1451", pet1451), ("mri", mri), (MASK_KEY, mri_mask),
                     ("tabular", tabular)):
            if v is not None:
                arrays[k] = torch.as_tensor(v)
        label = torch.as_tensor(label)
        if label.ndim != 1 or label.dtype.is_floating_point or label.shape[0] == 0:
            raise ValueError("label must be a non-empty 1-D integer array")
        for k, v in arrays.items():
            if v.shape[0] != label.shape[0]:
                raise ValueError(f"{k} holds {v.shape[0]} samples, label {label.shape[0]}")
        if MASK_KEY in arrays and "mri" not in arrays:
            raise ValueError("mri_mask needs mri")
        return cls._build(_TensorSource(arrays, label, spec), device, storage, out_shape,
                          budget_bytes, 0, lossy)

    @classmethod
    def _build(cls, source, device, storage, out_shape, budget_bytes, num_workers, lossy):
        self = object.__new__(cls)
        first = source.first()
        vols = [k for k in VOLUME_KEYS if k in first]
        if not vols:
            raise ValueError("nothing to cache: the samples hold neither 'mri' nor 'pet1451'")
        shape = _shape3("the volume shape", first[vols[0]].shape)
        for k in vols + ([MASK_KEY] if MASK_KEY in first else []):
            v = first[k]
            if tuple(v.shape) != shape:
                raise ValueError(f"{k} has shape {tuple(v.shape)}, {vols[0]} has {shape}")
            if v.dtype != torch.float64:
                raise ValueError(f"{k} must be float64 (the loader's dtype), got {v.dtype}")
        self.n, self.in_shape = source.n, shape
        self.out_shape = shape if out_shape is None else _shape3("out_shape", out_shape)
        self.volume_keys = tuple(vols)
        self.has_mask = MASK_KEY in first
        self.has_tabular = "tabular" in first
        if self.has_tabular and tuple(first["tabular"].shape) != (TABULAR_COLS,):
            raise ValueError(f"tabular rows hold {TABULAR_COLS} values")
        self.tabular_dtype = first["tabular"].dtype if self.has_tabular else None
        self.label_dtype = first["label"].dtype
        self.spec = source.spec
        self.device = torch.device(device)
        vox = shape[0] * shape[1] * shape[2]
        self.vox = vox

        # the plan is checked against the budget before anything is allocated
        self.storage = _AUTO_ORDER[0] if storage == "auto" else storage
        self.mask_storage = "bits" if self.has_mask else None
        budget = budget_bytes
        self.passes = 0
        while True:
            total, parts = self._plan()
            if budget is None:
                if self.device.type != "cuda":
                    raise L.MMADError(f"the cache lives on a HIP device (got {self.device})")
                budget = int(DEFAULT_BUDGET_FRACTION * torch.cuda.mem_get_info(self.device)[0])
            if total > budget:
                raise CacheBudgetError(total, budget, ", ".join(
                    f"{k} {v}" for k, v in parts.items()) + f"; {self.n} samples of {shape} in "
                    f"{self.storage}")
            if self.device.type != "cuda":
                raise L.MMADError(f"the cache lives on a HIP device (got {self.device})")
            self.plan = parts
            counts = self._fill(source, num_workers)
            self.passes += 1
            inexact = {k: counts[k] for k in self.volume_keys if counts[k]}
            if self.has_mask and self.mask_storage != "bits" and counts[MASK_KEY]:
                inexact[MASK_KEY] = counts[MASK_KEY]
            redo = False
            if inexact:
                if storage == "auto" and self.storage != _AUTO_ORDER[-1]:
                    self.storage = _AUTO_ORDER[_AUTO_ORDER.index(self.storage) + 1]
                    redo = True
                elif not lossy:
                    raise CacheInexact(self.storage, inexact)
            if self.has_mask and self.mask_storage == "bits" and counts["mask_nonbinary"]:
                self.mask_storage = "values"          # resolved to the volumes' dtype below
                redo = True
            if not redo:
                break
            self._stores = None                       # free before the wider plan is allocated
        if self.mask_storage == "values":
            self.mask_storage = self.storage
        self.mismatches = {k: counts[k] for k in self.volume_keys}
        self.nbytes = sum(t.numel() * t.element_size() for t in self._stores.values())
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self

    def _plan(self):
        mask = None if not self.has_mask else ("bits" if self.mask_storage == "bits" else "values")
        return required_bytes(self.n, self.vox, len(self.volume_keys), self.storage, mask,
                              self.has_tabular)

    def _kind(self, key):
        if key == MASK_KEY and self.mask_storage == "bits":
            return L.BITS
        return STORAGE[self.storage][0]

    def _stride(self, key):
        if key == MASK_KEY and self.mask_storage == "bits":
            return mask_stride_bytes(self.vox)
        return scan_stride_bytes(self.vox, self.storage)

    def _fill(self, source, num_workers):
        """one walk over the data: upload float64 chunks, narrow them into the stores, read
        the counters once at the end"""
        dev, n, vox = self.device, self.n, self.vox
        lib = L.load()
        keys = list(self.volume_keys) + ([MASK_KEY] if self.has_mask else [])
        stores = {}
        for k in keys:
            stride = self._stride(k)
            if stride != lib.mmad_cache_stride_bytes(self._kind(k), vox):
                raise L.MMADError("store stride disagrees with the library's")
            stores[k] = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        stores["label"] = torch.empty(n, dtype=torch.int64, device=dev)
        if self.has_tabular:
            stores["tabular"] = torch.empty((n, TABULAR_COLS), dtype=torch.float64, device=dev)
        names = keys + ["mask_nonbinary"]
        counters = torch.zeros(len(names), dtype=torch.int64, device=dev)
        ws = torch.empty(lib.mmad_cache_ws_bytes(), dtype=torch.uint8, device=dev)
        slot = 0
        with torch.cuda.device(dev):
            for chunk in source.chunks(chunk_scans(n, vox), num_workers):
                c = int(chunk["label"].shape[0])
                if slot + c > n:
                    raise L.MMADError("the data source yielded more samples than its length")
                for k in keys:
                    x = chunk[k]
                    if tuple(x.shape) != (c,) + self.in_shape:
                        raise ValueError(f"sample {slot}..: {k} has shape {tuple(x.shape[1:])}, "
                                         f"the first sample {self.in_shape}")
                    x = x.to(dev, torch.float64).contiguous()
                    cnt = counters[names.index(k):]
                    if k == MASK_KEY and self.mask_storage == "bits":
                        L.call("mmad_cache_pack_mask", c, vox, L.ptr(x), L.ptr(stores[k]), slot,
                               n, L.ptr(counters[len(names) - 1:]), L.ptr(ws), L.stream())
                    else:
                        L.call("mmad_cache_store", self._kind(k), c, vox, L.ptr(x),
                               L.ptr(stores[k]), slot, n, L.ptr(cnt), L.ptr(ws), L.stream())
                    # the staging chunk is reused by the allocator only in stream order
                stores["label"][slot:slot + c] = chunk["label"].to(dev, torch.int64)
                if self.has_tabular:
                    stores["tabular"][slot:slot + c] = chunk["tabular"].to(dev, torch.float64)
                if isinstance(source, _DatasetSource) and NORM_SPEC_KEY in chunk:
                    if len(set(chunk[NORM_SPEC_KEY])) != 1 or chunk[NORM_SPEC_KEY][0] != self.spec:
                        raise ValueError("samples carry different normalisation settings")
                slot += c
        if slot != n:
            raise L.MMADError(f"the data source yielded {slot} samples, its length is {n}")
        host = counters.cpu().tolist()                # the fill's one read of the device
        self._stores = stores
        return dict(zip(names, host))

    # ----------------------------------------------------------------------------- fetch
    def __len__(self):
        return self.n

    @property
    def keys(self):
        """the tensor keys of a fetched batch, in the dataset's order"""
        have = set(self.volume_keys) | {"label"}
        if self.has_mask:
            have.add(MASK_KEY)
        if self.has_tabular:
            have.add("tabular")
        return tuple(k for k in BATCH_ORDER if k in have)

    def store_bytes(self, key):
        """device bytes of one key's store"""
        t = self._stores[key]
        return t.numel() * t.element_size()

    def empty_batch(self, batch_size):
        """a batch dict of the fetched layout with uninitialised tensors"""
        out = {}
        for k in self.keys:
            if k == "label":
                out[k] = torch.empty(batch_size, dtype=self.label_dtype, device=self.device)
            elif k == "tabular":
                out[k] = torch.empty((batch_size, TABULAR_COLS), dtype=self.tabular_dtype,
                                     device=self.device)
            else:
                out[k] = torch.empty((batch_size,) + self.out_shape, dtype=torch.float64,
                                     device=self.device)
        if self.spec is not None:
            out[NORM_SPEC_KEY] = [self.spec] * batch_size
        return out

    def _launch(self, out, order, cursor, scratch=None):
        """the fetch launches for one batch: ``out`` (tensors of ``empty_batch``'s layout) from
        ``order[cursor + b]``; ``cursor`` None reads from position 0"""
        b = int(out["label"].shape[0])
        olen = order.numel()
        L.require_device(order, cursor, *[v for v in out.values() if torch.is_tensor(v)])
        if order.dtype != torch.int64 or not order.is_contiguous():
            raise L.MMADError("the order must be a contiguous int64 device tensor")
        st = L.stream()
        for k in self.keys:
            if k in ("label", "tabular"):
                continue
            o = out[k]
            if o.shape != (b,) + self.out_shape or o.dtype != torch.float64 or \
                    not o.is_contiguous():
                raise L.MMADError(f"{k}: the batch buffer must be contiguous float64 "
                                  f"{(b,) + self.out_shape}, got {o.dtype} {tuple(o.shape)}")
            L.call("mmad_cache_fetch", self._kind(k), b, self.n, *self.in_shape, *self.out_shape,
                   L.ptr(self._stores[k]), L.ptr(order), L.ptr(cursor), olen, L.ptr(o),
                   L.ptr(self._bad), st)
        lab, tab = out["label"], out.get("tabular")
        if lab.shape != (b,) or not lab.is_contiguous():
            raise L.MMADError(f"label: the batch buffer must be a contiguous ({b},) tensor")
        lab64 = lab if lab.dtype == torch.int64 else scratch["label"]
        tab64 = None
        if self.has_tabular:
            if tab.shape != (b, TABULAR_COLS) or not tab.is_contiguous():
                raise L.MMADError(f"tabular: the batch buffer must be contiguous "
                                  f"({b}, {TABULAR_COLS})")
            tab64 = tab if tab.dtype == torch.float64 else scratch["tabular"]
        L.call("mmad_cache_fetch_rows", b, self.n, TABULAR_COLS if self.has_tabular else 0,
               L.ptr(self._stores["label"]), L.ptr(self._stores.get("tabular")), L.ptr(order),
               L.ptr(cursor), olen, L.ptr(lab64), L.ptr(tab64), L.ptr(self._bad), st)
        if lab64 is not lab:
            lab.copy_(lab64)
        if tab64 is not None and tab64 is not tab:
            tab.copy_(tab64)                          # float64 -> the dataset's dtype, exact

    def _scratch(self, batch_size):
        """float64 / int64 landing buffers for rows whose dataset dtype is another one"""
        s = {}
        if self.label_dtype != torch.int64:
            s["label"] = torch.empty(batch_size, dtype=torch.int64, device=self.device)
        if self.has_tabular and self.tabular_dtype != torch.float64:
            s["tabular"] = torch.empty((batch_size, TABULAR_COLS), dtype=torch.float64,
                                       device=self.device)
        return s

    def fetch(self, indices):
        """The batch that collating ``[ds[i] for i in indices]`` and moving it to the device
        would give.  ``indices``: a host sequence or CPU tensor, validated here
        (``IndexError`` when out of range)."""
        idx = validate_indices(indices, self.n)
        with torch.cuda.device(self.device):
            order = idx.to(self.device)
            out = self.empty_batch(idx.numel())
            self._launch(out, order, None, self._scratch(idx.numel()))
        return out

    def bad_index_seen(self):
        """whether any fetch kernel met an index or an order position out of range (reads the
        device: a diagnostic, not part of the step)"""
        return bool(self._bad.item())

    def feed(self, batch_size, rank=0, world=1, shuffle=True, seed=15, drop_last=True,
             pad_last=False):
        return CacheFeed(self, batch_size, rank, world, shuffle, seed, drop_last, pad_last)


class CacheFeed:
    """This rank's batches of a :class:`DeviceVolumeCache`, epoch after epoch, in the order a
    ``DataLoader(ds, batch_size, sampler=ShardSampler(ds, rank, world, shuffle, seed),
    drop_last=drop_last)`` would deliver them.

    The epoch's order (``data_parallel.shard_indices``) is computed on the host and uploaded
    from pinned memory without a synchronisation; a device cursor marks the next batch.  Steps
    are counted on the host, so the epoch boundary is known without reading the device.

    * eager: ``for batch in feed`` yields the rest of the current epoch and moves to the next;
      :meth:`next_batch` returns one batch;
    * captured: :meth:`fetch_into` (the fetch launches, then ``cursor += batch_size``) is what
      ``GraphedTrainStep(feed=...)`` captures at the head of its step; it calls
      :meth:`before_replay` ahead of every replay, which rolls the epoch over when the
      previous one is used up.

    ``drop_last=False, pad_last=True`` gives full-shape batches over a ragged epoch, for a
    captured evaluation that must see every sample: the device order is padded to
    ``steps_per_epoch * batch_size`` entries by repeating the epoch's last index (every fetch
    stays in range), :meth:`fetch_into` is allowed, and :attr:`valid_rows` says how many of the
    epoch's rows are real -- the ``limit`` of a ``metrics.EpochMeter``, which ignores the rest.
    The eager paths (:meth:`next_batch`, iteration, :meth:`epoch_batches`) are unchanged: their
    last batch is short.

    The device state is created on first use; :meth:`epoch_order` / :meth:`epoch_batches` /
    :meth:`padded_order` are host-only."""

    def __init__(self, cache, batch_size, rank=0, world=1, shuffle=True, seed=15, drop_last=True,
                 pad_last=False):
        batch_size, rank, world = int(batch_size), int(rank), int(world)
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        if world <= 0 or not 0 <= rank < world:
            raise ValueError(f"rank must lie in [0, world), got rank {rank} of {world}")
        self.cache, self.n = cache, int(cache.n)
        self.batch_size, self.rank, self.world = batch_size, rank, world
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.pad_last = bool(pad_last)
        if self.pad_last and self.drop_last:
            raise ValueError("pad_last pads the short last batch that drop_last=True drops: "
                             "pass drop_last=False with it")
        self.per_rank = -(-self.n // world)
        self.steps_per_epoch = (self.per_rank // batch_size if drop_last
                                else -(-self.per_rank // batch_size))
        if self.steps_per_epoch == 0:
            raise ValueError(f"this rank's {self.per_rank} samples do not fill one batch of "
                             f"{batch_size} (drop_last=True)")
        self.epoch, self.step = 0, 0
        self._order = self._cursor = self._scratch = None

    # ------------------------------------------------------------------------- host side
    def epoch_order(self, epoch):
        """this rank's sample indices of ``epoch``"""
        return shard_indices(self.n, self.rank, self.world, epoch, self.shuffle, self.seed)

    def epoch_batches(self, epoch):
        """the index lists of ``epoch``'s batches (the last one short without drop_last)"""
        o, b = self.epoch_order(epoch), self.batch_size
        return [o[s * b:(s + 1) * b] for s in range(self.steps_per_epoch)]

    def __len__(self):
        return self.steps_per_epoch

    @property
    def valid_rows(self):
        """the samples one epoch of this feed delivers (padding rows of ``pad_last`` left out)"""
        return self.steps_per_epoch * self.batch_size if self.drop_last else self.per_rank

    @property
    def order_len(self):
        """entries of the device order"""
        return self.steps_per_epoch * self.batch_size if self.pad_last else self.per_rank

    def padded_order(self, epoch):
        """the device order of ``epoch``: :meth:`epoch_order`, with ``pad_last`` followed by
        repeats of its last index up to ``steps_per_epoch * batch_size`` entries"""
        o = list(self.epoch_order(epoch))
        return o + o[-1:] * (self.order_len - len(o))

    # ----------------------------------------------------------------------- device side
    def _ensure(self):
        if self._order is None:
            dev = self.cache.device
            self._order = torch.empty(self.order_len, dtype=torch.int64, device=dev)
            self._cursor = torch.zeros((), dtype=torch.int64, device=dev)
            self._scratch = self.cache._scratch(self.batch_size)
            self._upload()

    def _upload(self):
        host = torch.tensor(self.padded_order(self.epoch), dtype=torch.int64).pin_memory()
        # stream-ordered behind the fetches of the epoch before; the pinned block goes back to
        # torch's host allocator, which reuses it only after this copy has run
        self._order.copy_(host, non_blocking=True)
        self._cursor.zero_()

    def prepare(self):
        """create the device state (order, cursor) and launch the fetch kernels once into a
        throw-away batch, so that a capture that follows records launches only"""
        first = self._order is None
        self._ensure()
        if first:
            with torch.cuda.device(self.cache.device):
                self.cache._launch(self.cache.empty_batch(self.batch_size), self._order,
                                   self._cursor, self._scratch)
        return self

    def set_epoch(self, epoch):
        """start ``epoch`` from its first batch"""
        self.epoch, self.step = int(epoch), 0
        if self._order is not None:
            self._upload()
        return self

    def next_epoch(self):
        """upload the next epoch's order and zero the cursor (asynchronous)"""
        return self.set_epoch(self.epoch + 1)

    def _tick(self):
        if self.step >= self.steps_per_epoch:
            self.next_epoch()
        self.step += 1

    def before_replay(self):
        """host bookkeeping for one replay of a graph that holds :meth:`fetch_into`"""
        self._ensure()
        self._tick()

    def fetch_into(self, static):
        """Fetch the next batch into ``static``'s tensors (the cache's keys; shapes of
        ``cache.empty_batch(batch_size)``) and advance the device cursor.  Capturable: under
        stream capture only the launches are recorded, and every replay is announced with
        :meth:`before_replay`; run eagerly, the call counts as a step itself."""
        if not self.drop_last and not self.pad_last and self.per_rank % self.batch_size:
            raise ValueError("fetch_into needs full batches: build the feed with drop_last=True "
                             "(or drop_last=False, pad_last=True)")
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self._order is None:
            raise RuntimeError("call feed.prepare() before capturing fetch_into")
        self._ensure()
        missing = [k for k in self.cache.keys if not torch.is_tensor(static.get(k))]
        if missing:
            raise KeyError(f"the batch buffers lack {missing}")
        if not capturing:
            self._tick()
        with torch.cuda.device(self.cache.device):
            self.cache._launch(static, self._order, self._cursor, self._scratch)
            self._cursor.add_(self.batch_size)
        return static

    def peek(self):
        """the next batch in fresh tensors, without advancing"""
        self._ensure()
        if self.step >= self.steps_per_epoch:
            return self.cache.fetch(self.epoch_batches(self.epoch + 1)[0])
        return self.cache.fetch(self.epoch_batches(self.epoch)[self.step])

    def next_batch(self):
        """the next batch in fresh tensors (eager use)"""
        self._ensure()
        self._tick()
        b = min(self.batch_size, self.per_rank - (self.step - 1) * self.batch_size)
        with torch.cuda.device(self.cache.device):
            out = self.cache.empty_batch(b)
            scratch = self._scratch if b == self.batch_size else self.cache._scratch(b)
            self.cache._launch(out, self._order, self._cursor, scratch)
            self._cursor.add_(b)
        return out

    def __iter__(self):
        if self.step >= self.steps_per_epoch:
            self.next_epoch()
        while self.step < self.steps_per_epoch:
            yield self.next_batch()
