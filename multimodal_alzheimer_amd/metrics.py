"""Per-epoch metrics accumulated on the device (csrc/meter.hip).

The reference's epoch numbers -- ``{split}_loss_epoch``, ``{split}_f1_epoch`` and the per-class
F1 that ``Base_Model``'s ``*_epoch_end`` hooks log (pkg/models/base_model.py:91-149) and that
``EarlyStopping`` / ``ModelCheckpoint`` / ``ReduceLROnPlateau`` monitor -- come from
torchmetrics objects updated from Python on every step and from a Python list of every step's
outputs.  A captured step (``graph_step.GraphedTrainStep``) can feed neither: its outputs are
graph-owned buffers that the next replay overwrites, and a metric update that reads the device
cannot be captured.  :class:`EpochMeter` keeps the same numbers in one small device buffer:

* :meth:`EpochMeter.update` is one one-block launch (``mmad_meter_update``) that folds a step's
  logits, labels and loss into the buffer -- confusion matrix, counters, the running sum of the
  batch losses, optionally the rows themselves for the test-set bootstrap.  It reads no host
  value, so it is captured with the step and replays with it;
* a row limit set by :meth:`EpochMeter.reset` lives on the device: once ``limit`` rows have been
  offered the remaining rows of a batch are ignored, which is how the padded tail of a
  full-shape last batch (``device_cache.CacheFeed(pad_last=True)``) stays out of a validation
  score without the host saying which replay is the last;
* :meth:`EpochMeter.compute` (``mmad_meter_compute``) evaluates the buffer on the device,
  :meth:`EpochMeter.snapshot` also starts a non-blocking copy to pinned memory behind an event:
  epoch *e*'s numbers are read while epoch *e + 1* replays.

The definitions are those of ``mmad_bootstrap_cls_metrics`` (torchmetrics 0.10 macro F1 and
multiclass MCC); the epoch loss is the mean over batches, as ``torch.stack(losses).mean()``.
There is no CPU path: a CPU tensor raises.
"""
import torch

from . import _lib as L

MAX_CLASSES = 16
# eight-byte slots of the state (include/mmad.h, csrc/meter.hip)
SEEN, COUNTED, BATCHES, LIMIT, BAD_LABELS, OVERFLOW, LOSS_SUM, LOSS_LAST, CM = range(9)
COUNTER_NAMES = ("seen", "counted", "batches", "limit", "bad_labels", "overflow")
# slots of mmad_meter_compute's output
OUT_LOSS, OUT_F1, OUT_MCC, OUT_ACC, OUT_F1_CLASS = range(5)


def criterion_spec(criterion):
    """``criterion.fused_spec()`` -- (weight, gamma, mode) of the fused loss launch -- or None
    for a criterion that has none (or whose settings the launch does not cover)"""
    spec = getattr(criterion, "fused_spec", None)
    return spec() if spec is not None else None


def _named(out, n_classes):
    return {"loss": out[OUT_LOSS], "f1": out[OUT_F1], "mcc": out[OUT_MCC],
            "accuracy": out[OUT_ACC], "f1_per_class": out[OUT_F1_CLASS:OUT_F1_CLASS + n_classes]}


class MeterSnapshot:
    """An epoch's numbers on their way to the host (:meth:`EpochMeter.snapshot`)."""

    def __init__(self, n_classes, state, out, event):
        self.n_classes, self._state, self._out, self._event = n_classes, state, out, event

    def result(self):
        """Wait for this snapshot's copy -- its event only, not the device -- and return a dict
        of CPU tensors: ``loss`` (mean batch loss), ``f1``, ``mcc``, ``accuracy`` (0-d
        float64), ``f1_per_class`` (float64, one per class), ``confusion`` (int64, rows =
        target), ``loss_sum`` and the counters of the state as Python numbers."""
        self._event.synchronize()
        c = self.n_classes
        res = _named(self._out, c)
        res["confusion"] = self._state[CM:CM + c * c].reshape(c, c)
        res["loss_sum"] = float(self._state[LOSS_SUM:LOSS_SUM + 1].view(torch.float64))
        for i, name in enumerate(COUNTER_NAMES):
            res[name] = int(self._state[i])
        return res


class EpochMeter:
    """``EpochMeter(n_classes, criterion=None, keep_rows=0, device="cuda")``.

    ``criterion``: the model's loss (``Lyr.CrossEntropyLoss`` / ``FocalLoss``); its
    ``fused_spec()`` lets the update launch compute a batch's loss itself -- needed when
    :meth:`update` gets no loss (an evaluation forward) or when only a prefix of the batch
    counts (a padded tail).  ``keep_rows``: capacity of the row tables (f64 logits and labels of
    every counted row, in order) that :meth:`rows` hands to ``bootstrap_metric``; 0 keeps none.
    """

    def __init__(self, n_classes, criterion=None, keep_rows=0, device="cuda"):
        n_classes, keep_rows = int(n_classes), int(keep_rows)
        if not 1 <= n_classes <= MAX_CLASSES:
            raise ValueError(f"EpochMeter counts up to {MAX_CLASSES} classes, got {n_classes}")
        if keep_rows < 0:
            raise ValueError("keep_rows must not be negative")
        device = torch.device(device)
        if device.type != "cuda":
            raise L.MMADError("EpochMeter runs on HIP devices only (got device "
                              f"{device}) -- there is no CPU fallback")
        self.n_classes, self.keep_rows, self.device = n_classes, keep_rows, device
        self.spec = criterion_spec(criterion) if criterion is not None else None
        self._weight = None                  # the spec's class weights as f64 on the device
        self._limit = -1
        self._batch = None                   # the batch size of the last update
        self._landing = {}                   # batch size -> int64 landing buffer for labels
        self._state = self.rows_logits = self.rows_labels = None

    def prepare(self):
        """allocate the device state and the class weights (done by the first use; call it ahead
        of a capture)"""
        if self._state is None:
            c, dev = self.n_classes, self.device
            self._state = torch.zeros(CM + c * c, dtype=torch.int64, device=dev)
            self._state[LIMIT].fill_(self._limit)
            if self.keep_rows:
                self.rows_logits = torch.zeros((self.keep_rows, c), dtype=torch.float64,
                                               device=dev)
                self.rows_labels = torch.zeros(self.keep_rows, dtype=torch.int64, device=dev)
            if self.spec is not None and self.spec[0] is not None:
                if self.spec[0].numel() != c:
                    raise ValueError(f"the criterion weighs {self.spec[0].numel()} classes, the "
                                     f"meter counts {c}")
                self._weight = self.spec[0].detach().to(device=dev,
                                                        dtype=torch.float64).contiguous()
        return self

    @property
    def state(self):
        """the device state: int64 slots, layout in include/mmad.h"""
        return self.prepare()._state

    # ------------------------------------------------------------------------- launches
    def _check_tail(self, limit, batch):
        if self.spec is None and limit >= 0 and batch and limit % batch:
            raise ValueError(
                f"a limit of {limit} rows ends inside a batch of {batch}: the loss of that "
                "batch's counted rows has to be computed by the meter, which needs a criterion "
                "with a fused_spec()")

    def landing(self, batch, dtype):
        """the int64 landing buffer for a ``batch`` of labels of another dtype (made ahead of a
        capture by whoever captures :meth:`update`); None for int64 labels"""
        if dtype == torch.int64:
            return None
        if batch not in self._landing:
            self._landing[batch] = torch.empty(batch, dtype=torch.int64, device=self.device)
        return self._landing[batch]

    def update(self, logits, labels, loss=None):
        """Count one batch: ``logits`` (B, C) float32 / float64, ``labels`` (B,) of any integer
        dtype, ``loss`` the batch's loss as a float64 scalar tensor (None: the meter computes
        the criterion's).  One launch on the current stream; capturable."""
        L.require_device(logits, labels, loss)
        if logits.dim() != 2 or logits.shape[1] != self.n_classes or \
                logits.dtype not in (torch.float32, torch.float64):
            raise L.MMADError(f"EpochMeter.update expects (B, {self.n_classes}) fp32 / f64 "
                              f"logits, got {logits.dtype} {tuple(logits.shape)}")
        b = int(logits.shape[0])
        labels = labels.reshape(-1)
        if labels.numel() != b or labels.dtype.is_floating_point:
            raise L.MMADError(f"EpochMeter.update expects {b} integer labels")
        if loss is not None and (loss.numel() != 1 or loss.dtype != torch.float64):
            raise L.MMADError("EpochMeter.update expects the loss as one float64 value")
        if loss is None and self.spec is None:
            raise ValueError("EpochMeter.update without a loss computes the criterion itself: "
                             "build the meter with a criterion that has a fused_spec()")
        self._check_tail(self._limit, b)
        self._batch = b
        self.prepare()
        x = logits.detach().contiguous()
        y = labels.detach().contiguous()
        y64 = self.landing(b, y.dtype)
        if y64 is not None:
            y64.copy_(y)
            y = y64
        gamma, mode = (self.spec[1], self.spec[2]) if self.spec is not None else (0.0, -1)
        L.call("mmad_meter_update", b, self.n_classes, L.dtype_code(x.dtype), L.ptr(x), L.ptr(y),
               L.ptr(None if loss is None else loss.detach()), L.ptr(self._weight), float(gamma),
               int(mode), L.ptr(self.state), L.ptr(self.rows_logits), L.ptr(self.rows_labels),
               self.keep_rows, L.stream())

    def reset(self, limit=None):
        """Zero the state and set the row limit (None: count every row).  Stream-ordered, no
        synchronisation; the row tables are not cleared, ``counted`` says how much of them is
        valid."""
        limit = -1 if limit is None else int(limit)
        if limit < -1:
            raise ValueError("limit must be None or a row count")
        self._check_tail(limit, self._batch)
        self._limit = limit
        self.state.zero_()
        self.state[LIMIT].fill_(limit)

    def _compute(self):
        out = torch.empty(OUT_F1_CLASS + self.n_classes, dtype=torch.float64,
                          device=self.device)
        L.call("mmad_meter_compute", self.n_classes, L.ptr(self.state), L.ptr(out), L.stream())
        return out

    def compute(self):
        """the epoch's numbers as device tensors, no host read: ``loss``, ``f1``, ``mcc``,
        ``accuracy`` (0-d float64) and ``f1_per_class``"""
        return _named(self._compute(), self.n_classes)

    def snapshot(self):
        """:meth:`compute` plus a non-blocking copy of the state and the results into pinned
        memory, behind an event: returns a :class:`MeterSnapshot` at once.  The meter may be
        reset and updated again right away (the copy is stream-ordered in front of that)."""
        out = self._compute()
        host_state = torch.empty(self.state.shape, dtype=torch.int64, pin_memory=True)
        host_out = torch.empty(out.shape, dtype=torch.float64, pin_memory=True)
        host_state.copy_(self.state, non_blocking=True)
        host_out.copy_(out, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return MeterSnapshot(self.n_classes, host_state, host_out, event)

    # ---------------------------------------------------------------------------- views
    @property
    def confusion(self):
        """the confusion matrix (rows = target) as an int64 device view of the state"""
        c = self.n_classes
        return self.state[CM:CM + c * c].view(c, c)

    @property
    def loss_sum(self):
        return self.state[LOSS_SUM:LOSS_SUM + 1].view(torch.float64)[0]

    @property
    def loss_last(self):
        return self.state[LOSS_LAST:LOSS_LAST + 1].view(torch.float64)[0]

    def counters(self):
        """the counters as Python ints (one host sync)"""
        return dict(zip(COUNTER_NAMES, self.state[:len(COUNTER_NAMES)].tolist()))

    def rows(self):
        """``(y_hat[:counted], y[:counted])``: device views of the row tables, the concatenated
        f64 logits and labels of the epoch's counted rows in order -- what ``test_epoch_end``
        hands to ``bootstrap_metric``.  Reads ``counted`` (one host sync); raises when rows were
        dropped because ``keep_rows`` was too small."""
        if not self.keep_rows:
            raise ValueError("this meter keeps no rows: build it with keep_rows=<rows per epoch>")
        c = self.counters()
        if c["overflow"]:
            raise ValueError(f"{c['overflow']} of {c['counted']} rows did not fit keep_rows="
                             f"{self.keep_rows}")
        return self.rows_logits[:c["counted"]], self.rows_labels[:c["counted"]]

    # ------------------------------------------------------------------- data parallel
    def all_reduce(self, group=None):
        """Sum the matrix, the counters (all but ``limit``) and ``loss_sum`` over the ranks of
        ``group``: one small collective, once per epoch.  Afterwards :meth:`compute` gives the
        all-rank numbers, the loss as the mean over all ranks' batches.  The counts travel as
        float64 (exact below 2^53); the row tables stay local."""
        import torch.distributed as dist
        c2 = self.n_classes * self.n_classes
        ints = torch.cat([self.state[:LIMIT], self.state[BAD_LABELS:LOSS_SUM],
                          self.state[CM:CM + c2]])
        buf = torch.cat([ints.to(torch.float64), self.loss_sum.reshape(1)])
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
        ints = buf[:-1].to(torch.int64)
        self.state[:LIMIT].copy_(ints[:LIMIT])
        self.state[BAD_LABELS:LOSS_SUM].copy_(ints[LIMIT:LIMIT + 2])
        self.state[CM:CM + c2].copy_(ints[LIMIT + 2:])
        self.state[LOSS_SUM:LOSS_SUM + 1].copy_(buf[-1:].view(torch.int64))
