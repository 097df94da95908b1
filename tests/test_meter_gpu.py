"""The epoch meter on the device (csrc/meter.hip, metrics.EpochMeter) and the two captured loops
built on it (graph_step.GraphedTrainStep(meter=...), graph_step.GraphedEvalEpoch).

The kernel is checked against the CPU: oracle.metrics_ref.confusion / macro_f1 / mcc (pinned
by scikit-learn) for the matrix and the scores, head_ops.logits_and_loss for each batch loss.
The matrix, the counters, every batch loss and the loss sum are compared exactly (bits); the
f64 scores within 1e-12, the project's f64 bar for the losses.  Models are Anat_CNN ResNet-10 at
32^3, two scans per batch."""
import copy

import numpy as np
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import device_cache as dc
from multimodal_alzheimer_amd import head_ops, metrics
from multimodal_alzheimer_amd.classifiers import FocalLoss
from multimodal_alzheimer_amd.graph_step import GraphedEvalEpoch, GraphedTrainStep
from multimodal_alzheimer_amd.layers import CrossEntropyLoss
from multimodal_alzheimer_amd.lightning_compat import (MulticlassF1Score,
                                                       MulticlassMatthewsCorrCoef)
from oracle import metrics_ref
from tests import _poison as P
from tests.test_adam_repack_gpu import _hparams

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-12
N_UPDATES = 4


def _bits(t):
    return t.detach().reshape(-1).cpu().contiguous().view(torch.int64)


def _criteria(c):
    w = torch.linspace(0.3, 1.7, c, dtype=torch.float64)
    return [CrossEntropyLoss(weight=w), FocalLoss(gamma=0), FocalLoss(gamma=2),
            FocalLoss(gamma=2.5)]


def _batches(b, c, dtype, scenario, seed):
    """N_UPDATES batches of (logits, labels).  Row 0 of every batch is an exact tie between its
    first two classes; batch 1 holds a label of -1 and batch 2 a label of C (row b - 1, b > 1).
    'absent': the last class is never a label and never a prediction, so macro F1 leaves it out
    -- at C = 2 everything is class 0 and MCC is 0.  'mixed': every class occurs."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(N_UPDATES):
        x = torch.randn((b, c), generator=g, dtype=torch.float64).to(dtype)
        hi = c - 1 if scenario == "absent" else c
        y = torch.randint(0, hi, (b,), generator=g)
        if scenario == "absent":
            x[:, c - 1] = -50.0
        x[0, 0] = x[0, 1] = 3.0                      # the tie: the first index wins
        if k == 1 and b > 1:                         # (alone in a batch it would make the
            y[b - 1] = -1                            # batch loss 0 / 0, as loss_kernel does)
        if k == 2 and b > 1:
            y[b - 1] = c
        out.append((x.to(DEV), y.to(DEV)))
    return out


def _ref_loss(x, y, spec):
    return head_ops.logits_and_loss(x, y, *spec)[1].detach()


def _scores(cm):
    """(macro F1, MCC, accuracy, per-class F1) of a confusion matrix in numpy f64"""
    tp = np.diag(cm).astype(np.float64)
    den = 2 * tp + (cm.sum(0) - tp) + (cm.sum(1) - tp)
    per = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    acc = float(np.trace(cm)) / float(cm.sum()) if cm.sum() else 0.0
    return metrics_ref.macro_f1(cm), metrics_ref.mcc(cm), acc, per


class _Host:
    """the meter's bookkeeping restated on the host"""

    def __init__(self, c, limit, cap):
        self.c, self.limit, self.cap = c, limit, cap
        self.seen = self.counted = self.batches = self.bad = self.over = 0
        self.cm = np.zeros((c, c), dtype=np.int64)
        self.losses, self.rows_x, self.rows_y = [], [], []

    def valid(self, b):
        return b if self.limit is None else max(0, min(b, self.limit - self.seen))

    def add(self, x, y, loss):
        b = len(y)
        v = self.valid(b)
        self.seen += b
        if v == 0:
            return
        xv, yv = x[:v].double().cpu(), y[:v].cpu()
        pred = torch.argmax(xv, dim=1)
        ok = (yv >= 0) & (yv < self.c)
        self.cm += metrics_ref.confusion(pred[ok].numpy(), yv[ok].numpy(), self.c)
        self.bad += int((~ok).sum())
        room = max(0, self.cap - self.counted)
        self.over += max(0, v - room) if self.cap else 0
        self.rows_x.append(xv[:room])
        self.rows_y.append(yv[:room])
        self.counted += v
        self.batches += 1
        self.losses.append(loss)

    def loss_sum(self):
        s = torch.zeros((), dtype=torch.float64)
        for v in self.losses:
            s = s + v.cpu()
        return s

    def check(self, meter):
        got = meter.counters()
        want = {"seen": self.seen, "counted": self.counted, "batches": self.batches,
                "limit": -1 if self.limit is None else self.limit, "bad_labels": self.bad,
                "overflow": self.over}
        assert got == want
        assert np.array_equal(meter.confusion.cpu().numpy(), self.cm)
        assert torch.equal(_bits(meter.loss_sum), _bits(self.loss_sum()))
        res = meter.compute()
        f1, mcc, acc, per = _scores(self.cm)
        if self.batches:
            assert abs(float(res["loss"]) - float(self.loss_sum()) / self.batches) <= TOL
        else:
            assert torch.isnan(res["loss"])
        assert abs(float(res["f1"]) - f1) <= TOL
        assert abs(float(res["mcc"]) - mcc) <= TOL
        assert abs(float(res["accuracy"]) - acc) <= TOL
        assert np.abs(res["f1_per_class"].cpu().numpy() - per).max() <= TOL
        return res


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("b", [1, 2, 5, 64, 300])
@pytest.mark.parametrize("c", [2, 3, 16])
def test_update_and_compute_against_the_cpu(c, b, dtype):
    # limits under which `valid` takes B, B - 1, 1 and 0 (None: every row counts)
    limits = [2 * b + (b - 1), b + 1, None]
    for ci, crit in enumerate(_criteria(c)):
        scenario = "absent" if ci % 2 else "mixed"
        data = _batches(b, c, dtype, scenario, seed=100 * c + b + ci)
        cap = N_UPDATES * b
        meter = metrics.EpochMeter(c, criterion=crit, keep_rows=cap)
        spec = metrics.criterion_spec(crit)
        spec = (None if spec[0] is None else spec[0].to(DEV), spec[1], spec[2])
        seen_valid = set()
        for limit in limits:
            meter.reset(limit)
            host = _Host(c, limit, cap)
            for k, (x, y) in enumerate(data):
                v = host.valid(b)
                seen_valid.add(v)
                # the first two batches hand their loss in, as a captured train step does: a
                # full batch takes it as it is, a cut one (batch 1 under the second limit)
                # computes its own
                given = _ref_loss(x, y, spec) if k < 2 else None
                meter.update(x, y, given)
                if v:
                    want = given if (given is not None and v == b) else \
                        _ref_loss(x[:v], y[:v], spec)
                    assert torch.equal(_bits(meter.loss_last), _bits(want)), (limit, k, v)
                host.add(x, y, want if v else None)
            res = host.check(meter)
            if scenario == "absent":
                assert float(res["f1_per_class"][c - 1]) == 0.0      # absent: left out of the mean
                if c == 2:
                    assert float(res["mcc"]) == 0.0 and float(res["accuracy"]) == 1.0
            # the row tables: every counted row, in order, widened exactly
            rx, ry = meter.rows()
            assert torch.equal(_bits(rx), _bits(torch.cat(host.rows_x)))
            assert torch.equal(ry.cpu(), torch.cat(host.rows_y))
        assert seen_valid >= {0, 1, b - 1, b}


@pytest.mark.parametrize("c", [2, 3, 16])
def test_nan_row_wins_the_argmax_and_ties_take_the_first(c):
    b = 5
    x = torch.zeros((b, c), dtype=torch.float64)
    x[0, :] = 1.0                                    # all tied: class 0
    x[1, c - 1] = float("nan")                       # a NaN wins
    x[2, 0] = float("nan")
    x[2, c - 1] = float("nan")                       # the first NaN wins
    x[3, c - 1] = 2.0
    x[3, c // 2] = 2.0                               # tied maxima: the lower index
    x[4, 0] = -1.0
    y = torch.tensor([0, c - 1, 0, c // 2, 1 % c])
    crit = CrossEntropyLoss()
    meter = metrics.EpochMeter(c, criterion=crit)
    meter.update(x.to(DEV), y.to(DEV))
    pred = torch.argmax(x, dim=1)
    assert pred.tolist()[:4] == [0, c - 1, 0, c // 2]
    assert np.array_equal(meter.confusion.cpu().numpy(),
                          metrics_ref.confusion(pred.numpy(), y.numpy(), c))
    want = _ref_loss(x.to(DEV), y.to(DEV), metrics.criterion_spec(crit))
    assert torch.isnan(want) and torch.equal(_bits(meter.loss_last), _bits(want))
    assert meter.counters()["counted"] == b


def test_row_tables_overflow_is_counted():
    c, b, cap = 3, 5, 7
    data = _batches(b, c, torch.float32, "mixed", seed=7)
    meter = metrics.EpochMeter(c, criterion=CrossEntropyLoss(), keep_rows=cap)
    host = _Host(c, None, cap)
    for x, y in data:
        meter.update(x, y)
        host.add(x, y, None)
    cnt = meter.counters()
    assert cnt["counted"] == N_UPDATES * b and cnt["overflow"] == N_UPDATES * b - cap
    assert cnt["overflow"] == host.over
    assert torch.equal(_bits(meter.rows_logits), _bits(torch.cat(host.rows_x)))
    assert torch.equal(meter.rows_labels.cpu(), torch.cat(host.rows_y))
    with pytest.raises(ValueError, match="did not fit"):
        meter.rows()


def test_refusals():
    m = metrics.EpochMeter(3)
    x, y = torch.zeros((4, 3), device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="fused_spec"):
        m.update(x, y)                               # no loss and no criterion
    m.update(x, y, torch.zeros((), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="ends inside a batch"):
        m.reset(limit=6)                             # a cut batch needs the criterion
    m.reset(limit=8)
    with pytest.raises(L.MMADError):
        m.update(torch.zeros((4, 2), device=DEV), y)
    lib = L.load()
    st = m.state
    assert lib.mmad_meter_update(4, 17, L.F32, x.data_ptr(), y.data_ptr(), None, None, 0.0, 0,
                                 st.data_ptr(), None, None, 0, None) == 1001
    assert lib.mmad_meter_update(4, 3, L.F32, None, y.data_ptr(), None, None, 0.0, 0,
                                 st.data_ptr(), None, None, 0, None) == 1003
    assert lib.mmad_meter_update(4, 3, L.F32, x.data_ptr(), y.data_ptr() + 4, None, None, 0.0, 0,
                                 st.data_ptr(), None, None, 0, None) == 1001
    assert lib.mmad_meter_compute(17, st.data_ptr(), x.data_ptr(), None) == 1001
    assert lib.mmad_meter_compute(3, None, x.data_ptr(), None) == 1003
    torch.cuda.synchronize()
    assert m.counters()["seen"] == 0                 # nothing was launched by the refused calls


def test_poisoned_allocations_give_the_same_state():
    """update / compute with every torch.empty buffer (the label landing buffer, compute's
    output) pre-filled with NaN, then with zeros, and the operands between NaN margins: the
    same state and result bits, and no margin byte changed."""
    c, b = 3, 5
    data = _batches(b, c, torch.float32, "mixed", seed=11)
    crit = CrossEntropyLoss(weight=torch.tensor([0.2, 0.3, 0.5], dtype=torch.float64))

    def run():
        meter = metrics.EpochMeter(c, criterion=crit, keep_rows=N_UPDATES * b)
        meter.reset(limit=3 * b + 2)
        for x, y in data:
            meter.update(P.guarded(x), P.guarded(y.to(torch.int32)))    # int32: landing buffer
        out = meter.compute()
        torch.cuda.synchronize()
        return {"state": meter.state.clone(), "rows": meter.rows_logits.clone(),
                "out": torch.cat([out["loss"].reshape(1), out["f1"].reshape(1),
                                  out["mcc"].reshape(1), out["accuracy"].reshape(1),
                                  out["f1_per_class"]])}

    plain = run()
    assert torch.isfinite(plain["out"]).all()
    for fill in ("A", "B"):
        with P.poisoned(fill) as p:
            got = run()
            assert p.records, "nothing was allocated through torch.empty"
            p.check()
        for k in plain:
            assert torch.equal(_bits(plain[k]), _bits(got[k])), (fill, k)


# ---------------------------------------------------------------------- captured loops
def _cache(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 32, 32, 32), dtype=torch.float64, generator=g)
    y = torch.randint(0, 2, (n,), generator=g)
    return dc.DeviceVolumeCache.from_tensors(y, mri=x)


def test_captured_train_step_updates_the_meter():
    n, bs, warm = 9, 2, 2
    cache = _cache(n, 9)
    torch.manual_seed(3)
    a = M.Anat_CNN(_hparams()).cuda()
    b = copy.deepcopy(a)
    meter = metrics.EpochMeter(2, criterion=a.criterion)
    gs = GraphedTrainStep(a, a.configure_optimizers(), warmup=warm,
                          feed=cache.feed(bs, shuffle=True, seed=4), meter=meter)
    cnt = meter.counters()
    assert cnt["counted"] == 0 and cnt["seen"] == 0 and cnt["batches"] == 0   # warm-up uncounted
    twin = GraphedTrainStep(b, b.configure_optimizers(), warmup=warm,
                            feed=cache.feed(bs, shuffle=True, seed=4))
    assert len(gs.feed) == 4
    losses, outs, labels = [], [], []
    for _ in range(4):
        out = gs()
        losses.append(out["loss"].clone())
        outs.append(out["outputs"].clone())
        labels.append(out["labels"].clone())
        twin()
    torch.cuda.synchronize()
    total = torch.zeros((), dtype=torch.float64)
    for v in losses:
        total = total + v.cpu()
    assert torch.equal(_bits(meter.loss_sum), _bits(total))
    pred = torch.argmax(torch.cat(outs).cpu(), dim=1).numpy()
    want = metrics_ref.confusion(pred, torch.cat(labels).cpu().numpy(), 2)
    assert np.array_equal(meter.confusion.cpu().numpy(), want)
    cnt = meter.counters()
    assert (cnt["counted"], cnt["seen"], cnt["batches"], cnt["bad_labels"]) == (8, 8, 4, 0)
    res = a.epoch_metrics(meter, "train")
    assert abs(float(res["train_loss_epoch"]) - float(total) / 4) <= TOL
    assert abs(float(res["train_f1_epoch"]) - np.float32(metrics_ref.macro_f1(want))) <= 1e-7
    # the meter changes nothing of the training itself
    for (na, pa), (nb, pb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert na == nb and torch.equal(pa, pb), na


def _val_model(seed):
    torch.manual_seed(seed)
    return M.Anat_CNN(_hparams()).cuda().eval()


def test_captured_validation_epoch_counts_the_short_tail():
    n, bs = 7, 2
    cache = _cache(n, 21)
    model = _val_model(5)
    meter = metrics.EpochMeter(2, criterion=model.criterion, keep_rows=n)
    feed = cache.feed(bs, shuffle=False, drop_last=False, pad_last=True)
    assert len(feed) == 4 and feed.valid_rows == 7
    ev = GraphedEvalEpoch(model, feed, meter)
    snap = ev.run()
    first = snap.result()
    state1, rows1 = meter.state.clone(), meter.rows_logits.clone()
    assert first["counted"] == 7 and first["seen"] == 8 and first["batches"] == 4
    assert first["bad_labels"] == 0 and first["overflow"] == 0
    assert not cache.bad_index_seen()

    # the same padded batches, eagerly, scored on the host over the valid prefix only
    spec = metrics.criterion_spec(model.criterion)
    order = feed.padded_order(0)
    assert order == [0, 1, 2, 3, 4, 5, 6, 6]
    cm = np.zeros((2, 2), dtype=np.int64)
    total = torch.zeros((), dtype=torch.float64)
    xs, ys = [], []
    with torch.no_grad():
        for s in range(4):
            batch = cache.fetch(order[s * bs:(s + 1) * bs])
            out = model.general_step(batch, 0, "pred")
            v = min(bs, n - s * bs)
            x, y = out["outputs"][:v], out["labels"][:v]
            loss = out["loss"] if v == bs else _ref_loss(x, y, spec)
            total = total + loss.cpu()
            cm += metrics_ref.confusion(torch.argmax(x.cpu(), dim=1).numpy(), y.cpu().numpy(), 2)
            xs.append(x.clone())
            ys.append(y.clone())
    assert np.array_equal(first["confusion"].numpy(), cm)
    assert first["loss_sum"] == float(total)
    assert torch.equal(_bits(meter.loss_sum), _bits(total))

    # snapshot().result() is compute()
    now = meter.compute()
    for k in ("loss", "f1", "mcc", "accuracy", "f1_per_class"):
        assert torch.equal(_bits(first[k]), _bits(now[k])), k
    f1, mcc, acc, per = _scores(cm)
    assert abs(float(first["loss"]) - float(total) / 4) <= TOL
    assert abs(float(first["f1"]) - f1) <= TOL and abs(float(first["mcc"]) - mcc) <= TOL
    assert abs(float(first["accuracy"]) - acc) <= TOL

    # a second run: the same bits
    ev.run().result()
    assert torch.equal(meter.state, state1) and torch.equal(_bits(meter.rows_logits), _bits(rows1))

    # the rows the meter kept are the host-collected rows; so is their bootstrap
    y_hat, y = torch.cat(xs), torch.cat(ys)
    rx, ry = meter.rows()
    assert torch.equal(_bits(rx), _bits(y_hat)) and torch.equal(ry, y)
    torch.manual_seed(1)
    got = model.test_metrics(meter)
    torch.manual_seed(1)
    f1_boot = model.bootstrap_metric(MulticlassF1Score(num_classes=2, average="macro"), y_hat, y)
    mcc_boot = model.bootstrap_metric(MulticlassMatthewsCorrCoef(num_classes=2), y_hat, y)
    assert torch.equal(got["test_f1_epoch_boot"], f1_boot[0])
    assert torch.equal(got["test_f1_epoch_ci"], f1_boot[1])
    assert torch.equal(got["test_mcc_epoch_boot"], mcc_boot[0])
    assert torch.equal(got["test_mcc_epoch_ci"], mcc_boot[1])
    assert float(got["test_loss_epoch"]) == float(first["loss"])
    assert abs(float(got["test_mcc_epoch"]) - np.float32(mcc)) <= 1e-7


def test_validation_epoch_needs_a_fused_criterion_for_the_tail():
    cache = _cache(7, 22)
    model = _val_model(6)
    feed = cache.feed(2, shuffle=False, drop_last=False, pad_last=True)
    meter = metrics.EpochMeter(2, criterion=torch.nn.CrossEntropyLoss())
    with pytest.raises(ValueError, match="fused_spec"):
        GraphedEvalEpoch(model, feed, meter)
