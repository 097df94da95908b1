"""Host side of the epoch meter and of a feed's padded last batch: CacheFeed(pad_last=True)'s
step count, valid rows and device order; EpochMeter's refusals (more than 16 classes, CPU
tensors: there is no CPU path); and the key set of Base_Model.epoch_metrics against
_epoch_end's.  No device is touched."""
import types

import pytest
import torch

from multimodal_alzheimer_amd import _lib, device_cache as dc, metrics
from multimodal_alzheimer_amd.classifiers import Base_Model
from multimodal_alzheimer_amd.data_parallel import shard_indices


@pytest.mark.parametrize("n,b,world", [(7, 2, 1), (9, 4, 2), (8, 2, 1)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_pad_last_steps_valid_rows_and_order(n, b, world, shuffle):
    cache = types.SimpleNamespace(n=n)                 # the order needs the length only
    per = -(-n // world)
    steps = -(-per // b)
    for rank in range(world):
        feed = dc.CacheFeed(cache, b, rank=rank, world=world, shuffle=shuffle, seed=5,
                            drop_last=False, pad_last=True)
        assert feed.steps_per_epoch == len(feed) == steps
        assert feed.valid_rows == per
        assert feed.order_len == steps * b
        for epoch in (0, 3):
            real = shard_indices(n, rank, world, epoch, shuffle, 5)
            order = feed.padded_order(epoch)
            assert len(order) == steps * b
            assert order[:per] == real == feed.epoch_order(epoch)
            assert order[per:] == [real[-1]] * (steps * b - per)      # the tail repeats the last
            assert all(0 <= i < n for i in order)
            # the eager view is untouched: a short last batch
            batches = feed.epoch_batches(epoch)
            assert [len(x) for x in batches] == [b] * (per // b) + ([per % b] if per % b else [])
    if n == 8:
        assert feed.padded_order(0) == feed.epoch_order(0)            # no tail: nothing added


def test_pad_last_needs_drop_last_false():
    cache = types.SimpleNamespace(n=7)
    with pytest.raises(ValueError, match="drop_last=False"):
        dc.CacheFeed(cache, 2, pad_last=True)
    with pytest.raises(ValueError, match="drop_last=False"):
        dc.CacheFeed(cache, 2, drop_last=True, pad_last=True)


@pytest.mark.parametrize("drop_last", [True, False])
def test_feed_without_the_keyword_is_unchanged(drop_last):
    n, b = 7, 2
    cache = types.SimpleNamespace(n=n)
    feed = dc.CacheFeed(cache, b, shuffle=False, drop_last=drop_last)
    assert feed.pad_last is False
    assert len(feed) == (3 if drop_last else 4)
    assert feed.order_len == feed.per_rank == 7                      # the order is not padded
    assert feed.padded_order(0) == feed.epoch_order(0) == list(range(7))
    assert feed.valid_rows == (6 if drop_last else 7)
    if not drop_last:
        # a ragged epoch without padding still cannot be captured
        with pytest.raises(ValueError, match="full batches"):
            feed.fetch_into({})


def test_meter_refuses_too_many_classes():
    with pytest.raises(ValueError, match="16 classes"):
        metrics.EpochMeter(17)
    with pytest.raises(ValueError, match="16 classes"):
        metrics.EpochMeter(0)
    with pytest.raises(ValueError, match="keep_rows"):
        metrics.EpochMeter(3, keep_rows=-1)
    assert metrics.MAX_CLASSES == 16


def test_meter_refuses_cpu_tensors():
    with pytest.raises(_lib.MMADError, match="no CPU fallback"):
        metrics.EpochMeter(3, device="cpu")
    m = metrics.EpochMeter(3)                          # nothing is allocated before first use
    logits, labels = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.MMADError, match="no CPU fallback"):
        m.update(logits, labels, torch.zeros((), dtype=torch.float64))
    with pytest.raises(_lib.MMADError, match="no CPU fallback"):
        m.update(logits, labels)


def test_state_layout_constants():
    # the slots documented in include/mmad.h
    assert (metrics.SEEN, metrics.COUNTED, metrics.BATCHES, metrics.LIMIT, metrics.BAD_LABELS,
            metrics.OVERFLOW, metrics.LOSS_SUM, metrics.LOSS_LAST, metrics.CM) == tuple(range(9))
    assert metrics.COUNTER_NAMES == ("seen", "counted", "batches", "limit", "bad_labels",
                                     "overflow")


class _Tiny(Base_Model):
    def forward(self, x):
        return x

    def general_step(self, batch, batch_idx, mode):
        raise NotImplementedError

    def configure_optimizers(self):
        return None


@pytest.mark.parametrize("nc", [2, 3])
def test_epoch_metrics_keys_are_epoch_ends_plus_mcc(nc):
    model = _Tiny({"n_classes": nc})
    model.current_epoch = 4
    outputs = [{"loss": torch.tensor(0.5, dtype=torch.float64)},
               {"loss": torch.tensor(1.5, dtype=torch.float64)}]
    ref = model._epoch_end(outputs, "val")
    res = {"loss": torch.tensor(1.0, dtype=torch.float64),
           "f1": torch.tensor(0.25, dtype=torch.float64),
           "mcc": torch.tensor(-0.5, dtype=torch.float64),
           "accuracy": torch.tensor(0.5, dtype=torch.float64),
           "f1_per_class": torch.linspace(0, 1, nc, dtype=torch.float64)}
    got = model.epoch_metrics(res, "val")
    assert set(got) == set(ref) | {"val_mcc_epoch"}
    assert got["step"] == ref["step"] == 4.0
    assert got["val_loss_epoch"].dtype == ref["val_loss_epoch"].dtype == torch.float64
    assert float(got["val_loss_epoch"]) == float(ref["val_loss_epoch"]) == 1.0
    for k in ref:
        if "f1" in k:
            assert got[k].dtype == ref[k].dtype == torch.float32, k
            assert got[k].shape == ref[k].shape, k
    assert got["val_mcc_epoch"].dtype == torch.float32
    assert float(got[f"val_f1_epoch_class_{nc - 1}"]) == 1.0
    # a snapshot-like handle is unwrapped the same way
    handle = types.SimpleNamespace(result=lambda: res)
    assert set(model.epoch_metrics(handle, "test")) == {k.replace("val_", "test_") for k in got}
