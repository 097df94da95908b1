"""EpochMeter.all_reduce at world size 2: each rank meters its own shard of an epoch, one small
collective sums the matrices, the counters and the loss sums, and both ranks then hold the
numbers of one meter fed both shards.

Two processes share the test box's one GPU, as in tests/test_grad_guard_world2_gpu.py (RCCL
refuses two ranks on one device, so the collective is gloo over the same CUDA tensors)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
C, B, STEPS = 3, 5, 3


def _shard(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return [(torch.randn((B, C), generator=g), torch.randint(0, C, (B,), generator=g))
            for _ in range(STEPS)]


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist

    from multimodal_alzheimer_amd import metrics
    from multimodal_alzheimer_amd.layers import CrossEntropyLoss
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        crit = CrossEntropyLoss(weight=torch.tensor([0.5, 0.2, 0.3], dtype=torch.float64))
        # a rank's last batch is cut short by its limit: 2 full batches and 3 (rank 0) or 4
        # (rank 1) rows of the third
        shards = []
        for r in range(world):
            m = metrics.EpochMeter(C, criterion=crit)
            m.reset(2 * B + 3 + r)
            for x, y in _shard(r):
                m.update(x.cuda(), y.cuda())
            shards.append(m)
        mine = shards[rank]
        local, first, second = mine.state.clone(), shards[0].state.clone(), shards[1].state.clone()
        # one meter fed the counted rows of both shards
        both = metrics.EpochMeter(C, criterion=crit)
        for r in range(world):
            for k, (x, y) in enumerate(_shard(r)):
                v = B if k < 2 else 3 + r
                both.update(x[:v].cuda(), y[:v].cuda())
        one = both.compute()
        mine.all_reduce()
        res = mine.compute()
        torch.cuda.synchronize()
        torch.save({"local": local.cpu(), "reduced": mine.state.cpu(), "shard0": first.cpu(),
                    "shard1": second.cpu(), "both": both.state.cpu(),
                    "one": torch.cat([one[k].reshape(-1) for k in
                                      ("loss", "f1", "mcc", "accuracy", "f1_per_class")]).cpu(),
                    "out": torch.cat([res["loss"].reshape(1), res["f1"].reshape(1),
                                      res["mcc"].reshape(1), res["accuracy"].reshape(1),
                                      res["f1_per_class"]]).cpu()},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_all_reduce_gives_both_ranks_the_epoch_of_both_shards(tmp_path):
    from multimodal_alzheimer_amd import metrics as mt
    ctx = mp.get_context("spawn")
    port = 31600 + os.getpid() % 400
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=150)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    res = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2)]
    s0, s1 = res[0]["shard0"], res[0]["shard1"]
    assert torch.equal(res[0]["local"], s0) and torch.equal(res[1]["local"], s1)
    assert not torch.equal(s0[mt.CM:], s1[mt.CM:]), "shards identical"
    ints = [i for i in range(len(s0)) if i not in (mt.LIMIT, mt.LOSS_SUM, mt.LOSS_LAST)]
    f64 = lambda s, i: float(s[i:i + 1].view(torch.float64))       # noqa: E731
    for r in range(2):
        red = res[r]["reduced"]
        assert torch.equal(red[ints], s0[ints] + s1[ints]), r      # matrix and counters: sums
        assert int(red[mt.COUNTED]) == (2 * B + 3) + (2 * B + 4) and int(red[mt.BATCHES]) == 6
        assert int(red[mt.LIMIT]) == 2 * B + 3 + r                 # the limit stays the rank's
        assert f64(red, mt.LOSS_SUM) == f64(s0, mt.LOSS_SUM) + f64(s1, mt.LOSS_SUM)
    assert torch.equal(res[0]["reduced"][ints], res[1]["reduced"][ints])
    assert torch.equal(res[0]["out"].view(torch.int64), res[1]["out"].view(torch.int64))
    # the same epoch numbers as one meter fed both shards: the mean over all six batches
    out = res[0]["out"]
    assert torch.equal(res[0]["reduced"][mt.CM:], res[0]["both"][mt.CM:])
    assert int(res[0]["both"][mt.BATCHES]) == 6
    assert (out - res[0]["one"]).abs().max() <= 1e-12
    want_loss = (f64(s0, mt.LOSS_SUM) + f64(s1, mt.LOSS_SUM)) / 6
    assert abs(float(out[mt.OUT_LOSS]) - want_loss) <= 1e-12
    import numpy as np

    from oracle import metrics_ref
    cm = (s0[mt.CM:] + s1[mt.CM:]).reshape(C, C).numpy()
    assert abs(float(out[mt.OUT_F1]) - metrics_ref.macro_f1(cm)) <= 1e-12
    assert abs(float(out[mt.OUT_MCC]) - metrics_ref.mcc(cm)) <= 1e-12
    assert abs(float(out[mt.OUT_ACC]) - float(np.trace(cm)) / float(cm.sum())) <= 1e-12
