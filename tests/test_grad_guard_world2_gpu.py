"""The gradient guard under data parallelism at world size 2 (GraphedTrainStep(reducer=...,
collectives="after", skip_nonfinite=True)): one rank's backward overflows on one replay, the
all-reduce carries the non-finite gradients to both ranks, and both skip that step together with
no collective of the guard's own -- their guard states and parameters stay bitwise equal.

Two processes share the test box's one GPU, as in tests/test_dp_graph_world2_gpu.py (RCCL
refuses two ranks on one device, so the collective is gloo over the same CUDA tensors).
Anat_CNN ResNet-10, bf16, 32^3, two scans per rank, a different batch on every rank."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
STEPS, WARM, BAD_STEP = 3, 1, 1


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist

    import multimodal_alzheimer_amd as M
    from multimodal_alzheimer_amd.data_parallel import GradAllReduce
    from multimodal_alzheimer_amd.graph_step import GraphedTrainStep
    from tests.test_adam_repack_gpu import _batch, _hparams
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        # the same weights on both ranks; an initialisation from which the model's closing
        # ReLU stays alive (tests/test_grad_guard_gpu.py, twin())
        torch.manual_seed(13)
        m = M.Anat_CNN(_hparams()).cuda()
        batches = [_batch(30 + rank + i) for i in range(STEPS)]
        opt = m.configure_optimizers()
        red = GradAllReduce(m.parameters(), bucket_mb=4.0)
        gs = GraphedTrainStep(m, opt, batches[0], warmup=WARM, reducer=red,
                              collectives="after", skip_nonfinite=True)
        skips = []
        for i in range(STEPS):
            if i == BAD_STEP:
                torch.cuda.synchronize()
                held = [p.detach().clone() for p in m.parameters()]
                if rank == 1:
                    gs._one.fill_(float("inf"))       # this rank's backward overflows
            gs(batches[i])
            if i == BAD_STEP:
                gs._one.fill_(1.0)
                torch.cuda.synchronize()
                unchanged = all(torch.equal(p, h) for p, h in zip(m.parameters(), held))
            skips.append(gs.guard.stats()["skip"])
        torch.cuda.synchronize()
        moved = any(not torch.equal(p, h) for p, h in zip(m.parameters(), held))
        torch.save({"state": gs.guard.state.cpu(), "skips": skips, "unchanged": unchanged,
                    "moved": moved, "stats": gs.guard.stats(),
                    "params": {k: p.detach().cpu() for k, p in m.named_parameters()},
                    "batch0": batches[0]["mri"].cpu()},
                   os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_both_ranks_skip_the_step_one_of_them_overflowed(tmp_path):
    ctx = mp.get_context("spawn")
    port = 31100 + os.getpid() % 400
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=150)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    res = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(2)]
    assert not torch.equal(res[0]["batch0"], res[1]["batch0"]), "shards identical"
    for r in range(2):
        assert res[r]["skips"] == [int(i == BAD_STEP) for i in range(STEPS)], (r, res[r]["skips"])
        assert res[r]["unchanged"], r                 # the bad replay left the weights alone
        assert res[r]["moved"], r                     # the replay after it trained again
        assert res[r]["stats"]["skipped"] == 1 and res[r]["stats"]["steps"] == WARM + STEPS
    assert torch.equal(res[0]["state"].view(torch.int64), res[1]["state"].view(torch.int64))
    for k in res[0]["params"]:
        assert torch.equal(res[0]["params"][k], res[1]["params"][k]), k
