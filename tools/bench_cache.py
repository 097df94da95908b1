"""Device-cache fetch timings (multimodal_alzheimer_amd.device_cache), sides interleaved.

    python tools/bench_cache.py [--batch 8] [--rounds 7] [--calls 200] [--skip-step]

One fetch of a batch of volumes out of a device-resident store into contiguous float64:

* flat: 128^3 scans, geometry unchanged;
* pad:  91 x 109 x 91 scans (the reference geometry) centre-padded to 96 x 112 x 96;

each from float32 and from float64 storage, ``mmad_cache_fetch`` against what a user would write
in torch today on the same store memory: ``store.index_select(0, idx).double()`` (and
``F.pad`` of that for the pad variant) -- two passes, or three.

The store is larger than the 256 MiB last-level cache and consecutive calls fetch different
batches (one shuffled pass over the store after another), so reads come from HBM.  Device events
around ``calls`` back-to-back launches; per round one figure per side, sides alternating; the
median over rounds is reported with bytes moved / time, where bytes moved = the stored bytes of
the batch read once + the float64 batch written once (the compulsory traffic of either side).

Then the step: ``GraphedTrainStep`` of the MRI-only ResNet-10 (bench.py's workload, batch 8 at
128^3, bf16) replaying on one resident batch, against the same step fed by a ``CacheFeed`` over 64
float32 scans (every replay fetches its own next batch inside the graph), in alternating blocks.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_alzheimer_amd import _lib as L, device_cache as dc  # noqa: E402

VARIANTS = {"flat_128": ((128, 128, 128), (128, 128, 128), 64),
            "pad_91x109x91_to_96x112x96": ((91, 109, 91), (96, 112, 96), 128)}


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls          # ms per call


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def one_variant(shape, out_shape, n, storage, b, rounds, calls):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((n,) + shape, dtype=torch.float32, device="cuda", generator=g).double()
    label = torch.zeros(n, dtype=torch.int64)
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x, storage=storage, out_shape=out_shape)
    del x
    vox = shape[0] * shape[1] * shape[2]
    kind, size, dtype = dc.STORAGE[storage]
    stride = dc.scan_stride_bytes(vox, storage)
    # the same store memory as a torch tensor (N, D, H, W); rows `stride` bytes apart
    store = cache._stores["mri"].view(dtype).view(n, stride // size)[:, :vox].view((n,) + shape)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(1)).cuda()
    nb = n // b
    cursors = [torch.tensor(k * b, dtype=torch.int64, device="cuda") for k in range(nb)]
    idxs = [order[k * b:(k + 1) * b].contiguous() for k in range(nb)]
    out = torch.empty((b,) + out_shape, dtype=torch.float64, device="cuda")
    pads = []
    for o, i in zip(reversed(out_shape), reversed(shape)):
        pads += [(o - i) // 2, (o - i) - (o - i) // 2]
    flat = shape == out_shape
    st = L.stream()

    def fetch(i):
        L.call("mmad_cache_fetch", kind, b, n, *shape, *out_shape, L.ptr(cache._stores["mri"]),
               L.ptr(order), L.ptr(cursors[i % nb]), n, L.ptr(out), L.ptr(cache._bad), st)

    def torch_form(i):
        y = store.index_select(0, idxs[i % nb]).double()
        return y if flat else F.pad(y, pads)

    # both sides give the same batch
    fetch(1)
    assert torch.equal(out, torch_form(1)), "fetch and the torch form disagree"
    sides = {"mmad_cache_fetch": fetch, "torch_index_select_double": torch_form}
    for fn in sides.values():
        timed(fn, 5)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, calls))
    assert not cache.bad_index_seen()
    res = {k: summary(v) for k, v in ms.items()}
    moved = b * vox * size + out.numel() * 8
    for k in res:
        res[k]["moved_GBps"] = round(moved / (res[k]["median_ms"] * 1e-3) / 1e9, 1)
    res["fetch_over_torch_time"] = round(res["mmad_cache_fetch"]["median_ms"]
                                         / res["torch_index_select_double"]["median_ms"], 3)
    return {"storage": storage, "scans": n, "store_MB": round(cache.store_bytes("mri") / 1e6, 1),
            "moved_MB": round(moved / 1e6, 2), "sides": res}


def step_times(b, s, n, rounds, steps, precision):
    import multimodal_alzheimer_amd as M
    from bench import hparams
    from multimodal_alzheimer_amd.graph_step import GraphedTrainStep
    g = torch.Generator(device="cuda").manual_seed(1000)
    x = torch.rand((n, s, s, s), device="cuda", dtype=torch.float32, generator=g).double()
    y = torch.randint(0, 2, (n,), device="cuda", generator=g).cpu()
    cache = dc.DeviceVolumeCache.from_tensors(y, mri=x, storage="float32")
    del x
    feed = cache.feed(b, shuffle=True)
    batch = feed.peek()
    sides = {}
    for name, fd in (("resident_batch", None), ("cache_feed", feed)):
        torch.manual_seed(15)
        m = M.Anat_CNN(hparams(precision)).cuda()
        sides[name] = GraphedTrainStep(m, m.configure_optimizers(), batch, warmup=3, feed=fd)
    for gs in sides.values():
        timed(lambda i: gs(), 5)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, gs in sides.items():
            ms[k].append(timed(lambda i: gs(), steps))
    assert not cache.bad_index_seen()
    out = {k: summary(v) for k, v in ms.items()}
    for k in out:
        out[k]["volumes_per_s"] = round(b / (out[k]["median_ms"] * 1e-3), 1)
    return {"workload": f"Anat_CNN ResNet-10, batch {b} x {s}^3, {precision}, graph replay; the "
                        f"feed draws from {n} float32 scans", "steps_per_round": steps,
            "rounds": rounds, "sides": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cache.py needs a HIP device: a time is only measured on one")
    res = {"batch": a.batch, "rounds": a.rounds, "calls": a.calls,
           "device": torch.cuda.get_device_name(0), "variants": {}}
    for name, (shape, out_shape, n) in VARIANTS.items():
        for storage in ("float32", "float64"):
            res["variants"][f"{name}_{storage}"] = one_variant(shape, out_shape, n, storage,
                                                               a.batch, a.rounds, a.calls)
            torch.cuda.empty_cache()
    if not a.skip_step:
        res["step"] = step_times(a.batch, 128, 64, a.rounds, a.steps, a.precision)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
