"""What the epoch meter costs a captured training step (multimodal_alzheimer_amd.metrics).

    python tools/bench_meter.py [--batch 8] [--size 128] [--rounds 7] [--steps 32]

The workload is bench.py's (BASELINE config 2: Anat_CNN ResNet-10, MRI only, bf16, batch 8 at
128^3), built here.  Three ``GraphedTrainStep``s from the same seed replay on one resident batch:
two without a meter (``plain_a`` / ``plain_b``: the A/A pair, whose difference is the noise of
this measurement) and one with ``meter=EpochMeter(...)`` (one more one-block launch per replay).
The three sides alternate block by block in one process; device events around ``steps``
back-to-back replays, one figure per side and round, medians reported.

For scale, the eager Lightning-style path is timed too: ``model.training_step`` (``_step``: the
stand-in torchmetrics objects' update, with its ``.cpu()`` per step) + backward + Adam, launched
from Python.

``meter_cost_ms`` = with_meter - mean(plain_a, plain_b) medians; ``aa_spread_ms`` = |plain_a -
plain_b| medians.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_alzheimer_amd as M  # noqa: E402
from multimodal_alzheimer_amd import metrics  # noqa: E402
from multimodal_alzheimer_amd.graph_step import GraphedTrainStep  # noqa: E402


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls          # ms per call


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--eager-steps", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meter.py needs a HIP device: a time is only measured on one")
    from bench import hparams
    b, s = a.batch, a.size
    g = torch.Generator(device="cuda").manual_seed(1000)
    batch = {"mri": torch.rand((b, s, s, s), device="cuda", dtype=torch.float64, generator=g),
             "label": torch.randint(0, 2, (b,), device="cuda", generator=g)}

    def model():
        torch.manual_seed(15)
        return M.Anat_CNN(hparams(a.precision)).cuda()

    sides, meter = {}, None
    for name in ("plain_a", "with_meter", "plain_b"):
        m = model()
        mt = metrics.EpochMeter(2, criterion=m.criterion) if name == "with_meter" else None
        meter = mt or meter
        sides[name] = GraphedTrainStep(m, m.configure_optimizers(), batch, warmup=3, meter=mt)
    for gs in sides.values():
        timed(gs, 5)
    ms = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, gs in sides.items():
            ms[k].append(timed(gs, a.steps))
    counted = meter.counters()["counted"]
    assert counted == (5 + a.rounds * a.steps) * b, counted      # every replay was metered

    # the eager _step path: torchmetrics-style update (a .cpu() per step) + backward + Adam
    em = model()
    opt = em.configure_optimizers()

    def eager():
        opt.zero_grad(set_to_none=True)
        em.training_step(batch, 0)["loss"].backward()
        opt.step()

    timed(eager, 3)
    eager_ms = [timed(eager, a.eager_steps) for _ in range(max(3, a.rounds // 2))]

    out = {k: summary(v) for k, v in ms.items()}
    out["eager_step_with_cpu_metrics"] = summary(eager_ms)
    for k in out:
        out[k]["volumes_per_s"] = round(b / (out[k]["median_ms"] * 1e-3), 1)
    pa, pb, wm = (out[k]["median_ms"] for k in ("plain_a", "plain_b", "with_meter"))
    res = {"workload": f"Anat_CNN ResNet-10, batch {b} x {s}^3, {a.precision}, graph replay on a "
                       "resident batch", "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "steps_per_round": a.steps, "sides": out,
           "meter_cost_ms": round(wm - (pa + pb) / 2, 4), "aa_spread_ms": round(abs(pa - pb), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
