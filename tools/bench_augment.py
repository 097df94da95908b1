"""Device augmentation timings (multimodal_alzheimer_amd.augment), sides interleaved.

    python tools/bench_augment.py [--batch 8] [--size 128] [--rounds 5] [--skip-step]

1. Kernel: ``mmad_affine_resample3d`` on a batch of float64 volumes under a drawn
   +-10 degree / +-5 % / +-4 voxel transform (both paddings) and on its flip-only path, against
   ``mmad_affine_norm`` on the same tensor -- the project's float64 streaming kernel with the
   same compulsory traffic (8 B read + 8 B written per voxel) -- and
   ``mmad_deform_resample3d`` under the same transform plus a drawn 7^3 elastic lattice at half
   the fold guard's cap (both paddings), with its ratio to the affine resample.  Device events
   around ``calls`` back-to-back launches; per round one figure per side, sides alternating.
2. Step: ``GraphedTrainStep`` of the MRI-only ResNet-10 (bench.py's workload) without
   ``hparams['augment']``, with it, and with it plus the elastic deformation, replays timed in
   alternating blocks.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_alzheimer_amd as M  # noqa: E402
from multimodal_alzheimer_amd import augment, preprocess  # noqa: E402
from multimodal_alzheimer_amd.graph_step import GraphedTrainStep  # noqa: E402

AUG = {"flip_p": 0.5, "rotate_deg": 10.0, "scale": [0.95, 1.05], "translate_vox": 4.0,
       "gain": [0.9, 1.1], "bias": [-0.1, 0.1]}
ELASTIC_GRID = 7


def elastic(shape):
    """AUG plus a 7^3 lattice at half the largest admissible bound for this shape"""
    cfg = dict(AUG, elastic_grid=ELASTIC_GRID)
    return dict(cfg, elastic_vox=0.5 * augment.AugmentConfig(**cfg).elastic_cap(shape))


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


def kernel_times(b, s, rounds, calls):
    torch.manual_seed(0)
    x = torch.rand((b, s, s, s), dtype=torch.float64, device="cuda")
    spatial = {k: v for k, v in AUG.items() if k in ("rotate_deg", "scale", "translate_vox")}
    theta, _ = augment.draw(spatial, b, (s, s, s), "cuda")
    flip, _ = augment.draw({"flip_p": [0.0, 0.0, 1.0]}, b, (s, s, s), "cuda")
    ecfg = {k: v for k, v in elastic((s, s, s)).items() if k.startswith("elastic")}
    lattice = augment.draw(ecfg, b, (s, s, s), "cuda", return_lattice=True)[2]
    sides = {
        "affine_norm": lambda: preprocess.affine_normalize(x, 0.5, 0.25),
        "resample_zeros": lambda: augment.resample(x, theta, "zeros"),
        "resample_border": lambda: augment.resample(x, theta, "border"),
        "resample_flip_only": lambda: augment.resample(x, flip, "zeros"),
        "deform_zeros": lambda: augment.resample(x, theta, "zeros", lattice=lattice),
        "deform_border": lambda: augment.resample(x, theta, "border", lattice=lattice),
    }
    for fn in sides.values():                   # warm every side at this shape
        timed(fn, 3)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, calls))
    out = {k: summary(v) for k, v in ms.items()}
    nbytes = 2 * x.numel() * 8                  # compulsory: every voxel read once, written once
    for k in out:
        out[k]["compulsory_GBps"] = round(nbytes / (out[k]["median_ms"] * 1e-3) / 1e9, 1)
        out[k]["ratio_to_affine_norm"] = round(
            out[k]["median_ms"] / out["affine_norm"]["median_ms"], 3)
    for pad in ("zeros", "border"):
        out["deform_" + pad]["ratio_to_affine_resample"] = round(
            out["deform_" + pad]["median_ms"] / out["resample_" + pad]["median_ms"], 3)
    return {"shape": [b, s, s, s], "compulsory_MB": round(nbytes / 1e6, 1), "calls": calls,
            "rounds": rounds, "elastic_vox": round(ecfg["elastic_vox"], 3), "sides": out}


def step_times(b, s, rounds, steps, precision):
    from bench import hparams
    g = torch.Generator(device="cuda").manual_seed(1000)
    batch = {"mri": torch.rand((b, s, s, s), device="cuda", dtype=torch.float64, generator=g),
             "label": torch.randint(0, 2, (b,), device="cuda", generator=g)}
    sides = {}
    for name, extra in (("plain", {}), ("augment", {"augment": AUG}),
                        ("augment_elastic", {"augment": elastic((s, s, s))})):
        torch.manual_seed(15)
        m = M.Anat_CNN(dict(hparams(precision), **extra)).cuda()
        sides[name] = GraphedTrainStep(m, m.configure_optimizers(), batch, warmup=3)
    for gs in sides.values():
        timed(gs, 5)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, gs in sides.items():
            ms[k].append(timed(gs, steps))
    out = {k: summary(v) for k, v in ms.items()}
    for k in out:
        out[k]["volumes_per_s"] = round(b / (out[k]["median_ms"] * 1e-3), 1)
    return {"workload": f"Anat_CNN ResNet-10, batch {b} x {s}^3, {precision}, graph replay",
            "steps_per_round": steps, "rounds": rounds, "sides": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a HIP device: a time is only measured on one")
    res = {"kernel": kernel_times(a.batch, a.size, a.rounds, a.calls)}
    if not a.skip_step:
        res["step"] = step_times(a.batch, a.size, a.rounds, a.steps, a.precision)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
