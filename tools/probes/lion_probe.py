"""Probe: the decode + update epilogue of SGD with momentum (wire.sgd), Lion (wire.lion) and AdamW (wire.adamw) on the
16.8 M-value flagship bucket (4096x4096+4096) and the 4.2 M-value one (1024x4096+4096), bfp_rne wire, bf16 copy
written, alternating in one process: warm-up, then 50 repetitions each, every launch timed with its own pair of events;
mean, min, spread (max - min) in us and TB/s of each kernel's own bytes. Per element SGD-momentum and Lion move 19.06
bytes (wire 1.0625, w 4+4, momentum 4+4, lp 2) and AdamW 27.06 (a second moment plane, 4+4): Lion should cost what
SGD-momentum costs. Prints one JSON line per bucket; `--out FILE` also writes them there.

`--mode steps`: the flagship MLP's training step through the forced multi-rank world-1 path under SGD-momentum, Lion and
AdamW, every trainer in a child process of its own (`--mode step --variant sgdm|lion|adamw`), `--rounds` children each,
alternating. (The unflagged step and bench.py against a built checkout of the parent commit: `tools/probes/sr_probe.py
--mode ab|bench --parent DIR`.)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402

BYTES = {"sgdm": 1.0625 + 4 * 4 + 2, "lion": 1.0625 + 4 * 4 + 2, "adamw": 1.0625 + 6 * 4 + 2}


def bucket(n, reps, warmup):
    assert n % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    buf = torch.empty(wire.shard_bytes("bfp_rne", n), dtype=torch.uint8, device="cuda")
    wire.pack(grad, buf, n, "bfp_rne")
    w = {k: torch.randn(n, device="cuda", generator=g) * 0.02 for k in BYTES}
    lp = {k: v.to(torch.bfloat16) for k, v in w.items()}
    m = {k: torch.zeros(n, device="cuda") for k in BYTES}
    v = torch.zeros(n, device="cuda")
    step = [0]
    ls = O.lion_scalars(1e-4, 1e-2, 0.9, 0.99)

    def sgdm():
        wire.sgd(buf, n, 1, w["sgdm"], codec="bfp_rne", lp=lp["sgdm"], mom=m["sgdm"], lr=1e-3, weight_decay=1e-2,
                 momentum=0.9)

    def lion():
        wire.lion(buf, n, 1, w["lion"], codec="bfp_rne", lp=lp["lion"], mom=m["lion"], scalars=ls)

    def adamw():
        step[0] += 1
        wire.adamw(buf, n, 1, w["adamw"], codec="bfp_rne", lp=lp["adamw"], mom=m["adamw"], var=v,
                   scalars=O.adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[0]))

    fns = {"sgdm": sgdm, "lion": lion, "adamw": adamw}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            us[k].append(s.elapsed_time(e) * 1e3)
    rec = {"probe": "lion", "elems": n, "codec": "bfp_rne", "reps": reps, "device": torch.cuda.get_device_name(0)}
    for k in fns:
        mean = statistics.mean(us[k])
        rec[f"{k}_mean_us"] = round(mean, 2)
        rec[f"{k}_min_us"] = round(min(us[k]), 2)
        rec[f"{k}_spread_us"] = round(max(us[k]) - min(us[k]), 2)
        rec[f"{k}_stdev_us"] = round(statistics.pstdev(us[k]), 2)
        rec[f"{k}_TBps"] = round(BYTES[k] * n / mean * 1e6 / 1e12, 3)
    rec["lion_over_sgdm"] = round(statistics.mean(us["lion"]) / statistics.mean(us["sgdm"]), 3)
    rec["adamw_over_sgdm"] = round(statistics.mean(us["adamw"]) / statistics.mean(us["sgdm"]), 3)
    rec["adamw_over_sgdm_from_bytes"] = round(BYTES["adamw"] / BYTES["sgdm"], 3)
    rec["state_bytes_per_param"] = {"sgdm": 4, "lion": 4, "adamw": 8}
    return rec


SIZES = [1024, 4096, 4096, 1024]


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


def step(a):
    """One trainer in this process: the flagship MLP's step through the forced multi-rank world-1 path (`force_comm`)
    under `a.variant` (sgdm | lion | adamw); every step timed with device events from its first launch to the landing
    of its last update."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
    from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
    from fpga_ai_nic_amd.parallel.transport import NativeTransport

    tp = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    eng = NativeAllReduce(tp, codec="bfp_rne", force_comm=True)
    model = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=1, adam=a.variant == "adamw",
                momentum=a.variant != "adamw", pad_fn=lambda n: eng.layout(n).n_pad)
    kw = {"sgdm": dict(lr=1e-3, weight_decay=1e-2, momentum=0.9),
          "lion": dict(lr=1e-4, weight_decay=1e-2, optimizer="lion"),
          "adamw": dict(lr=1e-3, weight_decay=1e-2, optimizer="adamw")}[a.variant]
    tr = DataParallelTrainer(model, eng, **kw)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(a.mb, SIZES[0], generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    y = torch.randint(0, SIZES[-1], (a.mb,), generator=g, dtype=torch.int32).cuda()

    def one():
        tr.step(x, y)
        tr.finish_async()

    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        one()
        e.record()
        e.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    tr.finish()
    return {"probe": "lion/step", "variant": a.variant, "mb": a.mb, "reps": a.reps,
            "mean_us": round(statistics.fmean(us), 2), "min_us": round(min(us), 2),
            "stdev_us": round(statistics.pstdev(us), 2), "prepack": bool(tr.prepack)}


def steps(a):
    """`--rounds` child processes per variant, alternating (several trainers in one process are not comparable)."""
    import subprocess

    me = os.path.abspath(__file__)
    out = {"sgdm": [], "lion": [], "adamw": []}
    for _ in range(a.rounds):
        for k in out:
            r = subprocess.run([sys.executable, me, "--mode", "step", "--variant", k, "--reps", str(a.reps), "--warmup",
                                str(a.warmup), "--mb", str(a.mb)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"child {k} failed ({r.returncode}): {r.stderr[-2000:]}")
            out[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"probe": "lion/steps", "rounds": a.rounds, "reps": a.reps, "mb": a.mb}
    for k, rs in out.items():
        means = [r["mean_us"] for r in rs]
        rec[f"{k}_child_means_us"] = means
        rec[f"{k}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{k}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{k}_min_us"] = min(r["min_us"] for r in rs)
    rec["lion_minus_sgdm_mean_us"] = round(rec["lion_mean_us"] - rec["sgdm_mean_us"], 2)
    rec["adamw_minus_sgdm_mean_us"] = round(rec["adamw_mean_us"] - rec["sgdm_mean_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step", "steps"], default="kernels")
    ap.add_argument("--variant", choices=["sgdm", "lion", "adamw"], default="lion")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mb", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "kernels":
        lines = [json.dumps(bucket(n, a.reps, a.warmup)) for n in (4096 * 4096 + 4096, 1024 * 4096 + 4096)]
    else:
        lines = [json.dumps(step(a) if a.mode == "step" else steps(a))]
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
