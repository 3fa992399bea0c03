"""Probe: the AdamW decode + update epilogue with f32 moment planes (wire.adamw) against 8-bit planes (wire.adamw_q) on
the 16.8 M-value flagship bucket (4096x4096+4096) and the 4.2 M-value one (1024x4096+4096), bfp_rne wire, bf16 copy
written, alternating in one process: warm-up, then 50 repetitions each, every launch timed with its own pair of events;
mean, min, spread (max - min) in us and TB/s of each kernel's own bytes. Per element wire.adamw moves 27.06 bytes (wire
1.0625, w 4+4, both moments 4+4 each, lp 2) and wire.adamw_q 15.31 (both planes 1.0625+1.0625 each): the byte count
predicts 1.77x. Prints one JSON line per bucket; `--out FILE` also writes them there.

`--mode steps`: the flagship MLP's AdamW training step through the forced multi-rank world-1 path, f32 against bfp8
state, every trainer in a child process of its own (`--mode step --variant f32|bfp8`), `--rounds` children each,
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

BYTES = {"adamw_f32": 1.0625 + 6 * 4 + 2, "adamw_bfp8": 1.0625 + 2 * 4 + 2 + 4 * 1.0625}


def bucket(n, reps, warmup):
    assert n % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    buf = torch.empty(wire.shard_bytes("bfp_rne", n), dtype=torch.uint8, device="cuda")
    wire.pack(grad, buf, n, "bfp_rne")
    w = {k: torch.randn(n, device="cuda", generator=g) * 0.02 for k in BYTES}
    lp = {k: v.to(torch.bfloat16) for k, v in w.items()}
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    mq, vq = wire.moment_plane(n, "cuda"), wire.moment_plane(n, "cuda")
    step = {k: 0 for k in BYTES}

    def scalars(k):
        step[k] += 1
        return O.adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[k])

    def f32():
        wire.adamw(buf, n, 1, w["adamw_f32"], codec="bfp_rne", lp=lp["adamw_f32"], mom=m, var=v,
                   scalars=scalars("adamw_f32"))

    def bfp8():
        s = scalars("adamw_bfp8")
        wire.adamw_q(buf, n, 1, w["adamw_bfp8"], codec="bfp_rne", lp=lp["adamw_bfp8"], mom_q=mq, var_q=vq, scalars=s,
                     seed=O.sr_step_seed(0, step["adamw_bfp8"], 0))

    fns = {"adamw_f32": f32, "adamw_bfp8": bfp8}
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
    rec = {"probe": "moment_codec", "elems": n, "codec": "bfp_rne", "reps": reps, "device": torch.cuda.get_device_name(0)}
    for k in fns:
        mean = statistics.mean(us[k])
        rec[f"{k}_mean_us"] = round(mean, 2)
        rec[f"{k}_min_us"] = round(min(us[k]), 2)
        rec[f"{k}_spread_us"] = round(max(us[k]) - min(us[k]), 2)
        rec[f"{k}_TBps"] = round(BYTES[k] * n / mean * 1e6 / 1e12, 3)
    rec["ratio_f32_over_bfp8"] = round(statistics.mean(us["adamw_f32"]) / statistics.mean(us["adamw_bfp8"]), 3)
    rec["ratio_from_bytes"] = round(BYTES["adamw_f32"] / BYTES["adamw_bfp8"], 3)
    rec["state_bytes_per_param"] = {"f32": 8, "bfp8": 2.125}
    return rec


SIZES = [1024, 4096, 4096, 1024]


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


def step(a):
    """One trainer in this process: the flagship MLP's AdamW step through the forced multi-rank world-1 path
    (`force_comm`), moments in `a.variant` (f32 | bfp8); every step timed with device events from its first launch to
    the landing of its last update."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
    from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
    from fpga_ai_nic_amd.parallel.transport import NativeTransport

    tp = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    eng = NativeAllReduce(tp, codec="bfp_rne", force_comm=True)
    model = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=1, adam=True, moment_codec=a.variant,
                pad_fn=lambda n: eng.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=1e-3, weight_decay=1e-2, optimizer="adamw", moment_codec=a.variant)
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
    return {"probe": "moment_codec/step", "variant": a.variant, "mb": a.mb, "reps": a.reps,
            "mean_us": round(statistics.fmean(us), 2), "min_us": round(min(us), 2),
            "stdev_us": round(statistics.pstdev(us), 2), "prepack": bool(tr.prepack)}


def steps(a):
    """`--rounds` child processes per variant, alternating (several trainers in one process are not comparable: the
    third one created reads ~130 us slow)."""
    import subprocess

    me = os.path.abspath(__file__)
    out = {"f32": [], "bfp8": []}
    for _ in range(a.rounds):
        for k in out:
            r = subprocess.run([sys.executable, me, "--mode", "step", "--variant", k, "--reps", str(a.reps), "--warmup",
                                str(a.warmup), "--mb", str(a.mb)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"child {k} failed ({r.returncode}): {r.stderr[-2000:]}")
            out[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"probe": "moment_codec/steps", "rounds": a.rounds, "reps": a.reps, "mb": a.mb}
    for k, rs in out.items():
        means = [r["mean_us"] for r in rs]
        rec[f"{k}_child_means_us"] = means
        rec[f"{k}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{k}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{k}_min_us"] = min(r["min_us"] for r in rs)
    rec["bfp8_minus_f32_mean_us"] = round(rec["bfp8_mean_us"] - rec["f32_mean_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step", "steps"], default="kernels")
    ap.add_argument("--variant", choices=["f32", "bfp8"], default="f32")
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
