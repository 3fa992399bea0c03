"""Probe: the Adafactor epilogue (wire.adafactor, six launches) against SGD with momentum (wire.sgd) and AdamW
(wire.adamw) on the 16.8 M-value bucket (4096x4096 + 4096 bias) and the 4.2 M-value one (1024x4096 + 4096), bfp_rne wire,
bf16 copy written, alternating in one process: warm-up, then 50 repetitions each, every call timed with its own pair of
events; then the six launches one by one (`phases` mask), 50 repetitions each. Mean, min and spread (max - min) in us.
Every figure is a CALL time: the event pair surrounds a Python call of the op, so it includes the host's enqueue path
(about 10 us for a one-block launch) and is an upper bound on the kernel time, not the kernel time.
Per element Adafactor moves the wire three times, master in and out and the bf16 copy: 3 x 1.0625 + 8 + 2 = 13.19 B
(derived, not measured; the fp64 tile partials add rows / 16 x 8 B per column); SGD-momentum 19.06 B, AdamW 27.06 B.
Prints one JSON line per bucket; `--out FILE` also writes them there."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402

BYTES = {"sgdm": 1.0625 + 4 * 4 + 2, "adafactor": 3 * 1.0625 + 2 * 4 + 2, "adamw": 1.0625 + 6 * 4 + 2}
LAUNCHES = ("stats", "factors", "rowscale", "rms", "scale", "apply")


def _time(fn, reps):
    us = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    return us


def _stats(rec, key, us):
    rec[f"{key}_mean_us"] = round(statistics.mean(us), 2)
    rec[f"{key}_min_us"] = round(min(us), 2)
    rec[f"{key}_spread_us"] = round(max(us) - min(us), 2)


def bucket(rows, cols, tail, reps, warmup):
    n_valid = rows * cols + tail
    n = (n_valid + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(0)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    buf = torch.empty(wire.shard_bytes("bfp_rne", n), dtype=torch.uint8, device="cuda")
    wire.pack(grad, buf, n, "bfp_rne")
    w = {k: torch.randn(n, device="cuda", generator=g) * 0.02 for k in BYTES}
    lp = {k: v.to(torch.bfloat16) for k, v in w.items()}
    m = {k: torch.zeros(n, device="cuda") for k in ("sgdm", "adamw")}
    v = torch.zeros(n, device="cuda")
    fac = torch.zeros(rows + cols + tail, device="cuda")
    ab = torch.empty_like(fac)
    partials = torch.empty(wire.adafactor_layout(rows, cols, n_valid)["length"], dtype=torch.float64, device="cuda")
    words = torch.zeros(4, device="cuda")
    step = [0]

    def sgdm():
        wire.sgd(buf, n, 1, w["sgdm"], codec="bfp_rne", lp=lp["sgdm"], mom=m["sgdm"], lr=1e-3, weight_decay=1e-2,
                 momentum=0.9, n_valid=n_valid)

    def adafactor(phases=63):
        step[0] += phases == 63
        wire.adafactor(buf, n, 1, w["adafactor"], fac, codec="bfp_rne", rows=rows, cols=cols,
                       scalars=O.adafactor_scalars(1e-3, 1e-2, max(step[0], 1)), lp=lp["adafactor"], n_valid=n_valid,
                       words=words, ab=ab, partials=partials, phases=phases)

    def adamw():
        wire.adamw(buf, n, 1, w["adamw"], codec="bfp_rne", lp=lp["adamw"], mom=m["adamw"], var=v,
                   scalars=O.adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, max(step[0], 1)), n_valid=n_valid)

    fns = {"sgdm": sgdm, "adafactor": adafactor, "adamw": adamw}
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            us[k] += _time(f, 1)
    rec = {"probe": "adafactor", "rows": rows, "cols": cols, "tail": tail, "codec": "bfp_rne", "reps": reps,
           "device": torch.cuda.get_device_name(0)}
    for k in fns:
        _stats(rec, k, us[k])
        rec[f"{k}_TBps"] = round(BYTES[k] * n_valid / statistics.mean(us[k]) * 1e6 / 1e12, 3)
    total = 0.0
    for i, name in enumerate(LAUNCHES):  # one by one: the buffers hold a whole update's values from the loop above
        t = _time(lambda i=i: adafactor(1 << i), reps)
        _stats(rec, f"launch_{name}", t)
        total += statistics.mean(t)
    rec["launches_sum_mean_us"] = round(total, 2)
    rec["adafactor_over_sgdm"] = round(statistics.mean(us["adafactor"]) / statistics.mean(us["sgdm"]), 3)
    rec["adafactor_over_sgdm_from_bytes"] = round(BYTES["adafactor"] / BYTES["sgdm"], 3)
    rec["state_bytes_per_bucket"] = {"sgdm": 4 * n_valid, "adafactor": 4 * (rows + cols + tail), "adamw": 8 * n_valid}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [bucket(4096, 4096, 4096, a.reps, a.warmup), bucket(1024, 4096, 4096, a.reps, a.warmup)]
    for r in recs:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
