"""Probe: the decode + update epilogue on the flagship's 4096x4096+4096 bucket (bfp_rne wire, bf16 copy written), SGD
with momentum against AdamW, alternating in one process: warm-up, then 20 repetitions each, every launch timed with its
own pair of events; median us and bytes/s. Per element the SGD-momentum epilogue moves 19.06 bytes (wire 1.0625, w 4+4,
mom 4+4, lp 2) and AdamW 27.06 (the second moment's 4+4 on top): the expected ratio is 1.42, accepted up to 1.6 (the
correctly rounded divide and sqrt). Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 4096 * 4096 + 4096
    assert n % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    buf = torch.empty(wire.shard_bytes("bfp_rne", n), dtype=torch.uint8, device="cuda")
    wire.pack(grad, buf, n, "bfp_rne")
    planes = {}
    for k in ("sgd", "adamw"):
        w = torch.randn(n, device="cuda", generator=g) * 0.02
        planes[k] = dict(w=w, lp=w.to(torch.bfloat16), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
    step = [0]

    def sgd():
        p = planes["sgd"]
        wire.sgd(buf, n, 1, p["w"], codec="bfp_rne", lp=p["lp"], mom=p["m"], lr=1e-3, weight_decay=1e-2, momentum=0.9)

    def adamw():
        p = planes["adamw"]
        step[0] += 1
        s = O.adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[0])
        wire.adamw(buf, n, 1, p["w"], codec="bfp_rne", lp=p["lp"], mom=p["m"], var=p["v"], scalars=s)

    fns = {"sgd_momentum": sgd, "adamw": adamw}
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            us[k].append(s.elapsed_time(e) * 1e3)
    bytes_per = {"sgd_momentum": 1.0625 + 4 * 4 + 2, "adamw": 1.0625 + 6 * 4 + 2}
    med = {k: statistics.median(v) for k, v in us.items()}
    rec = {"probe": "adamw_epilogue", "elems": n, "codec": "bfp_rne", "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for k in fns:
        rec[f"{k}_us"] = round(med[k], 2)
        rec[f"{k}_min_us"] = round(min(us[k]), 2)
        rec[f"{k}_TBps"] = round(bytes_per[k] * n / med[k] * 1e6 / 1e12, 3)
    rec["ratio_adamw_over_sgd"] = round(med["adamw"] / med["sgd_momentum"], 3)
    rec["ratio_from_bytes"] = round(bytes_per["adamw"] / bytes_per["sgd_momentum"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
