"""Probe: the trust-ratio (LAMB) epilogue against the AdamW epilogue on the flagship's 4096x4096+4096 bucket (bfp_rne
wire, bf16 copy written), alternating in one process: warm-up, then `--reps` repetitions, every launch timed with its own
pair of events; mean, min and max us and bytes/s from the mean. Per element AdamW moves 27.06 bytes (wire 1.0625, w 4+4,
both moments 4+4 each, lp 2); LAMB's pass 1 moves 21.06 (wire, w read, both moments read and written), the ratio launch
reads 32 KiB, pass 2 moves 18 (w and both moments read, w and lp written): 39.06 in all, 1.44 x AdamW. The yardstick is
the AdamW kernel's bytes/s in the same record and the spread between its repetitions. Prints one JSON line; `--out FILE`
also writes it there."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402


def timed(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    f()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 4096 * 4096 + 4096
    n_adapt = 4096 * 4096
    assert n % 256 == 0
    g = torch.Generator(device="cuda").manual_seed(0)
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    buf = torch.empty(wire.shard_bytes("bfp_rne", n), dtype=torch.uint8, device="cuda")
    wire.pack(grad, buf, n, "bfp_rne")
    planes = {}
    for k in ("adamw", "lamb"):
        w = torch.randn(n, device="cuda", generator=g) * 0.02
        planes[k] = dict(w=w, lp=w.to(torch.bfloat16), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
    pairs = wire.lamb_partials_for(planes["lamb"]["w"], n)
    partials = torch.zeros(2 * pairs, dtype=torch.float64, device="cuda")
    words = torch.zeros(3, device="cuda")
    step = [0, 0]

    def adamw():
        p = planes["adamw"]
        step[0] += 1
        s = O.adamw_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[0])
        return {"adamw": timed(lambda: wire.adamw(buf, n, 1, p["w"], codec="bfp_rne", lp=p["lp"], mom=p["m"],
                                                  var=p["v"], scalars=s))}

    def lamb():
        p = planes["lamb"]
        step[1] += 1
        s = O.lamb_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[1])
        t = {}
        t["lamb_pass1"] = timed(lambda: wire.lamb_moments(buf, n, 1, p["w"], codec="bfp_rne", mom=p["m"], var=p["v"],
                                                          scalars=s, partials=partials, n_adapt=n_adapt))
        t["lamb_ratio"] = timed(lambda: wire.lamb_ratio(partials, pairs, 1e-3, words))
        t["lamb_pass2"] = timed(lambda: wire.lamb_apply(p["w"], n, mom=p["m"], var=p["v"], scalars=s, words=words,
                                                        lp=p["lp"], n_adapt=n_adapt))
        # the three launches back to back, as a request's thunks enqueue them (no host wait in between)
        step[1] += 1
        s2 = O.lamb_scalars(1e-3, 1e-2, 0.9, 0.999, 1e-8, step[1])

        def three():
            wire.lamb_moments(buf, n, 1, p["w"], codec="bfp_rne", mom=p["m"], var=p["v"], scalars=s2,
                              partials=partials, n_adapt=n_adapt)
            wire.lamb_ratio(partials, pairs, 1e-3, words)
            wire.lamb_apply(p["w"], n, mom=p["m"], var=p["v"], scalars=s2, words=words, lp=p["lp"], n_adapt=n_adapt)

        t["lamb_epilogue"] = timed(three)
        return t

    for _ in range(a.warmup):
        adamw()
        lamb()
    torch.cuda.synchronize()
    us = {}
    for _ in range(a.reps):
        for f in (adamw, lamb):
            for k, v in f().items():
                us.setdefault(k, []).append(v)
    bytes_per = {"adamw": 1.0625 + 6 * 4 + 2, "lamb_pass1": 1.0625 + 5 * 4, "lamb_pass2": 3 * 4 + 4 + 2}
    bytes_per["lamb_epilogue"] = bytes_per["lamb_pass1"] + bytes_per["lamb_pass2"]
    rec = {"probe": "lamb_epilogue", "elems": n, "n_adapt": n_adapt, "codec": "bfp_rne", "reps": a.reps,
           "warmup": a.warmup, "partial_pairs": pairs, "device": torch.cuda.get_device_name(0),
           "phi": round(float(words[2]), 6)}
    for k, v in us.items():
        mean = statistics.fmean(v)
        rec[f"{k}_mean_us"] = round(mean, 2)
        rec[f"{k}_min_us"] = round(min(v), 2)
        rec[f"{k}_max_us"] = round(max(v), 2)
        if k in bytes_per:
            rec[f"{k}_TBps"] = round(bytes_per[k] * n / mean * 1e6 / 1e12, 3)
            rec[f"{k}_TBps_best"] = round(bytes_per[k] * n / min(v) * 1e6 / 1e12, 3)
            rec[f"{k}_TBps_worst"] = round(bytes_per[k] * n / max(v) * 1e6 / 1e12, 3)
    rec["ratio_lamb_over_adamw"] = round(rec["lamb_epilogue_mean_us"] / rec["adamw_mean_us"], 3)
    rec["ratio_sum_of_passes_over_adamw"] = round(
        (rec["lamb_pass1_mean_us"] + rec["lamb_ratio_mean_us"] + rec["lamb_pass2_mean_us"]) / rec["adamw_mean_us"], 3)
    rec["ratio_from_bytes"] = round(bytes_per["lamb_epilogue"] / bytes_per["adamw"], 2)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
