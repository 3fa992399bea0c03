"""Probe: what global-norm clipping costs. Three modes, each prints one JSON line (`--out FILE` also writes it there).

`--mode kernels`: the norm pass (`wire.sumsq`) on the flagship's largest bucket (4096x4096 + 4096, bfp_rne: 17 wire
bytes per 16 values, nothing stored per element) and on its smallest (4096x1024 + 1024), the coefficient launch over
the three buckets' partials, and the SGD-momentum update of the largest bucket with and without
the clip words, alternating in one process: warm-up, then `--reps` repetitions, every launch timed with its own pair of
events; mean, min and max us, and the wire-read GB/s of the norm pass from the mean.

`--mode step`: the flagship MLP's training step through the forced multi-rank world-1 path (`force_comm`: comm stream,
epilogues on the compute stream), SGD + momentum, `--reps` repetitions alternating a clipped trainer
(`max_grad_norm=1e30`: the coefficient is 1, the weights the unclipped trainer's) and an unclipped one, each step timed
with device events from its first launch to the landing of its last update. `--clip 0`: the unclipped trainer alone
(what another tree's build can run too). `--tree DIR`: import the package from DIR instead of this tree.

`--mode ab --parent DIR`: the unclipped step of the tree at DIR (a built checkout of the parent commit) against this
tree's, `--rounds` child processes each, alternating; every child runs `--mode step --clip 0`. Reports each child's mean
and the spread within each build's own repetitions."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [1024, 4096, 4096, 1024]


def timed(f):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    f()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def stats(rec, key, v):
    rec[f"{key}_mean_us"] = round(statistics.fmean(v), 2)
    rec[f"{key}_min_us"] = round(min(v), 2)
    rec[f"{key}_max_us"] = round(max(v), 2)
    rec[f"{key}_stdev_us"] = round(statistics.pstdev(v), 2)


def kernels(a):
    import torch

    from fpga_ai_nic_amd.ops import wire

    codec = "bfp_rne"
    buckets = [cin * cout + cout for cin, cout in zip(SIZES[:-1], SIZES[1:])]
    g = torch.Generator(device="cuda").manual_seed(0)
    wires, parts = [], []
    for n in buckets:
        assert n % 256 == 0
        grad = torch.randn(n, device="cuda", generator=g) * 1e-2
        buf = torch.empty(wire.shard_bytes(codec, n), dtype=torch.uint8, device="cuda")
        wire.pack(grad, buf, n, codec)
        wires.append(buf)
        parts.append(torch.zeros(wire.sumsq_partials_for(buf, n), dtype=torch.float64, device="cuda"))
    words = torch.zeros(4, device="cuda")
    big = max(range(len(buckets)), key=lambda i: buckets[i])
    small = min(range(len(buckets)), key=lambda i: buckets[i])
    n = buckets[big]
    w0 = torch.randn(n, device="cuda", generator=g) * 0.02
    planes = {k: dict(w=w0.clone(), m=torch.zeros(n, device="cuda"), lp=w0.to(torch.bfloat16))
              for k in ("plain", "clip")}

    def sumsq(i):
        return wire.sumsq(wires[i], buckets[i], 1, codec=codec, partials=parts[i])

    def coef():
        wire.clip_coef([(p, 0, p.numel()) for p in parts], 1e30, 1.0, words)

    def sgd(k):
        p = planes[k]
        wire.sgd(wires[big], n, 1, p["w"], codec=codec, lp=p["lp"], mom=p["m"], lr=1e-3, momentum=0.9,
                 clip=words if k == "clip" else None)

    runs = {"sumsq_big": lambda: sumsq(big), "sumsq_small": lambda: sumsq(small), "clip_coef": coef,
            "sgd_plain": lambda: sgd("plain"), "sgd_clip": lambda: sgd("clip")}
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            us[k].append(timed(f))
    rec = {"probe": "clip_epilogue/kernels", "codec": codec, "buckets": buckets, "reps": a.reps, "warmup": a.warmup,
           "partials": [p.numel() for p in parts], "device": torch.cuda.get_device_name(0),
           "coef": float(words[0]), "total": float(words[1])}
    for k, v in us.items():
        stats(rec, k, v)
    for k, i in (("sumsq_big", big), ("sumsq_small", small)):
        rec[f"{k}_wire_bytes"] = wires[i].numel()
        rec[f"{k}_GBps"] = round(wires[i].numel() / rec[f"{k}_mean_us"] * 1e6 / 1e9, 1)
        rec[f"{k}_GBps_best"] = round(wires[i].numel() / rec[f"{k}_min_us"] * 1e6 / 1e9, 1)
    same = all(torch.equal(planes["plain"][x], planes["clip"][x]) for x in ("w", "m", "lp"))
    rec["coef_1_update_bit_identical"] = bool(same)
    return rec


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


def step(a):
    import torch

    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
    from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
    from fpga_ai_nic_amd.parallel.transport import NativeTransport

    tp = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    kinds = ["plain", "clip"] if a.clip else ["plain"]
    trainers = {}
    for k in kinds:
        eng = NativeAllReduce(tp, codec="bfp_rne", force_comm=True)
        model = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=1, momentum=True,
                    pad_fn=lambda n, e=eng: e.layout(n).n_pad)
        kw = dict(max_grad_norm=1e30) if k == "clip" else {}
        trainers[k] = (DataParallelTrainer(model, eng, lr=0.05, momentum=0.9, **kw), model)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(a.mb, SIZES[0], generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    y = torch.randint(0, SIZES[-1], (a.mb,), generator=g, dtype=torch.int32).cuda()

    def one(k):
        tr = trainers[k][0]
        tr.step(x, y)
        tr.finish_async()

    for _ in range(a.warmup):
        for k in kinds:
            one(k)
    torch.cuda.synchronize()
    us = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k in kinds:
            us[k].append(timed(lambda: one(k)))
    for tr, _ in trainers.values():
        tr.finish()
    rec = {"probe": "clip_epilogue/step", "sizes": SIZES, "mb": a.mb, "reps": a.reps, "warmup": a.warmup,
           "tree": os.path.abspath(a.tree or HERE), "device": torch.cuda.get_device_name(0)}
    for k, v in us.items():
        stats(rec, f"step_{k}", v)
    if a.clip:
        rec["clip_minus_plain_mean_us"] = round(rec["step_clip_mean_us"] - rec["step_plain_mean_us"], 2)
        same = all(torch.equal(p.master, q.master) for p, q in zip(trainers["plain"][1].layers,
                                                                    trainers["clip"][1].layers))
        rec["weights_bit_identical"] = bool(same)
        rec["grad_norm"] = [float(v) for v in trainers["clip"][0].grad_norm.cpu()]
    return rec


def ab(a):
    me = os.path.abspath(__file__)
    out = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            r = subprocess.run([sys.executable, me, "--mode", "step", "--clip", "0", "--tree", tree, "--reps",
                                str(a.reps), "--warmup", str(a.warmup), "--mb", str(a.mb)], capture_output=True,
                               text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name} child failed ({r.returncode}): {r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"probe": "clip_epilogue/ab", "rounds": a.rounds, "reps": a.reps, "mb": a.mb}
    for name, rs in out.items():
        means = [r["step_plain_mean_us"] for r in rs]
        rec[f"{name}_child_means_us"] = means
        rec[f"{name}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{name}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{name}_rep_stdev_us"] = [r["step_plain_stdev_us"] for r in rs]
        rec[f"{name}_rep_min_us"] = [r["step_plain_min_us"] for r in rs]
    rec["this_minus_parent_mean_us"] = round(rec["this_mean_us"] - rec["parent_mean_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step", "ab"], default="kernels")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mb", type=int, default=1792)
    ap.add_argument("--clip", type=int, default=1)
    ap.add_argument("--tree", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    rec = {"kernels": kernels, "step": step, "ab": ab}[a.mode](a)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
