"""Probe: what error feedback costs. Three modes, each prints one JSON line (`--out FILE` also writes it there).

`--mode kernels`: on the flagship's largest bucket (4096x4096 + 4096 values) and its smallest (4096x1024 + 1024), f32
gradients, bfp_rne, one shard: `wire.pack_ef` against `wire.pack`, and `wire.reduce_ef` against `wire.reduce` at 1 and 2
slots, alternating in one process: warm-up, then `--reps` repetitions, every launch timed with its own pair of events;
mean, min, max and standard deviation in us, and the achieved TB/s from the mean over the bytes the kernel must move
(pack: 4 B gradient + 17/16 B wire per value, with feedback + 8 B of residual; reduce at k slots: 4 B local +
(k - 1) * 17/16 B of slots + 17/16 B out, with feedback + 8 B).

`--mode step`: the flagship MLP's training step through the forced multi-rank world-1 path (`force_comm`), SGD +
momentum, `--reps` repetitions alternating three trainers: the default (GEMM-encoded, prepacked), `prepack=False`, and
`prepack=False` with `error_feedback=True`; each step timed with device events from its first launch to the landing of
its last update. `--variants default`: the default trainer alone (what a tree without the feature can run too).
`--tree DIR`: import the package from DIR instead of this tree.

`--mode ab --parent DIR`: the default step of the tree at DIR (a built checkout of the parent commit) against this
tree's, `--rounds` child processes each, alternating; every child runs `--mode step --variants default`."""
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
    buckets = {"big": SIZES[1] * SIZES[2] + SIZES[2], "small": SIZES[2] * SIZES[3] + SIZES[3]}
    gen = torch.Generator(device="cuda").manual_seed(0)
    runs, nbytes = {}, {}
    for name, n in buckets.items():
        assert n % 256 == 0
        sb = wire.shard_bytes(codec, n)
        grad = torch.randn(n, device="cuda", generator=gen) * 1e-2
        resid = torch.zeros(n, device="cuda")
        P = torch.empty(sb, dtype=torch.uint8, device="cuda")
        slots = torch.empty(2 * sb, dtype=torch.uint8, device="cuda")
        wire.pack(torch.randn(2 * n, device="cuda", generator=gen) * 1e-2, slots, n, codec)
        S = torch.empty(sb, dtype=torch.uint8, device="cuda")
        runs[f"pack_{name}"] = lambda grad=grad, P=P, n=n: wire.pack(grad, P, n, codec)
        runs[f"pack_ef_{name}"] = lambda grad=grad, resid=resid, P=P, n=n: wire.pack_ef(grad, resid, P, n, codec)
        nbytes[f"pack_{name}"] = 4 * n + sb
        nbytes[f"pack_ef_{name}"] = 12 * n + sb
        for k in (1, 2):
            runs[f"reduce{k}_{name}"] = lambda k=k, grad=grad, slots=slots, S=S, n=n: wire.reduce(
                slots, k, k - 1, grad, S, None, n, codec)
            runs[f"reduce{k}_ef_{name}"] = lambda k=k, grad=grad, slots=slots, S=S, resid=resid, n=n: wire.reduce_ef(
                slots, k, k - 1, grad, resid, S, n, codec)
            nbytes[f"reduce{k}_{name}"] = 4 * n + k * sb
            nbytes[f"reduce{k}_ef_{name}"] = 12 * n + k * sb
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            us[k].append(timed(f))
    rec = {"probe": "error_feedback/kernels", "codec": codec, "buckets": buckets, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for k, v in us.items():
        stats(rec, k, v)
        rec[f"{k}_bytes"] = nbytes[k]
        rec[f"{k}_TBps"] = round(nbytes[k] / rec[f"{k}_mean_us"] * 1e6 / 1e12, 3)
        rec[f"{k}_TBps_best"] = round(nbytes[k] / rec[f"{k}_min_us"] * 1e6 / 1e12, 3)
    return rec


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


VARIANTS = {"default": {}, "noprepack": dict(prepack=False), "ef": dict(prepack=False, error_feedback=True)}


def step(a):
    import torch

    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
    from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
    from fpga_ai_nic_amd.parallel.transport import NativeTransport

    tp = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    kinds = a.variants.split(",")
    trainers = {}
    for k in kinds:
        eng = NativeAllReduce(tp, codec="bfp_rne", force_comm=True)
        model = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=1, momentum=True,
                    pad_fn=lambda n, e=eng: e.layout(n).n_pad)
        trainers[k] = DataParallelTrainer(model, eng, lr=0.05, momentum=0.9, **VARIANTS[k])
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(a.mb, SIZES[0], generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    y = torch.randint(0, SIZES[-1], (a.mb,), generator=g, dtype=torch.int32).cuda()

    def one(k):
        trainers[k].step(x, y)
        trainers[k].finish_async()

    for _ in range(a.warmup):
        for k in kinds:
            one(k)
    torch.cuda.synchronize()
    us = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k in kinds:
            us[k].append(timed(lambda: one(k)))
    for tr in trainers.values():
        tr.finish()
    rec = {"probe": "error_feedback/step", "sizes": SIZES, "mb": a.mb, "reps": a.reps, "warmup": a.warmup,
           "tree": os.path.abspath(a.tree or HERE), "device": torch.cuda.get_device_name(0),
           "prepack": {k: bool(trainers[k].prepack) for k in kinds}}
    for k, v in us.items():
        stats(rec, f"step_{k}", v)
    return rec


def ab(a):
    me = os.path.abspath(__file__)
    out = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            r = subprocess.run([sys.executable, me, "--mode", "step", "--variants", "default", "--tree", tree, "--reps",
                                str(a.reps), "--warmup", str(a.warmup), "--mb", str(a.mb)], capture_output=True,
                               text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name} child failed ({r.returncode}): {r.stderr[-2000:]}")
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"probe": "error_feedback/ab", "rounds": a.rounds, "reps": a.reps, "mb": a.mb}
    for name, rs in out.items():
        means = [r["step_default_mean_us"] for r in rs]
        rec[f"{name}_child_means_us"] = means
        rec[f"{name}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{name}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{name}_rep_stdev_us"] = [r["step_default_stdev_us"] for r in rs]
        rec[f"{name}_rep_min_us"] = [r["step_default_min_us"] for r in rs]
    rec["this_minus_parent_mean_us"] = round(rec["this_mean_us"] - rec["parent_mean_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step", "ab"], default="kernels")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mb", type=int, default=1792)
    ap.add_argument("--variants", default="default,noprepack,ef")
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
