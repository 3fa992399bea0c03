"""Probe: what stochastic rounding costs. Each mode prints one JSON line; `--mode all` runs every mode in a child
process of its own and writes the tables of `profiles/stochastic_rounding.txt` (`--out`).

`--mode kernels`: on the flagship's largest bucket (4096x4096 + 4096 values) and its smallest (4096x1024 + 1024), f32
gradients, both rne codecs, one shard: `wire.pack` against `wire.pack_sr` against `wire.pack_ef`, and `wire.reduce`
against `wire.reduce_sr` against `wire.reduce_ef` at 1 and 2 slots, alternating in one process: warm-up, then `--reps`
repetitions, every launch timed with its own pair of events; mean, min, max and standard deviation in us, and the
achieved TB/s from the mean over the bytes the kernel must move (the stochastic kernels move the plain kernels' bytes).

`--mode step`: the flagship MLP's training step through the forced multi-rank world-1 path (`force_comm`), SGD +
momentum, `--reps` repetitions alternating the trainers of `--variants`: `default` (GEMM-encoded, prepacked),
`noprepack`, `sr` (`prepack=False, stochastic_rounding=True`) and `ef` (`prepack=False, error_feedback=True`); each
step timed with device events from its first launch to the landing of its last update. `--tree DIR`: import the
package from DIR instead of this tree (a tree without the feature can run `--variants default`). A trailing digit
makes another trainer of the same variant (`noprepack,noprepack2,noprepack3`: what a trainer's position in the process
costs by itself).

`--mode steps`: the same trainers, but each in a child process of its own (`--mode step --variants <one>`), `--rounds`
children per variant, alternating. This is the comparison the report uses: with several trainers in one process the
third one created measured 135-145 us slower per step whatever its variant (`--mode step --variants
noprepack,noprepack2,noprepack3,noprepack4`, the report's position table).

`--mode ab --parent DIR`: the default step of the tree at DIR (a built checkout of the parent commit) against this
tree's, `--rounds` child processes each, alternating. `--mode bench --parent DIR`: `bench.py --gpus 1 --steps 100
--warmup 20` of both trees, `--rounds` runs each, alternating."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [1024, 4096, 4096, 1024]
CODECS = ["bfp_rne", "bfp4_rne"]


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

    buckets = {"big": SIZES[1] * SIZES[2] + SIZES[2], "small": SIZES[2] * SIZES[3] + SIZES[3]}
    gen = torch.Generator(device="cuda").manual_seed(0)
    runs, nbytes = {}, {}
    for codec in CODECS:
        for name, n in buckets.items():
            sb = wire.shard_bytes(codec, n)
            grad = torch.randn(n, device="cuda", generator=gen) * 1e-2
            resid = torch.zeros(n, device="cuda")
            P = torch.empty(sb, dtype=torch.uint8, device="cuda")
            slots = torch.empty(2 * sb, dtype=torch.uint8, device="cuda")
            wire.pack(torch.randn(2 * n, device="cuda", generator=gen) * 1e-2, slots, n, codec)
            S = torch.empty(sb, dtype=torch.uint8, device="cuda")
            kw = dict(grad=grad, resid=resid, P=P, slots=slots, S=S, n=n, codec=codec)
            k0 = f"{codec}/{name}"
            runs[f"{k0}/pack"] = lambda kw=kw: wire.pack(kw["grad"], kw["P"], kw["n"], kw["codec"])
            runs[f"{k0}/pack_sr"] = lambda kw=kw: wire.pack_sr(kw["grad"], kw["P"], kw["n"], kw["codec"], 12345, 0)
            runs[f"{k0}/pack_ef"] = lambda kw=kw: wire.pack_ef(kw["grad"], kw["resid"], kw["P"], kw["n"], kw["codec"])
            nbytes[f"{k0}/pack"] = nbytes[f"{k0}/pack_sr"] = 4 * n + sb
            nbytes[f"{k0}/pack_ef"] = 12 * n + sb
            for k in (1, 2):
                runs[f"{k0}/reduce{k}"] = lambda k=k, kw=kw: wire.reduce(
                    kw["slots"], k, k - 1, kw["grad"], kw["S"], None, kw["n"], kw["codec"])
                runs[f"{k0}/reduce{k}_sr"] = lambda k=k, kw=kw: wire.reduce_sr(
                    kw["slots"], k, k - 1, kw["grad"], kw["S"], kw["n"], kw["codec"], 12345, 0)
                runs[f"{k0}/reduce{k}_ef"] = lambda k=k, kw=kw: wire.reduce_ef(
                    kw["slots"], k, k - 1, kw["grad"], kw["resid"], kw["S"], kw["n"], kw["codec"])
                nbytes[f"{k0}/reduce{k}"] = nbytes[f"{k0}/reduce{k}_sr"] = 4 * n + k * sb
                nbytes[f"{k0}/reduce{k}_ef"] = 12 * n + k * sb
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            us[k].append(timed(f))
    rec = {"probe": "stochastic_rounding/kernels", "buckets": buckets, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "keys": list(runs)}
    for k, v in us.items():
        stats(rec, k, v)
        rec[f"{k}_bytes"] = nbytes[k]
        rec[f"{k}_TBps"] = round(nbytes[k] / rec[f"{k}_mean_us"] * 1e6 / 1e12, 3)
    return rec


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


VARIANTS = {"default": {}, "noprepack": dict(prepack=False),
            "sr": dict(prepack=False, stochastic_rounding=True, sr_seed=1),
            "ef": dict(prepack=False, error_feedback=True)}


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
        eng = NativeAllReduce(tp, codec=a.codec, force_comm=True)
        model = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=1, momentum=True,
                    pad_fn=lambda n, e=eng: e.layout(n).n_pad)
        trainers[k] = DataParallelTrainer(model, eng, lr=0.05, momentum=0.9, **VARIANTS[k.rstrip("0123456789")])
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
    rec = {"probe": "stochastic_rounding/step", "codec": a.codec, "sizes": SIZES, "mb": a.mb, "reps": a.reps,
           "warmup": a.warmup, "tree": os.path.abspath(a.tree or HERE), "device": torch.cuda.get_device_name(0),
           "kinds": kinds, "prepack": {k: bool(trainers[k].prepack) for k in kinds}}
    for k, v in us.items():
        stats(rec, f"step_{k}", v)
    return rec


def _child(args, timeout=900):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"child {args} failed ({r.returncode}): {r.stderr[-2000:]}")
    return r.stdout


def steps(a):
    me = os.path.abspath(__file__)
    kinds = a.variants.split(",")
    out = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k in kinds:
            o = _child([me, "--mode", "step", "--variants", k, "--codec", a.codec, "--reps", str(a.reps), "--warmup",
                        str(a.warmup), "--mb", str(a.mb)])
            out[k].append(json.loads(o.strip().splitlines()[-1]))
    rec = {"probe": "stochastic_rounding/steps", "codec": a.codec, "rounds": a.rounds, "reps": a.reps, "mb": a.mb,
           "kinds": kinds, "prepack": {k: out[k][0]["prepack"][k] for k in kinds}}
    for k, rs in out.items():
        means = [r[f"step_{k}_mean_us"] for r in rs]
        rec[f"{k}_child_means_us"] = means
        rec[f"{k}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{k}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{k}_rep_stdev_us"] = [r[f"step_{k}_stdev_us"] for r in rs]
        rec[f"{k}_min_us"] = min(r[f"step_{k}_min_us"] for r in rs)
    return rec


def ab(a):
    me = os.path.abspath(__file__)
    out = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            # (the parent tree has no such probe: this file runs against its package)
            o = _child([me, "--mode", "step", "--variants", "default", "--tree", tree, "--reps", str(a.reps), "--warmup",
                        str(a.warmup), "--mb", str(a.mb)])
            out[name].append(json.loads(o.strip().splitlines()[-1]))
    rec = {"probe": "stochastic_rounding/ab", "rounds": a.rounds, "reps": a.reps, "mb": a.mb}
    for name, rs in out.items():
        means = [r["step_default_mean_us"] for r in rs]
        rec[f"{name}_child_means_us"] = means
        rec[f"{name}_mean_us"] = round(statistics.fmean(means), 2)
        rec[f"{name}_child_spread_us"] = round(max(means) - min(means), 2)
        rec[f"{name}_rep_stdev_us"] = [r["step_default_stdev_us"] for r in rs]
    rec["this_minus_parent_mean_us"] = round(rec["this_mean_us"] - rec["parent_mean_us"], 2)
    return rec


def bench(a):
    out = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, tree in (("parent", a.parent), ("this", HERE)):
            o = _child([os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "20"])
            line = [l for l in o.strip().splitlines() if l.startswith("{")][-1]
            out[name].append(json.loads(line)["ms_per_step"])
    rec = {"probe": "stochastic_rounding/bench", "rounds": a.rounds}
    for name, v in out.items():
        rec[f"{name}_ms_per_step"] = v
        rec[f"{name}_mean_ms"] = round(statistics.fmean(v), 4)
        rec[f"{name}_spread_ms"] = round(max(v) - min(v), 4)
    rec["this_minus_parent_mean_ms"] = round(rec["this_mean_ms"] - rec["parent_mean_ms"], 4)
    return rec


def report(recs):
    """The text of profiles/stochastic_rounding.txt from the modes' records."""
    L = ["Stochastic rounding for the compressed mesh all-reduce: what it costs on one MI355X",
         "=" * 84,
         "Tool: tools/probes/sr_probe.py --mode all (modes kernels / steps / step / ab / bench, each in a process of its own).",
         "Every launch / step is timed with its own pair of device events; warm-up repetitions, then the timed",
         "repetitions; the kernels alternate inside one process, the trainers across processes. Nothing here is asserted",
         "by a test.", ""]
    k = recs.get("kernels")
    if k:
        L += [f"1. Kernels (mode kernels, {k['reps']} repetitions after {k['warmup']} warm-up, {k['device']}): one shard, f32",
              f"   gradients, big = {k['buckets']['big']} values, small = {k['buckets']['small']}. The stochastic kernels move",
              "   the plain kernels' bytes (4 B gradient + the wire per value; reduce at k slots reads k - 1 wire slots more);",
              "   the error-fed ones 8 B per value more (residual load + store). TB/s = bytes / mean time.", "",
              "   codec     bucket  kernel       mean us     min     max   stdev   TB/s"]
        for key in k["keys"]:
            codec, bucket, name = key.split("/")
            L.append(f"   {codec:9s} {bucket:6s}  {name:11s} {k[key + '_mean_us']:8.2f} {k[key + '_min_us']:7.2f} "
                     f"{k[key + '_max_us']:7.2f} {k[key + '_stdev_us']:7.2f} {k[key + '_TBps']:6.2f}")
        L += ["", "   stochastic minus plain, and error-fed minus plain, means in us (the stdev columns above are the yardstick):"]
        for codec in CODECS:
            for bucket in ("big", "small"):
                row = []
                for name in ("pack", "reduce1", "reduce2"):
                    b = k[f"{codec}/{bucket}/{name}_mean_us"]
                    row.append(f"{name} {k[f'{codec}/{bucket}/{name}_sr_mean_us'] - b:+.2f} / "
                               f"{k[f'{codec}/{bucket}/{name}_ef_mean_us'] - b:+.2f}")
                L.append(f"   {codec:9s} {bucket:6s}  " + "   ".join(row))
        L.append("")
    for tag in ("steps", "steps4"):
        t = recs.get(tag)
        if not t:
            continue
        L += [f"2{'b' if tag == 'steps4' else ''}. Training step, forced multi-rank world-1 path (mode steps, codec {t['codec']}, {t['mb']} rows): SGD +",
              f"   momentum on the flagship MLP, every trainer in a process of its own, {t['rounds']} child processes per trainer,",
              f"   alternating, {t['reps']} repetitions each: default = prepack (the GEMMs encode the wire; falls away by itself",
              "   for bfp4_rne), noprepack = the engine packs, sr = noprepack + stochastic_rounding, ef = noprepack +",
              "   error_feedback.", "",
              "   trainer     child means us" + " " * 14 + "mean     spread   min     stdev within a child   prepack"]
        for kind in t["kinds"]:
            L.append(f"   {kind:10s} " + "  ".join(f"{m:7.2f}" for m in t[f"{kind}_child_means_us"])
                     + f"   {t[f'{kind}_mean_us']:7.2f}   {t[f'{kind}_child_spread_us']:5.2f}   {t[f'{kind}_min_us']:7.2f}   "
                     + f"{min(t[f'{kind}_rep_stdev_us']):.1f} - {max(t[f'{kind}_rep_stdev_us']):.1f}" + " " * 12
                     + f"{t['prepack'][kind]}")
        if "sr" in t["kinds"] and "noprepack" in t["kinds"]:
            L += ["", f"   sr minus noprepack: {t['sr_mean_us'] - t['noprepack_mean_us']:+.2f} us per step"
                  + (f"; ef minus noprepack: {t['ef_mean_us'] - t['noprepack_mean_us']:+.2f} us"
                     if "ef" in t["kinds"] else "") + " (between the means of the children)."]
        L.append("")
    q = recs.get("position")
    if q:
        L += ["2c. What a trainer's position costs (mode step, four trainers of the SAME variant noprepack in one process,",
              "   alternating): a trainer's time depends on the order of creation whatever it runs (slowest here: position "
              + str(1 + max(range(len(q["kinds"])), key=lambda n: q[f"step_{q['kinds'][n]}_mean_us"])) + "),",
              "   so the trainers of tables 2 / 2b are compared across processes only. The cause is not known.", "",
              "   position   mean us     min     stdev"]
        for n, kind in enumerate(q["kinds"]):
            L.append(f"   {n + 1:<10d} {q[f'step_{kind}_mean_us']:7.2f} {q[f'step_{kind}_min_us']:8.2f} "
                     f"{q[f'step_{kind}_stdev_us']:7.2f}")
        L.append("")
    b = recs.get("ab")
    if b:
        L += [f"3. The step without the flag against the parent commit (mode ab): the default trainer alone, {b['rounds']} child",
              f"   processes per build, alternating parent / this tree, {b['reps']} repetitions each.", "",
              "   build    child means us" + " " * 14 + "mean     spread between children   stdev within a child"]
        for name in ("parent", "this"):
            L.append(f"   {name:8s} " + "  ".join(f"{m:7.2f}" for m in b[f"{name}_child_means_us"])
                     + f"   {b[f'{name}_mean_us']:7.2f}   {b[f'{name}_child_spread_us']:5.2f}" + " " * 20
                     + f"{min(b[f'{name}_rep_stdev_us']):.1f} - {max(b[f'{name}_rep_stdev_us']):.1f}")
        L += ["", f"   this minus parent: {b['this_minus_parent_mean_us']:+.2f} us between the means; the parent's own spread "
              f"between children is {b['parent_child_spread_us']:.2f} us.", ""]
    c = recs.get("bench")
    if c:
        L += [f"4. bench.py --gpus 1 --steps 100 --warmup 20 (the flagship world-1 step: GEMM-fused update, no engine request),",
              f"   this tree and the parent build alternating, {c['rounds']} runs each, ms per step:"]
        for name in ("this", "parent"):
            L.append(f"     {name:7s} " + "   ".join(f"{v:.4f}" for v in c[f"{name}_ms_per_step"])
                     + f"   mean {c[f'{name}_mean_ms']:.4f}   spread {c[f'{name}_spread_ms']:.4f}")
        L += [f"   this minus parent: {c['this_minus_parent_mean_ms']:+.4f} ms; the parent's own spread between runs is "
              f"{c['parent_spread_ms']:.4f} ms.", ""]
    L += ["5. Bytes between ranks: nil by construction against error feedback and against the plain wire — the wire format",
          "   is unchanged. What stochastic rounding saves against error feedback is the f32 plane per bucket and rank and",
          "   the 8 B per value of HBM traffic in both encoders (tables 1 and 2). More than one GPU: unmeasured here."]
    return "\n".join(L) + "\n"


def run_all(a):
    me = os.path.abspath(__file__)
    base = ["--reps", str(a.reps), "--warmup", str(a.warmup), "--mb", str(a.mb)]
    jobs = [("kernels", ["--mode", "kernels"]),
            ("steps", ["--mode", "steps", "--variants", "default,noprepack,sr,ef", "--rounds", str(a.rounds)]),
            ("steps4", ["--mode", "steps", "--variants", "noprepack,sr,ef", "--codec", "bfp4_rne", "--rounds",
                        str(a.rounds)]),
            ("position", ["--mode", "step", "--variants", "noprepack,noprepack2,noprepack3,noprepack4"])]
    if a.parent:
        jobs += [("ab", ["--mode", "ab", "--parent", a.parent, "--rounds", str(a.rounds)]),
                 ("bench", ["--mode", "bench", "--parent", a.parent, "--rounds", str(a.rounds)])]
    recs = {}
    for tag, args in jobs:
        recs[tag] = json.loads(_child([me] + args + base, timeout=1100).strip().splitlines()[-1])
        print(json.dumps({tag: recs[tag]}), flush=True)
    out = a.out or os.path.join(HERE, "profiles", "stochastic_rounding.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(report(recs))
    return {"probe": "stochastic_rounding/all", "out": out, "modes": list(recs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "step", "steps", "ab", "bench", "all"], default="all")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mb", type=int, default=1792)
    ap.add_argument("--codec", default="bfp_rne")
    ap.add_argument("--variants", default="default,noprepack,sr,ef")
    ap.add_argument("--tree", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    rec = {"kernels": kernels, "step": step, "steps": steps, "ab": ab, "bench": bench, "all": run_all}[a.mode](a)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
