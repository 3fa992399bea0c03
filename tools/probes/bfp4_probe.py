"""Probe: what the 4-bit wire costs or saves in the wire kernels of ONE GPU. On the flagship's largest bucket
(4096x4096 + 4096 values) and its smallest (4096x1024 + 1024), f32 gradients, one shard: `wire.pack`, `wire.reduce` at
1 and 2 slots, `wire.sgd` (master + momentum + bf16 copy) and `wire.pack_ef`, for `bfp_rne` (17 B per 16 values) and
`bfp4_rne` (9 B per 16 values), the two codecs alternating in one process: warm-up, then `--reps` repetitions, every
launch timed with its own pair of events. Prints one table row per kernel and codec — mean, min, max and standard
deviation in us, the bytes the kernel must move and the TB/s the mean achieves over them — and the spread of each
(`--out FILE` also writes the table there).

The bytes exchanged between ranks (what the narrower wire is for) are not measured here: that needs more than one GPU."""
import argparse
import os
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch

    from fpga_ai_nic_amd.ops import wire

    buckets = {"big": SIZES[1] * SIZES[2] + SIZES[2], "small": SIZES[2] * SIZES[3] + SIZES[3]}
    gen = torch.Generator(device="cuda").manual_seed(0)
    runs, nbytes = {}, {}
    for name, n in buckets.items():
        assert n % 256 == 0
        grad = torch.randn(n, device="cuda", generator=gen) * 1e-2
        two = torch.randn(2 * n, device="cuda", generator=gen) * 1e-2
        resid = torch.zeros(n, device="cuda")
        master, mom = torch.randn(n, device="cuda", generator=gen), torch.zeros(n, device="cuda")
        lp = master.to(torch.bfloat16)
        for codec in CODECS:
            sb = wire.shard_bytes(codec, n)
            P = torch.empty(sb, dtype=torch.uint8, device="cuda")
            S = torch.empty(sb, dtype=torch.uint8, device="cuda")
            slots = torch.empty(2 * sb, dtype=torch.uint8, device="cuda")
            wire.pack(two, slots, n, codec)
            key = lambda op: (op, name, codec)  # noqa: E731
            runs[key("pack")] = lambda P=P, n=n, c=codec, grad=grad: wire.pack(grad, P, n, c)
            nbytes[key("pack")] = 4 * n + sb
            for k in (1, 2):
                runs[key(f"reduce{k}")] = lambda k=k, S=S, slots=slots, n=n, c=codec, grad=grad: wire.reduce(
                    slots, k, k - 1, grad, S, None, n, c)
                nbytes[key(f"reduce{k}")] = 4 * n + k * sb
            # lr 0: the planes keep their values over the repetitions
            runs[key("sgd")] = lambda slots=slots, n=n, c=codec, master=master, mom=mom, lp=lp: wire.sgd(
                slots, n, 1, master, codec=c, lp=lp, mom=mom, lr=0.0, momentum=0.9)
            nbytes[key("sgd")] = sb + 18 * n  # wire in; master and momentum in and out, bf16 copy out
            runs[key("pack_ef")] = lambda P=P, n=n, c=codec, grad=grad, resid=resid: wire.pack_ef(grad, resid, P, n, c)
            nbytes[key("pack_ef")] = 12 * n + sb
    for _ in range(a.warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():  # (every repetition runs every kernel of both codecs once: they alternate)
            us[k].append(timed(f))
    lines = [f"# bfp4_probe: {torch.cuda.get_device_name(0)}, f32 gradients, one shard, reps {a.reps}, warmup {a.warmup}",
             f"# buckets: big {buckets['big']} values, small {buckets['small']} values; times in us per launch",
             f"{'kernel':<10}{'bucket':<7}{'codec':<10}{'mean':>9}{'min':>9}{'max':>9}{'stdev':>8}{'MB':>9}{'TB/s':>7}"]
    for (op, name, codec), v in us.items():
        mean = statistics.fmean(v)
        lines.append(f"{op:<10}{name:<7}{codec:<10}{mean:>9.2f}{min(v):>9.2f}{max(v):>9.2f}{statistics.pstdev(v):>8.2f}"
                     f"{nbytes[(op, name, codec)] / 1e6:>9.2f}{nbytes[(op, name, codec)] / mean * 1e6 / 1e12:>7.3f}")
    lines.append("# bfp4_rne against bfp_rne: difference of the means (us), and the spread (max - min) of each")
    for (op, name, codec), v in us.items():
        if codec != CODECS[0]:
            continue
        w = us[(op, name, CODECS[1])]
        lines.append(f"{op:<10}{name:<7}{statistics.fmean(w) - statistics.fmean(v):>+9.2f}   spread {CODECS[0]} "
                     f"{max(v) - min(v):.2f}, {CODECS[1]} {max(w) - min(w):.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
