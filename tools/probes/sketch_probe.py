"""Cost of the count-sketch kernels (csrc/sketch/sketch_kernels.hip) -> profiles/sketch.txt.

Two sections: (1) registers, LDS, scratch and occupancy of every kernel, from the compiler's own resource remarks
(needs no GPU; scratch is expected to be 0 bytes); (2) one reduction's launches on the 16.8 M- and 4.2 M-value buckets
at density 1 % with R = 5, C = 65536 on normal data: 50 repetitions, each running every launch on its own between a pair
of device events in the reduction's order (so every repetition is one valid reduction of one rank), then the whole
top-k select on the same gradient, alternating; median / min / max and the bytes the launch has to move over the
median. The accumulate reads both planes once per row (R times in all). The buckets (67 MB and 17 MB a plane) fit the
Infinity Cache: the GB/s are not HBM traffic. What the method saves is bytes between ranks, which one GPU cannot
measure. Section 2 needs the GPU and fails without it.

    python tools/probes/sketch_probe.py [--out profiles/sketch.txt] [--reps 50] [--resources-only]
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BUCKETS = (4096 * 4096 + 4096, 1024 * 4096 + 4096)
DENSITY, ROWS, COLS, SEED = 0.01, 5, 65536, 1
SELECT = ("hist0", "pick0", "hist1", "pick1", "hist2", "pick2", "count", "scan", "compact")


def resources() -> list[str]:
    rows = []
    for src, pat in (("sketch/sketch_kernels.hip", r"(sketch_\w+_kernel)(ILi(\d)E)?"),
                     ("topk/topk_kernels.hip", r"(topk_(?:hist|compact)_kernel)(ILi0ELb1|ILb1)()")):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3",
                                "--offload-arch=gfx950", f"-I{os.path.join(ROOT, 'csrc')}", "-c",
                                os.path.join(ROOT, "csrc", src), "-o", os.path.join(tmp, "k.o"),
                                "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
        cur = None
        for line in r.stderr.splitlines():
            if "Function Name:" in line:
                m = re.search(r"Function Name: \S*?" + pat, line)
                cur = None
                if m:
                    tag = f"<{m.group(3)}>" if m.group(3) else "<keys>" if "Lb1" in m.group(0) else ""
                    cur = {"name": m.group(1) + tag}
                    rows.append(cur)
                continue
            m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                          line)
            if m and cur is not None:
                cur[m.group(1).split(" ")[0]] = int(m.group(2))
    out = [f"{'kernel':<30}{'VGPRs':>7}{'AGPRs':>7}{'scratch B':>11}{'waves/SIMD':>12}{'LDS B':>8}"]
    for k in sorted(rows, key=lambda k: k["name"]):
        out.append(f"{k['name']:<30}{k['VGPRs']:>7}{k['AGPRs']:>7}{k['ScratchSize']:>11}{k['Occupancy']:>12}{k['LDS']:>8}")
    return out


def _row(tag, name, t, nbytes):
    med = statistics.median(t)
    return (f"{tag:<12}{name:<20}{med:>10.1f}{min(t):>9.1f}{max(t):>9.1f}{nbytes / 1e6:>10.1f}"
            f"{nbytes / med / 1e3:>8.0f}")


def timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import sketch as SK
    from fpga_ai_nic_amd.ops import topk as TK

    if not torch.cuda.is_available():
        raise SystemExit("sketch_probe: the timing section needs the GPU")
    C = _ext.require()
    dev = torch.device("cuda", 0)
    out = [f"{'bucket':<12}{'launch':<20}{'median us':>10}{'min us':>9}{'max us':>9}{'MB moved':>10}{'GB/s':>8}"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    for n in BUCKETS:
        n_pad = (n + 255) // 256 * 256
        k = TK.count(n, DENSITY)
        sk, part, words, nbytes = SK.layout(n_pad, k, ROWS, COLS)
        tiles = TK.layout(n_pad, k)[0]
        g0 = torch.randn(n_pad, device=dev, generator=torch.Generator(device=dev).manual_seed(n % 1000))
        g, e, e2 = g0.clone(), torch.zeros(n_pad, device=dev), torch.zeros(n_pad, device=dev)
        S, P = torch.zeros(sk, device=dev), torch.zeros(part, device=dev)
        wire, wire2 = (torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
        scratch, scratch2 = (torch.zeros(words, dtype=torch.int32, device=dev) for _ in range(2))
        strips = part // sk
        sel = {"hist0": 4 * n, "hist1": 4 * n, "hist2": 4 * n, "count": 4 * n, "compact": 4 * n + 8 * k,
               "pick0": 16384, "pick1": 8192, "pick2": 8192, "scan": 16 * tiles}
        steps = [("accumulate", 8 * n * ROWS + 4 * part, lambda: C.sketch.sketch(g, e, P, S, n, ROWS, COLS, SEED, 0, 1)),
                 ("combine", 4 * (part + sk), lambda: C.sketch.sketch(g, e, P, S, n, ROWS, COLS, SEED, 0, 2)),
                 ("estimate", 16 * n + 4 * sk, lambda: C.sketch.estimate(g, e, S, n, ROWS, COLS, SEED, 0))]
        steps += [(f"keys {s}", sel[s], (lambda i: lambda: C.topk.select_keys(g, wire, scratch, n, k, 0, 1 << i))(i))
                  for i, s in enumerate(SELECT)]
        steps += [("fetch", 16 * k, lambda: C.sketch.fetch(e, wire, n, k, 0)),
                  ("topk.accumulate", 4 * n + 8 * k, lambda: C.topk.accumulate(wire, 1, g, n, k, 1.0, 0))]
        times = {name: [] for name, _, _ in steps}
        times["reduction (sum)"], times["topk.select"] = [], []
        for rep in range(reps + 5):  # 5 warm-up repetitions
            g.copy_(g0)
            e.zero_()
            e2.zero_()
            total = 0.0
            for name, _, fn in steps:
                t = timed(fn)
                total += t
                if rep >= 5:
                    times[name].append(t)
            t = timed(lambda: C.topk.select(g0, e2, wire2, scratch2, n, k))
            if rep >= 5:
                times["reduction (sum)"].append(total)
                times["topk.select"].append(t)
        tag = f"{n / 1e6:.1f} M"
        for name, moved, _ in steps:
            out.append(_row(tag, name, times[name], moved))
        out.append(_row(tag, "reduction (sum)", times["reduction (sum)"], sum(m for _, m, _ in steps)))
        out.append(_row(tag, "topk.select", times["topk.select"], 12 * n + 16 * n + 8 * k))
        out.append(f"{tag:<12}strips = {strips}; one rank sends {4 * (sk + TK.k_pad(k)) / 1e6:.2f} MB per reduction "
                   f"whatever the world size; top-k sends {nbytes / 1e6:.2f} MB and receives (world - 1) times that")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    lines = ["Count-sketch kernels (tools/probes/sketch_probe.py)", "", "== resources (gfx950, compiler remarks)"]
    lines += resources()
    if not a.resources_only:
        lines += ["", f"== every launch of one reduction alone (R = {ROWS}, C = {COLS}, density {DENSITY:g}, normal "
                      f"data), then the whole top-k select; {a.reps} alternating repetitions, device events (us). The "
                      f"planes fit the Infinity Cache: the GB/s are not HBM traffic"] + timings(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
