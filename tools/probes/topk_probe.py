"""Cost of the top-k sparsification kernels (csrc/topk/topk_kernels.hip) -> profiles/topk.txt.

Three sections: (1) registers, LDS, scratch and occupancy of every kernel, from the compiler's own resource remarks
(needs no GPU; scratch is expected to be 0 bytes); (2) the select on the 16.8 M- and 4.2 M-value buckets at density
1 % and 0.1 %, once on normal data and once on data whose keys share one top digit (values in [1, 1.125): the hot-bin
case of the per-wave histograms): 50 repetitions, each running the nine launches one at a time in the select's order
with device events around every launch (so every repetition is one valid select) and then the whole select between
one pair of events; median / min / max and the bytes the launch has to move over the median; (3) accumulate at worlds
2 and 8. The buckets (67 MB and 17 MB a plane) fit the Infinity Cache: the GB/s are not HBM traffic. Sections 2 and 3
need the GPU and fail without it.

    python tools/probes/topk_probe.py [--out profiles/topk.txt] [--reps 50] [--resources-only]
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
DENSITIES = (0.01, 0.001)
STAGES = ("hist0", "pick0", "hist1", "pick1", "hist2", "pick2", "count", "scan", "compact")


def resources() -> list[str]:
    src = os.path.join(ROOT, "csrc", "topk", "topk_kernels.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "--offload-arch=gfx950",
                            f"-I{os.path.join(ROOT, 'csrc')}", "-c", src, "-o", os.path.join(tmp, "tk.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(topk_\w+_kernel)(ILi(\d)E)?", line)
        if m:
            cur = {"name": m.group(1) + (f"<{m.group(3)}>" if m.group(3) else "")}
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
    return (f"{tag:<28}{name:<10}{med:>10.1f}{min(t):>9.1f}{max(t):>9.1f}{nbytes / 1e6:>10.1f}"
            f"{nbytes / med / 1e3:>8.0f}")


def timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import topk as TK

    if not torch.cuda.is_available():
        raise SystemExit("topk_probe: the timing sections need the GPU")
    C = _ext.require().topk
    dev = torch.device("cuda", 0)
    head = f"{'bucket, density, data':<28}{'launch':<10}{'median us':>10}{'min us':>9}{'max us':>9}{'MB moved':>10}{'GB/s':>8}"
    out = [head]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    for n in BUCKETS:
        n_pad = (n + 255) // 256 * 256
        for density in DENSITIES:
            k = TK.count(n, density)
            _, words, nbytes = TK.layout(n_pad, k)
            for data in ("normal", "one-digit"):
                gen = torch.Generator(device=dev).manual_seed(n % 1000 + k)
                g = (torch.randn(n_pad, device=dev, generator=gen) if data == "normal"
                     else 1 + torch.rand(n_pad, device=dev, generator=gen) * 0.124)
                e = torch.zeros(n_pad, device=dev)
                wire = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                scratch = torch.zeros(words, dtype=torch.int32, device=dev)
                moved = {"hist0": 12 * n, "hist1": 4 * n, "hist2": 4 * n, "count": 4 * n, "compact": 4 * n + 16 * k,
                         "pick0": 16384, "pick1": 8192, "pick2": 8192, "scan": 16 * TK.layout(n_pad, k)[0]}
                times = {s: [] for s in STAGES + ("select",)}
                for rep in range(reps + 5):  # 5 warm-up repetitions
                    for i, s in enumerate(STAGES):
                        t = timed(lambda: C.select(g, e, wire, scratch, n, k, 0, 1 << i))
                        if rep >= 5:
                            times[s].append(t)
                    e.zero_()  # (the same input to every whole select; a one-digit plane would leave [1, 1.125) otherwise)
                    t = timed(lambda: C.select(g, e, wire, scratch, n, k))
                    e.zero_()
                    if rep >= 5:
                        times["select"].append(t)
                tag = f"{n / 1e6:.1f} M, {density:g}, {data}"
                for s in STAGES:
                    out.append(_row(tag, s, times[s], moved[s]))
                out.append(_row(tag, "select", times["select"], sum(moved.values())))
    out += ["", head.replace("bucket, density, data", "bucket, density, world ")]
    for n in BUCKETS:
        n_pad = (n + 255) // 256 * 256
        for density in DENSITIES:
            k = TK.count(n, density)
            kp, nbytes = TK.k_pad(k), TK.layout(n_pad, k)[2]
            for world in (2, 8):
                wires = torch.zeros(world * nbytes, dtype=torch.uint8, device=dev)
                for r in range(world):  # k distinct ascending indices and normal values per rank
                    w = wires[r * nbytes:(r + 1) * nbytes]
                    idx = w[: 4 * kp].view(torch.int32)
                    idx.fill_(-1)
                    idx[:k] = torch.randperm(n, device=dev)[:k].sort().values.to(torch.int32)
                    w[4 * kp:].view(torch.float32)[:k] = torch.randn(k, device=dev)
                g = torch.zeros(n_pad, device=dev)
                t = [timed(lambda: C.accumulate(wires, world, g, n, k, 1.0 / world)) for _ in range(reps + 5)][5:]
                out.append(_row(f"{n / 1e6:.1f} M, {density:g}, {world}", "accumulate", t, 4 * n + world * 8 * k))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    lines = ["Top-k sparsification kernels (tools/probes/topk_probe.py)", "", "== resources (gfx950, compiler remarks)"]
    lines += resources()
    if not a.resources_only:
        lines += ["", f"== every launch alone, then the whole select; {a.reps} alternating repetitions, device events "
                      f"(us). The planes fit the Infinity Cache: the GB/s are not HBM traffic"] + timings(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
