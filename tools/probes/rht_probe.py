"""Cost of the rotated one-bit kernels (csrc/rht/rht_kernels.hip) -> profiles/rht.txt.

Two sections: (1) registers, LDS, scratch and occupancy of every kernel, from the compiler's own resource remarks
(needs no GPU; scratch is expected to be 0 bytes); (2) encode, decode (one rank) and the bare transform, forward and
inverse, on the 16.8 M- and 4.2 M-value buckets on normal data, alternating with sign1's ``wire.pack_ef`` on the same
gradient: 50 repetitions, each launch alone between a pair of device events; median / min / max and the bytes the
launch has to move over the median. The buckets (67 MB and 17 MB a plane) fit the Infinity Cache: the GB/s are not HBM
traffic. What the method saves is bytes between ranks, which one GPU cannot measure. Section 2 needs the GPU and fails
without it.

    python tools/probes/rht_probe.py [--out profiles/rht.txt] [--reps 50] [--resources-only]
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
SEED = 1


def resources() -> list[str]:
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "--offload-arch=gfx950",
                            f"-I{os.path.join(ROOT, 'csrc')}", "-c", os.path.join(ROOT, "csrc", "rht", "rht_kernels.hip"),
                            "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, check=True)
    cur = None
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            m = re.search(r"Function Name: \S*?(rht_\w+_kernel)(ILb([01])E)?", line)
            cur = None
            if m:
                cur = {"name": m.group(1) + ({"0": "<forward>", "1": "<inverse>"}.get(m.group(3), ""))}
                rows.append(cur)
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    out = [f"{'kernel':<34}{'VGPRs':>7}{'AGPRs':>7}{'scratch B':>11}{'waves/SIMD':>12}{'LDS B':>8}"]
    for k in sorted(rows, key=lambda k: k["name"]):
        out.append(f"{k['name']:<34}{k['VGPRs']:>7}{k['AGPRs']:>7}{k['ScratchSize']:>11}{k['Occupancy']:>12}{k['LDS']:>8}")
    return out


def timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import bfp_oracle
    from fpga_ai_nic_amd.ops import rht as RH
    from fpga_ai_nic_amd.ops import wire as W

    if not torch.cuda.is_available():
        raise SystemExit("rht_probe: the timing section needs the GPU")
    C = _ext.require()
    dev = torch.device("cuda", 0)
    out = [f"{'bucket':<12}{'launch':<22}{'median us':>10}{'min us':>9}{'max us':>9}{'MB moved':>10}{'GB/s':>8}"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    for n in BUCKETS:
        n_pad = (n + 255) // 256 * 256
        _, rot, nbytes = RH.layout(n_pad, n)
        g = torch.randn(n_pad, device=dev, generator=torch.Generator(device=dev).manual_seed(n % 1000))
        e, y, back = torch.zeros(rot, device=dev), torch.zeros(rot, device=dev), torch.zeros(n_pad, device=dev)
        wire = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        e1, dec = torch.zeros(n_pad, device=dev), torch.zeros(n_pad, device=dev)
        sign1 = torch.zeros(bfp_oracle.shard_bytes("sign1", n_pad), dtype=torch.uint8, device=dev)
        steps = [("rht.encode", 4 * n + 8 * rot + nbytes, lambda: C.rht.encode(g, e, wire, n, SEED, 0)),
                 ("rht.decode (1 rank)", nbytes + 4 * n, lambda: C.rht.decode(wire, 1, dec, n, SEED, 1.0, 0)),
                 ("rht.transform", 4 * n + 4 * rot, lambda: C.rht.transform(g, y, n_pad, n, SEED, False, 0)),
                 ("rht.transform inverse", 4 * n + 4 * rot, lambda: C.rht.transform(y, back, n_pad, n, SEED, True, 0)),
                 ("sign1 wire.pack_ef", 12 * n_pad + sign1.numel(), lambda: W.pack_ef(g, e1, sign1, n_pad, "sign1"))]
        times = {name: [] for name, _, _ in steps}
        for rep in range(reps + 5):  # 5 warm-up repetitions
            for name, _, fn in steps:
                t = timed(fn)
                if rep >= 5:
                    times[name].append(t)
        tag = f"{n / 1e6:.1f} M"
        for name, moved, _ in steps:
            med = statistics.median(times[name])
            out.append(f"{tag:<12}{name:<22}{med:>10.1f}{min(times[name]):>9.1f}{max(times[name]):>9.1f}"
                       f"{moved / 1e6:>10.1f}{moved / med / 1e3:>8.0f}")
        out.append(f"{tag:<12}one rank sends {nbytes / 1e6:.2f} MB per reduction and receives (world - 1) times that; "
                   f"sign1 sends {sign1.numel() / 1e6:.2f} MB, f32 {4 * n / 1e6:.2f} MB")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rht.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    lines = ["Rotated one-bit kernels (tools/probes/rht_probe.py)", "", "== resources (gfx950, compiler remarks)"]
    lines += resources()
    if not a.resources_only:
        lines += ["", f"== every launch alone on normal data, alternating with sign1's pack_ef; {a.reps} repetitions, "
                      f"device events (us). The planes fit the Infinity Cache: the GB/s are not HBM traffic"]
        lines += timings(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
