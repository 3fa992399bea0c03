"""Cost of the PowerSGD low-rank kernels (csrc/lowrank/lowrank_kernels.hip) -> profiles/lowrank.txt.

Three sections: (1) registers, scratch and occupancy of every kernel, from the compiler's own resource remarks (needs
no GPU); (2) each kernel alone at 4096 x 4096 and 1024 x 4096, rank 4 and 16: 50 repetitions with the kernels
alternating inside each repetition, device events around every launch, median / min / max and the bytes the kernel
has to move over the median; (3) the two-rank reducer's relative Frobenius error against the fp64 run of the oracle
on the inputs of tests/test_gpu_lowrank.py::test_reducer_two_ranks. Sections 2 and 3 need the GPU and fail without it.

``--orth`` writes profiles/lowrank_cholqr.txt instead: the resources, then the orthogonalisation alone by both methods
(modified Gram-Schmidt in one workgroup; CholeskyQR2 in three launches over 256-row strips) at 4096 and 1024 rows,
r = 1, 4 and 16, the two methods alternating inside each repetition, on fresh copies of the same P.

    python tools/probes/lowrank_probe.py [--out profiles/lowrank.txt] [--reps 50] [--resources-only] [--orth]
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


def resources() -> list[str]:
    src = os.path.join(ROOT, "csrc", "lowrank", "lowrank_kernels.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "--offload-arch=gfx950",
                            f"-I{os.path.join(ROOT, 'csrc')}", "-c", src, "-o", os.path.join(tmp, "lr.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(lowrank_\w+_kernel)(ILb([01])E)?", line)
        if m:
            cur = {"name": m.group(1) + (f"<{m.group(3)}>" if m.group(2) else "")}  # (a template's bool argument)
            rows.append(cur)
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    out = [f"{'kernel':<30}{'VGPRs':>7}{'AGPRs':>7}{'scratch B':>11}{'waves/SIMD':>12}{'LDS B':>8}"]
    for k in rows:
        out.append(f"{k['name']:<30}{k['VGPRs']:>7}{k['AGPRs']:>7}{k['ScratchSize']:>11}{k['Occupancy']:>12}{k['LDS']:>8}")
    return out


def timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import lowrank_oracle as O

    if not torch.cuda.is_available():
        raise SystemExit("lowrank_probe: the timing sections need the GPU")
    C = _ext.require().lowrank
    dev = torch.device("cuda", 0)
    out = [f"{'shape':<12}{'r':>3}  {'kernel':<12}{'median us':>10}{'min us':>9}{'max us':>9}{'MB moved':>10}{'GB/s':>8}"]
    for rows, cols in ((4096, 4096), (1024, 4096)):
        for r in (4, 16):
            sp, sb, n_part = O.layout(rows, cols)
            g, e = torch.randn(rows * cols, device=dev), torch.randn(rows * cols, device=dev) * 0.125
            q = torch.from_numpy(O.init_q(cols, r, 0)).to(dev)
            part = torch.zeros(n_part, device=dev)
            p, qn, q2 = torch.zeros(rows, 16, device=dev), torch.zeros(cols, 16, device=dev), torch.zeros_like(q)
            C.project(g, e, q, part, rows, cols)
            C.combine(part, sp, p)
            p0 = p.clone()
            nm = rows * cols * 4
            # (orth and reconstruct work in place: orth on a fresh copy of P, reconstruct on planes whose values
            # do not matter to its time)
            kernels = {
                "project": (lambda: C.project(g, e, q, part, rows, cols), 2 * nm),
                "combine_p": (lambda: C.combine(part, sp, p), (sp + 1) * rows * 64),
                "orth": (lambda: C.orth(p, r), 0),
                "backproject": (lambda: C.backproject(g, e, p, part, rows, cols), 2 * nm),
                "combine_q": (lambda: C.combine(part, sb, qn), (sb + 1) * cols * 64),
                "reconstruct": (lambda: C.reconstruct(g, e, p, qn, q2, 1.0, rows, cols), 4 * nm),
            }
            times = {k: [] for k in kernels}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for rep in range(reps + 5):  # 5 warm-up repetitions
                for name, (fn, _) in kernels.items():
                    if name == "orth":
                        p.copy_(p0)
                    ev[0].record()
                    fn()
                    ev[1].record()
                    ev[1].synchronize()
                    if rep >= 5:
                        times[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
            for name, (_, nbytes) in kernels.items():
                t = times[name]
                med = statistics.median(t)
                rate = f"{nbytes / med / 1e3:8.0f}" if nbytes else f"{'-':>8}"
                out.append(f"{f'{rows}x{cols}':<12}{r:>3}  {name:<12}{med:>10.1f}{min(t):>9.1f}{max(t):>9.1f}"
                           f"{nbytes / 1e6:>10.1f}{rate}")
    return out


def orth_timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd.ops import lowrank as LR

    if not torch.cuda.is_available():
        raise SystemExit("lowrank_probe: the timing sections need the GPU")
    dev = torch.device("cuda", 0)
    out = [f"{'rows':<8}{'r':>3}  {'method':<10}{'median us':>10}{'min us':>9}{'max us':>9}{'p10 us':>9}{'p90 us':>9}"]
    for rows in (4096, 1024):
        for r in (1, 4, 16):
            p0 = torch.randn(rows, 16, generator=torch.Generator().manual_seed(rows + r)).to(dev)
            p0[:, r:] = 0
            p, part = torch.empty_like(p0), torch.zeros(4 * -(-rows // 256) * 256, device=dev)
            times = {"mgs": [], "cholqr2": []}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for rep in range(reps + 5):  # 5 warm-up repetitions
                for method in times:
                    p.copy_(p0)
                    ev[0].record()
                    LR.orth(p, r, method=method, part=part)
                    ev[1].record()
                    ev[1].synchronize()
                    if rep >= 5:
                        times[method].append(ev[0].elapsed_time(ev[1]) * 1e3)
            for method, t in times.items():
                dec = statistics.quantiles(t, n=10)
                out.append(f"{rows:<8}{r:>3}  {method:<10}{statistics.median(t):>10.1f}{min(t):>9.1f}{max(t):>9.1f}"
                           f"{dec[0]:>9.1f}{dec[-1]:>9.1f}")
    return out


def accuracy() -> list[str]:
    from types import SimpleNamespace

    import numpy as np
    import torch

    from fpga_ai_nic_amd.ops import lowrank_oracle as O
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    rows, cols, r = 80, 528, 4
    rng = np.random.default_rng(11)
    eighths = lambda *shape: np.round(rng.standard_normal(shape) * 8) / 8
    m = (eighths(rows, r) @ eighths(r, cols)).astype(np.float32)
    n = eighths(rows, cols).astype(np.float32)
    gs, zeros = [m + n, m - n], [np.zeros((rows, cols), np.float32)] * 2
    g32 = O.step(gs, zeros, O.init_q(cols, r, 0), r)[0]
    g64 = O.step(gs, zeros, O.init_q(cols, r, 0), r, dtype=np.float64)[0]

    def rank_fn(transport):
        b = SimpleNamespace(cin=rows, cout=cols, n=rows * cols, grad=torch.from_numpy(gs[transport.rank].ravel()).cuda())
        LowRankReducer(transport, r, seed=0).reduce(b)
        return b.grad.cpu().view(rows, cols).numpy().astype(np.float64)

    got = ThreadFabric(2).run(rank_fn)[0]
    fro = np.linalg.norm
    return [f"two-rank reducer, 80 x 528, r = 4, relative Frobenius error against the fp64 run: GPU "
            f"{fro(got - g64) / fro(g64):.3e}, f32 oracle {fro(g32 - g64) / fro(g64):.3e}"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="profiles/lowrank.txt, or profiles/lowrank_cholqr.txt with --orth")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--orth", action="store_true", help="time the orthogonalisation alone, mgs against cholqr2")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "lowrank_cholqr.txt" if a.orth else "lowrank.txt")
    lines = ["PowerSGD low-rank kernels (tools/probes/lowrank_probe.py)", "", "== resources (gfx950, compiler remarks)"]
    lines += resources()
    if a.orth and not a.resources_only:
        lines += ["", f"== orth alone (launch to completion, host launch cost of the three cholqr2 launches included), "
                      f"{a.reps} alternating repetitions, device events (us)"] + orth_timings(a.reps)
    elif not a.resources_only:
        lines += ["", f"== each kernel alone, {a.reps} alternating repetitions, device events (us)"] + timings(a.reps)
        lines += ["", "== accuracy"] + accuracy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
