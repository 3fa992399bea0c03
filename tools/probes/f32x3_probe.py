"""Cost and numerics of the bf16x3 split-precision GEMM (csrc/gemm/gemm_f32x3.hip) -> profiles/gemm_f32x3.txt.

Sections: (1) registers, scratch and occupancy of every instantiation, from the compiler's resource remarks (needs no
GPU; scratch must be 0); (2) the three MLP layouts at 1792 and 5376 rows x 2048 x 2048, four arms alternating inside
every repetition, device events around each call: today's f32 MFMA kernel, the bf16x3 kernel, and as a yardstick the
same three products as ONE call of the existing bf16 GEMM on K-concatenated pre-split planes ([A_h | A_h | A_l] .
[B_h ; B_l ; B_h]), timed without and with the torch ops that split and concatenate; (3) the two step errors behind
the tolerance of tests/test_gpu_gemm_f32x3.py::test_mlp_step; (4) ``mlp_mpi --dtype f32`` on the reference workload
with both ``--f32-gemm`` values (child processes, one after the other). Sections 2-4 need the GPU and fail without it.
``--parent DIR`` (a built checkout of the parent commit) adds bench.py on this tree and on DIR, alternating three
times; without it that comparison is written as unmeasured.

    python tools/probes/f32x3_probe.py [--out profiles/gemm_f32x3.txt] [--reps 50] [--resources-only] [--parent DIR]
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

LAYOUTS = (("forward", False, False), ("bwd-data", False, True), ("bwd-weight", True, False))
ROWS = (1792, 5376)
WORKLOAD = ["20", "5376", "0", "A", "32", "32", "32"] + ["2048"] * 11


def resources() -> list[str]:
    src = os.path.join(ROOT, "csrc", "gemm", "gemm_f32x3.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O3", "--offload-arch=gfx950",
                            f"-I{os.path.join(ROOT, 'csrc')}", "-c", src, "-o", os.path.join(tmp, "x3.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        # gemm_f32x3_kernel<AK, BKC, EPI, ACCUM, SPLIT> / f32x3_splitk_reduce_kernel<EPI, ACCUM>
        m = re.search(r"Function Name: \S*?(gemm_f32x3_kernel|f32x3_splitk_reduce_kernel)I(\S+?)EEv", line)
        if m:
            args = re.findall(r"Lb([01])|Li(\d)", m.group(2))
            cur = {"name": m.group(1), "args": tuple(int(b or i) for b, i in args)}
            rows.append(cur)
            continue
        m = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    out = ["gemm_f32x3_kernel<AK, BKC, EPI, ACCUM, SPLIT>: LDS is dynamic (64 KiB per workgroup: 2 workgroups = 2 "
           "waves/SIMD per CU, below the register limit shown)",
           f"{'kernel':<28}{'template args':<18}{'VGPRs':>7}{'AGPRs':>7}{'scratch B':>11}{'waves/SIMD':>12}"]
    for k in sorted(rows, key=lambda k: (k["name"] != "gemm_f32x3_kernel", k["args"])):
        out.append(f"{k['name']:<28}{str(k['args']):<18}{k['VGPRs']:>7}{k['AGPRs']:>7}{k['ScratchSize']:>11}"
                   f"{k['Occupancy']:>12}")
    worst = max(k["ScratchSize"] for k in rows)
    out.append(f"{len(rows)} instantiations, max scratch {worst} B")
    if worst:
        raise SystemExit("f32x3_probe: an instantiation spills to scratch")
    return out


def gemm_timings(reps: int) -> list[str]:
    import torch

    from fpga_ai_nic_amd.ops import gemm as G

    if not torch.cuda.is_available():
        raise SystemExit("f32x3_probe: the timing sections need the GPU")
    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    out = [f"{'rows x 2048 x 2048, layout':<30}{'arm':<26}{'median us':>10}{'min us':>9}{'max us':>9}{'TFLOP/s':>9}"
           f"{'max err / sum|a||b|':>22}"]
    for rows in ROWS:
        for name, a_t, b_t in LAYOUTS:
            # forward X[rows][2048] . W; bwd-data dZ[rows][2048] . W^T; bwd-weight X^T . dZ (K = rows)
            M, N, K = (2048, 2048, rows) if a_t else (rows, 2048, 2048)
            g = torch.Generator(device=dev).manual_seed(rows + 2 * a_t + b_t)
            A = torch.randn((K, M) if a_t else (M, K), device=dev, generator=g)
            B = torch.randn((N, K) if b_t else (K, N), device=dev, generator=g)
            Cs = {k: torch.empty(M, N, device=dev) for k in ("f32", "x3", "cat")}

            def planes():
                (ah, al), (bh, bl) = G.split_bf16(A), G.split_bf16(B)
                return torch.cat([ah, ah, al], 0 if a_t else 1), torch.cat([bh, bl, bh], 1 if b_t else 0)

            pa, pb = planes()

            def cat_split():
                a3, b3 = planes()
                G.gemm(a3, a_t, b3, b_t, Cs["cat"])

            arms = collections.OrderedDict([
                ("f32 MFMA (today)", lambda: G.gemm(A, a_t, B, b_t, Cs["f32"])),
                ("bf16x3 kernel", lambda: G.gemm(A, a_t, B, b_t, Cs["x3"], precision="bf16x3")),
                ("bf16 GEMM, K-concat planes", lambda: G.gemm(pa, a_t, pb, b_t, Cs["cat"])),
                ("  + split pass (torch ops)", cat_split)])
            times = {k: [] for k in arms}
            for rep in range(reps + 5):  # 5 warm-up repetitions (they also tune the bf16 plan)
                for k, fn in arms.items():
                    t = timed(fn)
                    if rep >= 5:
                        times[k].append(t)
            Ad, Bd = (A.t() if a_t else A).double(), (B.t() if b_t else B).double()
            ref, absprod = Ad @ Bd, Ad.abs() @ Bd.abs()
            errs = {"f32 MFMA (today)": Cs["f32"], "bf16x3 kernel": Cs["x3"], "bf16 GEMM, K-concat planes": Cs["cat"]}
            for k, t in times.items():
                med = statistics.median(t)
                e = f"2^{torch.log2(((errs[k].double() - ref).abs() / absprod).max()).item():.2f}" if k in errs else ""
                out.append(f"{f'{rows}, {name}':<30}{k:<26}{med:>10.1f}{min(t):>9.1f}{max(t):>9.1f}"
                           f"{2.0 * M * N * K / med / 1e6:>9.1f}{e:>22}")
    return out


def step_errors() -> list[str]:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_gemm_f32x3 as T

    ratio = T.coef(136) / ((136 + 2) * 2.0 ** -24)
    e_mfma, e_x3 = T._step_error("mfma"), T._step_error("bf16x3")
    return [f"max abs error of the master weights after one SGD step against float64 autograd: f32_gemm=mfma "
            f"{e_mfma:.3e}, f32_gemm=bf16x3 {e_x3:.3e} (x{e_x3 / e_mfma:.2f}); allowed ratio of the GEMM bounds at "
            f"K = 136: {ratio:.2f}"]


def _child(argv, cwd=ROOT, timeout=600):
    r = subprocess.run([sys.executable] + argv, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"f32x3_probe: {' '.join(argv)} exited {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def workload() -> list[str]:
    out = []
    for mode in ("mfma", "bf16x3"):
        text = _child(["-m", "fpga_ai_nic_amd.cli.mlp_mpi"] + WORKLOAD + ["--dtype", "f32", "--f32-gemm", mode])
        keep = [l for l in text.splitlines() if re.match(r"fp time|GFLOPS|SAMPLES/S|LOSS", l)]
        out.append(f"--f32-gemm {mode:<7} " + "; ".join(keep))
    return out


def bench_ab(parent: str | None) -> list[str]:
    if not parent:
        return ["bench.py --gpus 1 on this tree against a build of the parent commit: unmeasured (no --parent DIR)"]
    out = []
    for rnd in range(3):
        for tag, cwd in (("this tree", ROOT), ("parent", os.path.abspath(parent))):
            line = _child(["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=cwd).strip().splitlines()[-1]
            m = re.search(r'"(?:step_ms|ms_per_step|value)":\s*([0-9.eE+-]+)', line)
            out.append(f"round {rnd + 1}, {tag:<10} {m.group(0) if m else line[:160]}")
            print(out[-1], file=sys.stderr, flush=True)  # (progress: six runs of a minute or so each)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_f32x3.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    sections = [("resources (gfx950, compiler remarks)", resources)]
    if not a.resources_only:
        sections += [
            (f"GEMM arms; {a.reps} repetitions, the four arms alternating inside each, device events around every call "
             "(us; a call holds the host's enqueue path). randn operands", lambda: gemm_timings(a.reps)),
            ("one training step, MLP([64, 128, 72]), batch 136, SGD", step_errors),
            ("mlp_mpi, reference workload (10 x 2048^2 f32, MB 5376, one GPU)", workload),
            ("bench.py --gpus 1 --steps 200 --warmup 20 (the default bf16 path)", lambda: bench_ab(a.parent))]
    lines = ["bf16x3 split-precision GEMM (tools/probes/f32x3_probe.py)"]
    print(lines[0], flush=True)
    for title, fn in sections:  # (printed as they finish: the later sections take minutes)
        part = ["", "== " + title] + fn()
        print("\n".join(part), flush=True)
        lines += part
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
