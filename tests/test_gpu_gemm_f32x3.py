"""The bf16x3 split-precision GEMM (csrc/gemm/gemm_f32x3.hip) through ``ops.gemm.gemm(..., precision="bf16x3")``: every
output element inside the derived bound B of tests/test_gemm_f32x3_cpu.py against the float64 product of the f32
inputs, the sharpness a kernel without the cross terms misses, and one training step of the f32 MLP on it."""
import pytest
import torch
from test_gemm_f32x3_cpu import EPILOGUES, LAYOUTS, check, coef, inputs, run_case

from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import gemm as G
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (M, N, K, split_k): one tile and K tile; the two LDS stages wrap; M, N and K edges (zero-page staging, predicated
# stores); several tiles (XCD remap); slabs; slabs with ragged K ranges (17 K tiles as 6, 6, 5) on edge tiles
SHAPES = [(128, 128, 32, None), (128, 128, 96, None), (136, 200, 72, None), (256, 384, 64, None),
          (128, 128, 512, 2), (136, 72, 520, 3)]
ALL_EPILOGUES = SHAPES[2:3] + SHAPES[4:]
CASES = [(s, e) for s in SHAPES for e in EPILOGUES if e == "none" or s in ALL_EPILOGUES]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"at{int(l[0])}_bt{int(l[1])}")
@pytest.mark.parametrize("shape,epi_name", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_within_bound(shape, epi_name, layout):
    check(*run_case(shape[:3], layout, epi_name, DEV, split_k=shape[3]))


def test_sharpness_and_default_dispatch():
    """max |err| / sum|a||b| below 2^-13 (hi*hi alone sits near 2^-9); precision=None is bit-identical to itself
    before and after the bf16x3 call and differs from it (another kernel ran)."""
    d = inputs(128, 128, 512)
    A, B = d["A"].to(DEV), d["B"].to(DEV)
    out = [torch.empty(128, 128, device=DEV) for _ in range(3)]
    G.gemm(A, False, B, False, out[0])
    G.gemm(A, False, B, False, out[1], precision="bf16x3")
    G.gemm(A, False, B, False, out[2], precision=None)
    assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
    rel = ((out[1].cpu().double() - d["ab"]).abs() / d["absprod"]).max().item()
    print(f"max |err| / sum|a||b| = 2^{torch.log2(torch.tensor(rel)).item():.2f}")
    assert rel < 2.0 ** -13


def _step_error(f32_gemm):
    """Max abs error of the master weights after one SGD step against a float64 autograd step of the same model."""
    sizes, mb, lr = [64, 128, 72], 136, 0.1  # (the trainer's default learning rate)
    model = MLP(sizes, dtype=torch.float32, device=DEV, seed=3, f32_gemm=f32_gemm)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(mb, sizes[0], generator=g).to(DEV)
    y = torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV)
    Ws = [l.w_master.double().clone().requires_grad_(True) for l in model.layers]
    bs = [l.b_master.double().clone().requires_grad_(True) for l in model.layers]
    h = x.double()
    for i, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W + b
        if i + 1 < len(Ws):
            h = torch.relu(h)
    grads = torch.autograd.grad(torch.nn.functional.cross_entropy(h, y.long()), Ws + bs)
    tr = DataParallelTrainer(model, None, lr=lr)
    tr.step(x, y)
    tr.finish()
    err = 0.0
    for l, W, b, gW, gb in zip(model.layers, Ws, bs, grads[:len(Ws)], grads[len(Ws):]):
        err = max(err, (l.w_master.double() - (W - lr * gW)).abs().max().item(),
                  (l.b_master.double() - (b - lr * gb)).abs().max().item())
    return err


def test_mlp_step():
    """One engine-less SGD step of MLP([64, 128, 72], f32, f32_gemm="bf16x3"), batch 136: the updated master weights
    against a float64 autograd step. The tolerance is not fixed in advance: it is the error of the f32_gemm="mfma"
    step against the same float64 step, measured here, times the ratio of the two GEMM bounds at the step's largest K
    (136, the bwd-weight depth): coef(136) / ((136 + 2) * 2^-24) = 8.63.
    Measured on an MI355X (profiles/gemm_f32x3.txt): mfma step 6.988e-09, bf16x3 step 1.781e-08, a factor 2.55."""
    ratio = coef(136) / ((136 + 2) * 2.0 ** -24)
    e_mfma, e_x3 = _step_error("mfma"), _step_error("bf16x3")
    print(f"step max abs error: mfma {e_mfma:.3e}, bf16x3 {e_x3:.3e}, allowed ratio {ratio:.2f}")
    assert e_x3 <= ratio * e_mfma
