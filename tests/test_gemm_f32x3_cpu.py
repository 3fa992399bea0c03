"""``precision="bf16x3"`` off the GPU: the torch definition of the split (ops/gemm.py) inside the derived per-element
bound, and the refusals of the public interface. The inputs and the bound are shared with tests/test_gpu_gemm_f32x3.py.

Bound against the float64 product of the f32 inputs (per element; K the depth, ``splits`` the split-K factor):

    B = (3.03 * 2^-16 + 1.01 * (3K + splits + 2) * 2^-24) * sum_k |a_k||b_k| + eps_epilogue

3 * 2^-16 * (1 + 2^-7): what the two bf16 pieces leave of each operand (2^-16 relative each) plus the dropped l_a*l_b;
the second term: f32 accumulation of the 3K exact products, the slab sum and the epilogue, in any order;
eps_epilogue: one f32 rounding of the result (2^-24 of its magnitude) per add the epilogue performs (bias, accumulate).
Inputs stay in [2^-20, 2^20] in magnitude: no underflow term."""
import functools

import pytest
import torch

from fpga_ai_nic_amd.ops import gemm as G

LAYOUTS = [(a, b) for a in (False, True) for b in (False, True)]
# name -> (epilogue, accumulate)
EPILOGUES = {"none": (G.EPI_NONE, False), "bias": (G.EPI_BIAS, False), "bias_relu": (G.EPI_BIAS_RELU, False),
             "relu_mask": (G.EPI_RELU_MASK, False), "accumulate": (G.EPI_NONE, True),
             "bias_accumulate": (G.EPI_BIAS, True)}
U24 = 2.0 ** -24


def coef(K, splits=1):
    return 3.03 * 2.0 ** -16 + 1.01 * (3 * K + splits + 2) * U24


@functools.lru_cache(maxsize=None)
def inputs(M, N, K):
    """randn times 2^U(-6, 6) per row of A and per column of B (group exponents differ across a fragment), magnitudes
    clamped into [2^-20, 2^20]; the float64 products, computed once and never written."""
    g = torch.Generator().manual_seed((M * 1009 + N) * 1013 + K)

    def scaled(rows, cols, dim):
        shape = (rows, 1) if dim == 0 else (1, cols)
        t = torch.randn(rows, cols, generator=g) * torch.exp2(torch.rand(shape, generator=g) * 12 - 6)
        return torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -20, 2.0 ** 20)

    A, B = scaled(M, K, 0), scaled(K, N, 1)
    scale = (A.abs().double() @ B.abs().double()).sqrt()  # bias / old C of the size of the products' spread
    bias = torch.randn(N, generator=g) * scale.mean(0).float()
    c_old = torch.randn(M, N, generator=g) * scale.float()
    aux = torch.randn(M, N, generator=g)
    return dict(A=A, At=A.t().contiguous(), B=B, Bt=B.t().contiguous(), bias=bias, aux=aux, c_old=c_old,
                ab=A.double() @ B.double(), absprod=A.abs().double() @ B.abs().double())


def run_case(shape, layout, epi_name, dev, split_k=None):
    """One ``gemm(..., precision="bf16x3")`` call on ``dev``; returns (output, float64 reference, bound B)."""
    M, N, K = shape
    a_t, b_t = layout
    epi, accumulate = EPILOGUES[epi_name]
    d = inputs(M, N, K)
    ref, bound = d["ab"], coef(K, split_k or 1) * d["absprod"]
    if epi in (G.EPI_BIAS, G.EPI_BIAS_RELU):
        ref = ref + d["bias"].double()
        bound = bound + U24 * (ref.abs() + bound)
    if epi == G.EPI_BIAS_RELU:
        ref = torch.relu(ref)
    if epi == G.EPI_RELU_MASK:
        ref = ref * (d["aux"] > 0)
    if accumulate:
        ref = ref + d["c_old"].double()
        bound = bound + U24 * (ref.abs() + bound)
    C = (d["c_old"].clone() if accumulate else torch.full((M, N), float("nan"))).to(dev)
    G.gemm(d["At" if a_t else "A"].to(dev), a_t, d["Bt" if b_t else "B"].to(dev), b_t, C, epi,
           bias=d["bias"].to(dev) if epi in (G.EPI_BIAS, G.EPI_BIAS_RELU) else None,
           aux=d["aux"].to(dev) if epi == G.EPI_RELU_MASK else None, accumulate=accumulate, split_k=split_k,
           precision="bf16x3")
    return C.cpu().double(), ref, bound


def check(out, ref, bound):
    err = (out - ref).abs()
    worst = (err / bound).max().item()
    print(f"max err / B = {worst:.3f}, max abs err = {err.max().item():.3e}")
    assert torch.isfinite(out).all() and worst <= 1.0


@pytest.mark.parametrize("epi_name", ["none", "bias_accumulate"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"at{int(l[0])}_bt{int(l[1])}")
def test_cpu_path_within_bound(layout, epi_name):
    check(*run_case((24, 40, 72), layout, epi_name, "cpu"))


def test_split_is_the_definition():
    x = inputs(24, 40, 72)["A"]
    h, l = G.split_bf16(x)
    assert h.dtype == l.dtype == torch.bfloat16
    r = x.double() - h.double() - l.double()
    assert (r.abs() <= 2.0 ** -16 * x.abs().double()).all()
    assert ((x.double() - h.double()).abs() <= 2.0 ** -8 * x.abs().double()).all()


def test_refusals():
    A, B, C = torch.zeros(8, 8), torch.zeros(8, 8), torch.zeros(8, 8)
    with pytest.raises(ValueError, match="precision must be"):
        G.gemm(A, False, B, False, C, precision="tf32")
    with pytest.raises(ValueError, match="f32 operands"):
        G.gemm(A.bfloat16(), False, B.bfloat16(), False, C, precision="bf16x3")
    refused = dict(colsum=torch.zeros(8), wire=(torch.zeros(8, dtype=torch.uint8), 8, 0, 1), update=object(),
                   defer_reduce={})
    for name, value in refused.items():
        with pytest.raises(ValueError, match=f"does not take {name}="):
            G.gemm(A, False, B, False, C, precision="bf16x3", **{name: value})
    G.gemm(A, False, B, False, C, precision="f32")  # the default dispatch under its name


def test_mlp_and_cli_refuse_bf16():
    from fpga_ai_nic_amd.cli import mlp_mpi
    from fpga_ai_nic_amd.models.mlp import MLP

    with pytest.raises(ValueError, match="dtype=torch.float32"):
        MLP([8, 8], dtype=torch.bfloat16, f32_gemm="bf16x3")
    with pytest.raises(ValueError, match="mfma\\|bf16x3"):
        MLP([8, 8], dtype=torch.float32, f32_gemm="xf32")
    assert MLP([8, 8], dtype=torch.float32, f32_gemm="bf16x3").f32_gemm == "bf16x3"
    with pytest.raises(ValueError, match="needs --dtype f32"):
        mlp_mpi.run(["1", "8", "0", "A", "8", "8", "8", "8", "8", "--f32-gemm", "bf16x3", "--device", "cpu"])
