"""The bounds of tests/test_gpu_edge_numerics.py can be met and are not empty — shown without a GPU: the same inputs
and the same checking functions, run on the CPU fallbacks of ops.gemm.gemm, ops.nn.softmax_xent_slabs and
ops.nn.softmax_xent. (a) the float32 fallbacks pass every check; (b) outputs with the mistakes an edge path can make —
the partial last K-tile dropped, the partial tile row missing, a truncated bf16 output, a mask that lets +0 through, a
store into a guard row or column, slabs summed in the wrong order, a column sum that reads one row past K — fail."""
import pytest
import test_gpu_edge_numerics as E
import test_gpu_epilogue_numerics as T
import torch

CPU = "cpu"


def _spec(name):
    return next(s for s in T.SPECS + E.F32_SPECS if s.name == name)


# ---------------------------------------------------------------------------------------------------------------
# (a) the fallbacks pass


@pytest.mark.parametrize("shape", list(E.BF16_SHAPES))
@pytest.mark.parametrize("tile", E.BF16_TILES)
def test_bf16_edge_fallback_passes(tile, shape):
    E.all_bf16_epilogues(CPU, tile, shape)


@pytest.mark.parametrize("tile", E.BF16_TILES)
def test_bf16_subtile_fallback_passes(tile):
    E.subtile_bf16_epilogues(CPU, tile)


def test_bf16_staged_fallback_passes():
    E.staged_bf16_case(CPU)


@pytest.mark.parametrize("MN", list(E.F32_SHAPES))
def test_f32_fallback_passes(MN):
    E.all_f32_epilogues(CPU, MN)


def test_f32_colsum_fallback_passes():
    E.f32_colsum_case(CPU)


@pytest.mark.parametrize("sk", E.SLAB_SPLITS)
@pytest.mark.parametrize("Cc", E.SLAB_WIDTHS)
def test_slab_fallback_passes(Cc, sk):
    E.all_slab_cases(CPU, Cc, sk)


def test_slab_fallback_refuses():
    E.slab_refusals(CPU)


# ---------------------------------------------------------------------------------------------------------------
# (b) wrong outputs fail

BF16_CASE = E.bf16_case((128, 128), "sliver", 72)  # 136 x 136, K = one K-tile + one chunk
F32_CASE = (136, 136, 40, 128, 128, True)


@pytest.mark.parametrize("case,ktile", [(BF16_CASE, 64), (F32_CASE, 32)])
def test_dropped_partial_k_tile_fails(case, ktile):
    inp = E.inputs(case, CPU)
    K = case[2] // ktile * ktile
    assert 0 < K < case[2]
    wrong = inp["A"][:, :K].float() @ inp["B"][:K].float()
    with pytest.raises(AssertionError, match="out of bound"):
        E.verify_gemm(CPU, case, _spec("none_f32"), wrong, what="K truncated to a K-tile multiple")


@pytest.mark.parametrize("case", [BF16_CASE, F32_CASE])
def test_missing_partial_tile_row_fails(case):
    spec = _spec("bias_f32")
    C = E.run_gemm(CPU, case, 1, False, False, spec)[0].clone()
    E.verify_gemm(CPU, case, spec, C, what="as computed")
    C[case[3]:] = 0.0  # the rows of the second (partial) tile row never stored
    with pytest.raises(AssertionError, match="out of bound"):
        E.verify_gemm(CPU, case, spec, C, what="partial tile row zero")


def test_truncated_bf16_output_fails():
    for name in ("bias_bf16", "bias_relu_bf16", "relu_mask_bf16"):
        spec = _spec(name)
        C32 = E.run_gemm(CPU, BF16_CASE, 1, False, False, spec, bf16=False)[0]
        E.verify_gemm(CPU, BF16_CASE, spec, C32.to(T.BF), what="rounded to nearest")
        with pytest.raises(AssertionError, match="out of bound"):
            E.verify_gemm(CPU, BF16_CASE, spec, T._truncate_to_bf16(C32), what="truncated")


@pytest.mark.parametrize("case", [BF16_CASE, F32_CASE])
def test_mask_that_lets_zero_through_fails(case):
    N = case[1]
    inp = E.inputs(case, CPU)
    spec = _spec("relu_mask_f32")
    C = E.run_gemm(CPU, case, 1, False, False, spec)[0].clone()
    E.verify_gemm(CPU, case, spec, C, what="as computed")
    last = slice(N - 8, N)  # aux >= 0 instead of > 0 on the last valid 8-column group only
    C[:, last] = torch.where(inp["aux"].double()[:, last] >= 0, inp["ab"][:, last],
                             torch.zeros_like(inp["ab"][:, last])).float()
    with pytest.raises(AssertionError, match="out of bound"):
        E.verify_gemm(CPU, case, spec, C, what="mask >= 0 on the last column group")


@pytest.mark.parametrize("case", [BF16_CASE, F32_CASE])
def test_store_into_a_guard_fails(case):
    M, N = case[:2]
    spec = _spec("none_f32")
    for r, c in ((M, 0), (0, N)):  # guard row M, guard column N (relative to the view)
        C, full, _, _ = E.run_gemm(CPU, case, 1, False, False, spec, T.PADDED)
        E.verify_gemm(CPU, case, spec, C, full, what="as computed")
        full[r, T.PADDED[2] + c] = 0.0
        with pytest.raises(AssertionError, match="outside the output view"):
            E.verify_gemm(CPU, case, spec, C, full, what=f"store at ({r}, {c})")


def test_slabs_summed_in_reverse_order_fail():
    Cc, sk = 520, 3
    inp = E.slab_inputs(Cc, sk, CPU)
    right, wrong = E.slab_logits(inp["ws"], inp["bias"]), E.slab_logits(inp["ws"], inp["bias"], reverse=True)
    differ = int((~E._bits_equal(right, wrong)).sum())
    assert differ > 0, "these slabs do not tell the two orders apart: pick another seed"
    finite = torch.isfinite(right)
    assert float((right - wrong)[finite].abs().max()) < 1e-5, "the two orders differ by rounding only"
    outs = E.run_slabs(CPU, Cc, sk, False, False)
    E.verify_slabs(CPU, Cc, sk, False, False, outs)
    outs[0][0].copy_(wrong)  # what a kernel that adds the slabs last to first would have written
    with pytest.raises(AssertionError, match="logits differ"):
        E.verify_slabs(CPU, Cc, sk, False, False, outs)


def test_colsum_with_a_row_past_k_fails():
    case = E.bf16_case((128, 128), "sliver", 72)
    spec = _spec("colsum")
    C, full, cs, csfull = E.run_gemm(CPU, case, 1, True, False, spec)
    E.verify_gemm(CPU, case, spec, C, full, cs, csfull, what="as computed")
    extra = torch.randn(case[1], generator=torch.Generator().manual_seed(5)).to(T.BF).float()  # finite, non-zero
    cs += extra
    with pytest.raises(AssertionError, match="column sums"):
        E.verify_gemm(CPU, case, spec, C, full, cs, csfull, what="one more row")
    cs -= extra
    csfull[case[1]] = 0.0
    with pytest.raises(AssertionError, match="past the end"):
        E.verify_gemm(CPU, case, spec, C, full, cs, csfull, what="colsum guard")
