"""The bounds of tests/test_gpu_epilogue_numerics.py can be met and are not empty — shown without a GPU: the same
inputs and the same checking functions, run on the CPU fallbacks of ops.gemm.gemm, ops.nn.softmax_xent and
ops.nn.col_sum. (a) the float32 fallbacks pass every check; (b) a bf16 output that truncates instead of rounding to
nearest fails the bf16-output GEMM checks; (c) a gradient whose non-label entries are zero fails the softmax check."""
import pytest
import test_gpu_epilogue_numerics as T
import torch

CPU = "cpu"
PAIRS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("tile", list(T.TILES))
def test_gemm_fallback_passes_and_truncation_fails(tile):
    placed = [(K, sk, T.PLAIN) for K, sk in T.KSPLITS] + [(192, 1, T.PADDED), (128, 2, T.PADDED)]
    for K, sk, place in placed:
        for a_t, b_t in T.layouts_of(tile):
            for spec in T.specs_of(tile, a_t, b_t):
                T.run_and_verify_gemm(CPU, tile, K, sk, a_t, b_t, spec, place, what="cpu")  # (a)
                if spec.bf16:  # (b)
                    C32 = T.run_gemm(CPU, tile, K, sk, a_t, b_t, spec, place, bf16=False)[0]
                    T.verify_gemm(CPU, tile, K, spec, C32.to(T.BF), what="cpu, rounded to nearest")
                    with pytest.raises(AssertionError, match="out of bound"):
                        T.verify_gemm(CPU, tile, K, spec, T._truncate_to_bf16(C32), what="cpu, truncated")


@pytest.mark.parametrize("name,a_t,b_t", [("bias_relu_bf16", False, False), ("relu_mask_bf16", False, True)])
def test_gemm_staged_placement_fallback(name, a_t, b_t):
    spec = next(s for s in T.SPECS if s.name == name)
    T.run_and_verify_gemm(CPU, (256, 128), 192, 1, a_t, b_t, spec, T.STAGED, what="cpu staged")


def test_gemm_checks_reject_wrong_epilogues():
    """The exact conditions and the guards are not empty either: a mask that lets +0 through, a clamp that leaves a
    negative value, a store past the view."""
    tile, K = (256, 256), 192
    inp = T.gemm_inputs(tile, K, CPU)
    mask = next(s for s in T.SPECS if s.name == "relu_mask_f32")
    C, full, _, _ = T.run_gemm(CPU, tile, K, 1, False, False, mask, T.PADDED)
    wrong = torch.where(inp["aux"].double() >= 0, inp["ab"], torch.zeros_like(inp["ab"])).float()
    with pytest.raises(AssertionError, match="out of bound"):
        T.verify_gemm(CPU, tile, K, mask, wrong, what="mask >= 0")
    full[3, 0] = 0.0
    with pytest.raises(AssertionError, match="outside the output view"):
        T.verify_gemm(CPU, tile, K, mask, C, full, what="guard")
    relu = next(s for s in T.SPECS if s.name == "bias_relu_f32")
    C = T.run_gemm(CPU, tile, K, 1, False, False, relu)[0].clone()
    _, _, zero = T.gemm_expected(tile, K, CPU, relu.epi, False, False)
    C[zero] = -1e-7  # inside the bound, but not exactly 0
    with pytest.raises(AssertionError, match="not exactly 0"):
        T.verify_gemm(CPU, tile, K, relu, C, what="clamp")


def _relative_error(out, ref, absolute=0.0):
    """Worst relative error of ``out`` (beyond an absolute term) where the reference is not 0."""
    err = ((out.double() - ref).abs() - absolute).clamp(min=0.0)
    nz = ref != 0
    return float((err[nz] / ref[nz].abs()).max()) if bool(nz.any()) else 0.0


def test_softmax_fallback_relative_error():
    """The measurement behind SMX_R: the worst relative error of the float32 fallback (f32 outputs) on the test's own
    inputs — of every gradient entry but the label's (p * grad_scale, nothing cancels: the plain relative error; the
    label's p - 1 is what the absolute term SMX_A is for), and of the loss beyond its absolute term. It must not
    exceed the recorded SMX_R_MEASURED by more than a quarter (another libm may move it a little); SMX_R is 8 x the
    recorded value."""
    worst_d = worst_l = 0.0
    rows = torch.arange(T.SMX_M)
    for Cc in T.SMX_WIDTHS:
        for in_bf16 in (False, True):
            inp = T.softmax_inputs(Cc, in_bf16, CPU)
            d, _, loss, _ = T.run_softmax(CPU, Cc, in_bf16, False)
            ref = inp["d"].clone()
            ref[rows, inp["y"].long()] = 0.0  # leaves the label entries out
            worst_d = max(worst_d, _relative_error(d, ref))
            worst_l = max(worst_l, _relative_error(loss, inp["loss"], T.SMX_A * inp["loss_scale"]))
    print(f"softmax fallback: worst relative error dlogits {worst_d:.3g}, loss {worst_l:.3g}")
    assert max(worst_d, worst_l) <= 1.25 * T.SMX_R_MEASURED
    assert T.SMX_R == min(8 * T.SMX_R_MEASURED, 1e-4)


@pytest.mark.parametrize("in_bf16,out_bf16", PAIRS)
@pytest.mark.parametrize("Cc", T.SMX_WIDTHS)
def test_softmax_fallback_passes_and_zeroed_gradient_fails(Cc, in_bf16, out_bf16):
    for padded in (False, True) if Cc in T.SMX_PADDED_WIDTHS else (False,):
        d, dfull, loss, lfull = T.run_softmax(CPU, Cc, in_bf16, out_bf16, padded)
        T.verify_softmax(CPU, Cc, in_bf16, out_bf16, d, dfull, loss, lfull, what="cpu")  # (a)
    y = T.softmax_inputs(Cc, in_bf16, CPU)["y"].long()
    rows = torch.arange(T.SMX_M)
    zeroed = torch.zeros_like(d)
    zeroed[rows, y] = d[rows, y]
    with pytest.raises(AssertionError, match="out of bound"):  # (c)
        T.verify_softmax(CPU, Cc, in_bf16, out_bf16, zeroed, what="cpu, non-label gradient zeroed")
    with pytest.raises(AssertionError, match="out of bound"):  # a normaliser that is 1 % off
        T.verify_softmax(CPU, Cc, in_bf16, out_bf16, d.float() * 1.01, what="cpu, 1 % off")


@pytest.mark.parametrize("M", T.CS_ROWS)
def test_col_sum_fallback_passes(M):
    for case in T.all_colsum_cases(M):
        T.run_and_verify_colsum(CPU, *case)
