"""Per-element fp64 bounds next to the aligned path of tests/test_gpu_epilogue_numerics.py: the edge-tile bf16 GEMM
(gemm_bf16_kernel<..., RAGGED = true>: zero-page staging, predicated store_tile, ragged K splits with an empty split),
the f32 MFMA GEMM with its epilogues and split-K reduce (csrc/gemm/gemm_f32.hip), the softmax that folds the
classifier's split-K slabs (softmax_xent_slab_kernel, driven with synthetic slabs) and the wire epilogue on edge tiles.

Bounds (the project's own, see the aligned file):

* GEMM:  |out - ref64| <= 2e-5 * (|A| @ |B| [+ |bias|] [+ |C_old|]) + 1e-6, plus 2^-8 * |ref64| for a bf16 output.
         Every K here is <= 312, so 2e-5 is a worst-case bound for ANY f32 summation order:
         (K + splits + 2) * 2^-24 <= 1.9e-5 (f32 operands included, whose products round).
* slabs: logits bit-equal to torch's float32 ((s0 + s1) + ...) + bias (the kernel only adds: nothing contracts into an
         fma), loss / dlogits bit-equal to ops.nn.softmax_xent on those logits and inside its SMX_R / SMX_A bound
         against float64 of the same logits.
* wire:  bytes equal bfp_oracle.pack of the SAME plan's f32 EPI_NONE output (which the GEMM tests hold to the fp64
         bound); the bias segment by decoded value.

Every operand is a view into a taller (and, in the padded placement, wider) allocation whose surroundings are NaN,
and the bias has 8 NaN elements after it: a chunk that should have come from the zero page but was read from memory
poisons the result instead of faulting. Outputs sit in SENT-guarded allocations.

The helpers run on any device: tests/test_edge_numerics_cpu.py runs the same inputs and checks through the CPU
fallbacks (they must pass) and through deliberately wrong outputs (they must fail)."""
import functools

import numpy as np
import pytest
import test_gpu_epilogue_numerics as T
import torch
from test_gpu_epilogue_numerics import (BF, F32, HALF_ULP_BF16, MASK_EDGE, PADDED, PLAIN, SENT, SMX_R, STAGED, Spec,
                                        _check, _check_guard, _guarded, _widen)

from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import gemm as G
from fpga_ai_nic_amd.ops import nn as NN
from fpga_ai_nic_amd.ops import wire

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
LAYOUTS = [(a, b) for a in (False, True) for b in (False, True)]

# ---------------------------------------------------------------------------------------------------------------
# 1. GEMM cases: (M, N, K, bm, bn, f32) -> inputs and float64 products, computed once on the CPU

BF16_TILES = [(128, 128), (128, 256), (256, 128), (256, 256)]
# (K, split_k): one K-tile + one chunk; prologue / steady state / drain of the 3-stage ring with a partial last tile;
# 4 K-tiles as 2, 2 (the second split ends in the partial tile); 2, 2, 0 (an empty split, runtime-count reduce);
# 5 K-tiles as 2, 2, 1, 0 (an empty split, compile-time-4 reduce); K a BK multiple but not of BK * split
BF16_KSPLITS = [(72, 1), (200, 1), (200, 2), (200, 3), (312, 4), (192, 2)]
BF16_SHAPES = {
    "sliver": lambda bm, bn: (bm + 8, bn + 8),  # second tile row / column holds one 8-wide chunk
    "almost": lambda bm, bn: (2 * bm - 8, 2 * bn - 8),
    "k_only": lambda bm, bn: (bm, bn),  # aligned M, N, ragged K: mn_edge false, edge true
}
F32_SPECS = [
    Spec("none_f32", G.EPI_NONE, False, False, False),
    Spec("bias_f32", G.EPI_BIAS, False, False, False),
    Spec("bias_relu_f32", G.EPI_BIAS_RELU, False, False, False),
    Spec("relu_mask_f32", G.EPI_RELU_MASK, False, False, False),
    Spec("accumulate_f32", G.EPI_NONE, False, True, False),
    Spec("bias_accumulate_f32", G.EPI_BIAS, False, True, False),
]
# f32 GEMM (128 x 128 tiles, BK = 32): (M, N) -> (K, split_k)
F32_ALIGNED_KSPLITS = [(96, 1), (32, 1), (64, 2)]
F32_EDGE_KSPLITS = [(40, 1), (104, 1), (104, 2), (136, 4)]  # 136 / 4: 5 K-tiles as 2, 2, 1, 0
F32_SHAPES = {(256, 256): F32_ALIGNED_KSPLITS, (136, 136): F32_EDGE_KSPLITS, (248, 248): F32_EDGE_KSPLITS,
              (128, 128): F32_EDGE_KSPLITS, (8, 8): [(8, 1)]}


def bf16_specs(a_t, b_t):
    """The specs of the aligned file; the fused column sum is the bwd-weight layout's."""
    return [s for s in T.SPECS if not s.colsum or (a_t and not b_t)]


def bf16_case(tile, shape, K):
    return BF16_SHAPES[shape](*tile) + (K,) + tuple(tile) + (False,)


@functools.lru_cache(maxsize=None)
def _inputs_cpu(case):
    M, N, K, bm, bn, f32 = case
    dt = F32 if f32 else BF
    g = torch.Generator().manual_seed(((M * 1009 + N) * 1013 + K) * 4 + 2 * (bm == 256) + f32)
    A = torch.randn(M, K, generator=g).to(dt)
    B = torch.randn(K, N, generator=g).to(dt)
    bias = torch.randn(N, generator=g)
    bias[(torch.arange(N) // 8) % 2 == 1] -= 1.5  # half of the columns: a real share of exact zeros after the ReLU
    bias = bias.to(dt)
    aux = torch.randn(M, N, generator=g).to(BF)  # bf16 values: the bf16 and the f32 activation hold the same numbers
    edge = torch.tensor(MASK_EDGE * 2).to(BF)
    assert (edge.double() > 0).tolist() == [False, False, True, True] * 2
    # both sides of the tile boundary, a row inside the second tile, the last valid row / 8-column group
    rows = sorted({r for r in (0, bm - 1, bm, bm + 5, M - 1) if 0 <= r < M})
    cols = sorted({c for c in (0, bn - 8, bn, N - 8) if 0 <= c <= N - 8})
    for r in rows:
        for c in cols:
            aux[r, c:c + 8] = edge
    c_old = torch.randn(M, N, generator=g)
    Ad, Bd = A.double(), B.double()
    return dict(A=A, At=A.t().contiguous(), B=B, Bt=B.t().contiguous(), bias=bias, aux=aux, aux32=aux.float(),
                c_old=c_old, ab=Ad @ Bd, absprod=Ad.abs() @ Bd.abs(), colsum=Bd.sum(0), colabs=Bd.abs().sum(0))


@functools.lru_cache(maxsize=None)
def inputs(case, dev):
    """The inputs of one case and their float64 products: shared, never written."""
    return {k: v.to(dev) for k, v in _inputs_cpu(case).items()}


def _framed(t, cpad):
    """``t`` as a view into an allocation with 8 more rows and ``cpad`` more columns, all NaN."""
    tall = torch.full((t.shape[0] + 8, t.shape[1]), NAN, dtype=t.dtype, device=t.device)
    tall[:t.shape[0]] = t
    return _widen(tall, cpad)[:t.shape[0]]


@functools.lru_cache(maxsize=None)
def operand(case, dev, name, cpad):
    """A / At / B / Bt in its NaN frame (read-only, so shared between the calls of a case)."""
    return _framed(inputs(case, dev)[name], cpad)


@functools.lru_cache(maxsize=None)
def bias_of(case, dev):
    b = inputs(case, dev)["bias"]
    full = torch.full((b.numel() + 8,), NAN, dtype=b.dtype, device=dev)
    full[:b.numel()] = b
    return full[:b.numel()]


@functools.lru_cache(maxsize=None)
def aux_of(case, dev, bf16, cpad, col0):
    M, N = case[:2]
    full = torch.full((M + 8, N + cpad), NAN, dtype=BF if bf16 else F32, device=dev)
    view = full[:M, col0:col0 + N]
    view.copy_(inputs(case, dev)["aux"])
    return view


@functools.lru_cache(maxsize=None)
def expected(case, dev, epi, bf16, accumulate):
    """(ref64, bound, must_be_zero) of one epilogue."""
    inp = inputs(case, dev)
    ref, mag = inp["ab"], inp["absprod"]
    zero = None
    if epi in (G.EPI_BIAS, G.EPI_BIAS_RELU):
        ref = ref + inp["bias"].double()
        mag = mag + inp["bias"].double().abs()
    if epi == G.EPI_BIAS_RELU:
        zero = ref < -(2e-5 * mag + 1e-6)
        ref = torch.relu(ref)
    if epi == G.EPI_RELU_MASK:
        zero = ~(inp["aux"].double() > 0)
        ref = torch.where(zero, torch.zeros_like(ref), ref)
    if accumulate:
        ref = ref + inp["c_old"].double()
        mag = mag + inp["c_old"].double().abs()
    bound = 2e-5 * mag + 1e-6
    if bf16:
        bound = bound + HALF_ULP_BF16 * ref.abs()
    return ref, bound, zero


def run_gemm(dev, case, sk, a_t, b_t, spec, place=PLAIN, bf16=None):
    """One ``ops.gemm.gemm`` call of ``spec`` (``bf16`` overrides its output type: the f32 twin of a bf16 case).
    Returns (C view, C allocation, colsum view or None, colsum allocation or None)."""
    M, N, K, bm, bn, f32 = case
    inp = inputs(case, dev)
    bf16 = spec.bf16 if bf16 is None else bf16
    abpad, cpad, col0 = place
    A = operand(case, dev, "At" if a_t else "A", abpad)
    B = operand(case, dev, "Bt" if b_t else "B", abpad)
    full, C = _guarded(M, N, BF if bf16 else F32, dev, grow=8, pad=cpad, col0=col0)
    if spec.accumulate:
        C.copy_(inp["c_old"])
    kw = {}
    if spec.epi in (G.EPI_BIAS, G.EPI_BIAS_RELU):
        kw["bias"] = bias_of(case, dev)
    if spec.epi == G.EPI_RELU_MASK:
        kw["aux"] = aux_of(case, dev, bf16, cpad, col0)
    cs = csfull = None
    if spec.colsum:
        csfull = torch.full((N + 8,), SENT, device=dev)
        cs = csfull[:N]
        cs.fill_(NAN)
        kw["colsum"] = cs
    if place == STAGED:  # 8-byte but not 16-byte aligned: ops.gemm.gemm stages the bf16 output through a copy
        assert bf16 and not G._aligned16(C, kw.get("bias"), kw.get("aux"))
    G.gemm(A, a_t, B, b_t, C, spec.epi, accumulate=spec.accumulate, split_k=sk, tile=None if f32 else (bm, bn), **kw)
    return C, full, cs, csfull


def verify_gemm(dev, case, spec, C, full=None, cs=None, csfull=None, what=""):
    """The checks of one epilogue's output (``spec.bf16`` says which bound applies, whatever produced ``C``)."""
    inp = inputs(case, dev)
    ref, bound, zero = expected(case, dev, spec.epi, spec.bf16, spec.accumulate)
    _check(C, ref, bound, what)
    if zero is not None:
        nz = int((C[zero] != 0).sum())
        assert nz == 0, f"{what}: {nz} of {int(zero.sum())} masked / clamped elements are not exactly 0"
    if full is not None:
        _check_guard(full, C, what)
    if spec.colsum:
        _check(cs, inp["colsum"], 2e-5 * inp["colabs"] + 1e-6, what + " column sums")
        assert bool((csfull[cs.numel():] == SENT).all()), f"{what}: column sums written past the end"


def run_and_verify_gemm(dev, case, sk, a_t, b_t, spec, place=PLAIN, what=""):
    what = f"{what} M,N,K,bm,bn,f32={case} split_k={sk} a_t={a_t} b_t={b_t} {spec.name}"
    C, full, cs, csfull = run_gemm(dev, case, sk, a_t, b_t, spec, place)
    verify_gemm(dev, case, spec, C, full, cs, csfull, what)
    if spec.bf16:
        # the same plan with an f32 output, rounded by torch: "same arithmetic, element for element" (epi8_bf16)
        C32 = run_gemm(dev, case, sk, a_t, b_t, spec, place if place != STAGED else PLAIN, bf16=False)[0]
        same = C32.to(BF).contiguous().view(torch.int16) == C.contiguous().view(torch.int16)
        assert bool(same.all()), f"{what}: {int((~same).sum())} bf16 outputs differ from the rounded f32 output"


def all_bf16_epilogues(dev, tile, shape, ksplits=BF16_KSPLITS):
    for K, sk in ksplits:
        case = bf16_case(tile, shape, K)
        for place, name in ((PLAIN, "plain"), (PADDED, "padded")):
            for a_t, b_t in LAYOUTS:
                for spec in bf16_specs(a_t, b_t):
                    run_and_verify_gemm(dev, case, sk, a_t, b_t, spec, place, what=name)


def all_f32_epilogues(dev, MN):
    for K, sk in F32_SHAPES[MN]:
        case = MN + (K, 128, 128, True)
        for place, name in ((PLAIN, "plain"), (PADDED, "padded")):
            for a_t, b_t in LAYOUTS:
                for spec in F32_SPECS:
                    run_and_verify_gemm(dev, case, sk, a_t, b_t, spec, place, what=name)


SUBTILE = {tile: (8, 8, 8) + tile + (False,) for tile in BF16_TILES}


def subtile_bf16_epilogues(dev, tile):
    """M = N = K = 8: one 16-B chunk per operand row, everything else of the tile from the zero page."""
    for place, name in ((PLAIN, "plain"), (PADDED, "padded")):
        for a_t, b_t in LAYOUTS:
            for spec in bf16_specs(a_t, b_t):
                run_and_verify_gemm(dev, SUBTILE[tile], 1, a_t, b_t, spec, place, what=name)


def staged_bf16_case(dev):
    """A bf16 output (and activation) at column 4 — 8-byte, not 16-byte aligned — on a sliver shape."""
    case = bf16_case((256, 128), "sliver", 200)
    for name, a_t, b_t in (("bias_relu_bf16", False, False), ("relu_mask_bf16", False, True)):
        spec = next(s for s in T.SPECS if s.name == name)
        run_and_verify_gemm(dev, case, 2, a_t, b_t, spec, STAGED, what="staged")


def f32_colsum_case(dev, place=PADDED):
    """``colsum`` with f32 operands: the col_sum fallback inside ops.gemm.gemm, on a ragged N."""
    case = (136, 136, 104, 128, 128, True)
    spec = Spec("colsum_f32", G.EPI_NONE, False, False, True)
    for a_t, b_t in LAYOUTS:
        what = f"f32 colsum a_t={a_t} b_t={b_t}"
        verify_gemm(dev, case, spec, *run_gemm(dev, case, 2, a_t, b_t, spec, place), what=what)


@pytest.mark.parametrize("shape", list(BF16_SHAPES))
@pytest.mark.parametrize("tile", BF16_TILES)
def test_bf16_edge_tile_epilogues(C, tile, shape):
    """Every layout, epilogue, K split and placement of a forced tile on a shape that is not a multiple of it."""
    all_bf16_epilogues(DEV, tile, shape)


@pytest.mark.parametrize("tile", BF16_TILES)
def test_bf16_subtile_epilogues(C, tile):
    subtile_bf16_epilogues(DEV, tile)


def test_bf16_edge_staged_output(C):
    staged_bf16_case(DEV)


def test_bf16_224_row_tiles_have_no_edge_path(C):
    A = torch.zeros(232, 64, dtype=BF, device=DEV)
    B = torch.zeros(64, 128, dtype=BF, device=DEV)
    out = torch.zeros(232, 128, device=DEV)
    with pytest.raises(ValueError, match="unsupported"):
        G.gemm(A, False, B, False, out, tile=(224, 128))


@pytest.mark.parametrize("MN", list(F32_SHAPES))
def test_f32_gemm_epilogues(C, MN):
    """The f32 MFMA GEMM: every layout, epilogue (x accumulate), forced split and placement, aligned and edge shapes."""
    all_f32_epilogues(DEV, MN)


def test_f32_gemm_colsum_fallback(C):
    f32_colsum_case(DEV)


# ---------------------------------------------------------------------------------------------------------------
# 2. slab softmax on synthetic slabs

SLAB_M = T.SMX_M
SLAB_SPLITS = [1, 2, 3, 4, 5]  # 2 and 4: compile-time split counts; 1, 3, 5: the runtime-count instantiation
# 512-class chunks per row (NCH): 1, 1, 2 (one vector in the last chunk), 3 (partial last chunk), 4 (one vector in the
# last chunk), 4
SLAB_WIDTHS = [8, 512, 520, 1288, 1544, 2048]
SLAB_PADDED_WIDTHS = [520, 1544]  # also with ld, ldd > C
SLAB_SPECIAL_ROWS = (29, 30, 31, 32, 33, 36)  # all-equal, dominant at / away from the label, +1e4, -inf first / last


@functools.lru_cache(maxsize=None)
def _slab_inputs_cpu(Cc, sk):
    """ws [sk][M][C] f32 whose sum has the spread of the existing softmax inputs; in the special rows the whole value
    (minus the bias, so that sum + bias gives the special row back) sits in slab 0 and the other slabs are zero. The
    labels are the existing inputs': 0, C - 1, 7, 8, 511, 512 in the first rows."""
    base = T._softmax_inputs_cpu(Cc, False)
    g = torch.Generator().manual_seed(11 * Cc + sk)
    ws = torch.randn(sk, SLAB_M, Cc, generator=g) * 3 / sk ** 0.5
    bias = torch.randn(Cc, generator=g).to(BF)
    for r in SLAB_SPECIAL_ROWS:
        ws[1:, r] = 0.0
        ws[0, r] = base["x"][r] - bias.float()
    return dict(ws=ws.contiguous(), bias=bias, y=base["y"])


@functools.lru_cache(maxsize=None)
def slab_inputs(Cc, sk, dev):
    return {k: v.to(dev) for k, v in _slab_inputs_cpu(Cc, sk).items()}


def slab_logits(ws, bias, reverse=False):
    """torch's float32 ((s0 + s1) + ...) + bias: the split order of the kernel (``reverse``: the wrong order)."""
    order = list(range(ws.shape[0]))[::-1] if reverse else list(range(ws.shape[0]))
    acc = ws[order[0]].clone()
    for q in order[1:]:
        acc = acc + ws[q]
    return acc + bias.float()


def _bits_equal(a, b):
    return a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32) == \
        b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32)


def run_slabs(dev, Cc, sk, out_bf16, padded):
    """Returns [(view, allocation)] of logits, dlogits and loss."""
    inp = slab_inputs(Cc, sk, dev)
    pad, col0 = (16, 8) if padded else (0, 0)
    lgfull, lg = _guarded(SLAB_M, Cc, F32, dev, grow=3, pad=pad, col0=col0)
    dfull, d = _guarded(SLAB_M, Cc, BF if out_bf16 else F32, dev, grow=3, pad=pad, col0=col0)
    lfull = torch.full((SLAB_M + 3,), SENT, device=dev)
    loss = lfull[:SLAB_M]
    loss.fill_(NAN)
    NN.softmax_xent_slabs(dict(ws=inp["ws"], sk=sk), inp["bias"], lg, inp["y"], d, loss, T.SMX_GRAD_SCALE)
    return (lg, lgfull), (d, dfull), (loss, lfull)


def verify_slabs(dev, Cc, sk, out_bf16, padded, outs, what=""):
    inp = slab_inputs(Cc, sk, dev)
    (lg, lgfull), (d, dfull), (loss, lfull) = outs
    what = f"{what} slabs C={Cc} sk={sk} out={'bf16' if out_bf16 else 'f32'} padded={padded}"
    want = slab_logits(inp["ws"], inp["bias"])
    same = _bits_equal(lg, want)
    assert bool(same.all()), f"{what}: {int((~same).sum())} logits differ from the ordered float32 sum + bias"
    # the two-launch path on those logits, placed alike
    pad, col0 = (16, 8) if padded else (0, 0)
    xfull = torch.full((SLAB_M, Cc + pad), NAN, device=dev)
    x = xfull[:, col0:col0 + Cc]
    x.copy_(want)
    d2 = _guarded(SLAB_M, Cc, d.dtype, dev, grow=3, pad=pad, col0=col0)[1]
    loss2 = torch.full((SLAB_M,), NAN, device=dev)
    NN.softmax_xent(x, inp["y"], d2, loss2, T.SMX_GRAD_SCALE)
    assert bool(_bits_equal(loss, loss2).all()), f"{what}: loss rows differ from softmax_xent on the same logits"
    assert bool(_bits_equal(d, d2).all()), f"{what}: dlogits differ from softmax_xent on the same logits"
    T.verify_softmax(dev, Cc, False, out_bf16, d, dfull, loss, lfull, r=SMX_R, what=what,
                     inp=T.softmax_reference(want, inp["y"]))
    _check_guard(lgfull, lg, what + " logits")


def all_slab_cases(dev, Cc, sk):
    for padded in (False, True) if Cc in SLAB_PADDED_WIDTHS else (False,):
        for out_bf16 in (False, True):
            verify_slabs(dev, Cc, sk, out_bf16, padded, run_slabs(dev, Cc, sk, out_bf16, padded))


def slab_refusals(dev):
    """C > 2048, C % 8 != 0 and a workspace that does not hold sk slabs raise."""
    for Cc, sk, short in ((2056, 2, 0), (12, 2, 0), (512, 3, 1)):
        ws = torch.zeros(sk - short, SLAB_M, Cc, device=dev)
        bias = torch.zeros(Cc, dtype=BF, device=dev)
        lg = torch.zeros(SLAB_M, Cc, device=dev)
        d = torch.zeros(SLAB_M, Cc, device=dev)
        loss = torch.zeros(SLAB_M, device=dev)
        y = torch.zeros(SLAB_M, dtype=torch.int32, device=dev)
        with pytest.raises((RuntimeError, ValueError)):
            NN.softmax_xent_slabs(dict(ws=ws, sk=sk), bias, lg, y, d, loss, 1.0)


@pytest.mark.parametrize("sk", SLAB_SPLITS)
@pytest.mark.parametrize("Cc", SLAB_WIDTHS)
def test_slab_softmax_on_synthetic_slabs(C, Cc, sk):
    all_slab_cases(DEV, Cc, sk)


def test_slab_softmax_refusals(C):
    slab_refusals(DEV)


# ---------------------------------------------------------------------------------------------------------------
# 3. wire epilogue on edge tiles (bwd-weight layout, N % 16 == 0)

WIRE_TILES = [(256, 256), (256, 128), (128, 128)]
WIRE_KSPLITS = [(200, 1), (200, 2), (312, 4)]
WIRE_SHAPES = {"sliver": lambda bm, bn: (bm + 8, bn + 16), "almost": lambda bm, bn: (2 * bm - 8, 2 * bn - 16)}
WIRE_OFF, WIRE_POST, WIRE_SHARDS, WIRE_OWN = 48, 32, 3, 1
WIRE_FILL = 0xA5


def _wire_case(tile, shape, K):
    return WIRE_SHAPES[shape](*tile) + (K,) + tuple(tile) + (False,)


def _plan_reference(case, sk):
    """The same plan's f32 EPI_NONE output (what part 1 holds to the fp64 bound)."""
    M, N, K, bm, bn, _ = case
    ref = torch.full((M, N), NAN, device=DEV)
    G.gemm(operand(case, DEV, "At", 64), True, operand(case, DEV, "B", 64), False, ref, G.EPI_NONE, split_k=sk,
           tile=(bm, bn))
    return ref


@pytest.mark.parametrize("shape", list(WIRE_SHAPES))
@pytest.mark.parametrize("tile", WIRE_TILES)
def test_wire_epilogue_on_edge_tiles(C, tile, shape):
    """The BFP wire epilogue (in-kernel and through the split-K wire reduce over a ragged K) with the fused bias
    gradient on an edge tile: W bytes equal the oracle's pack of the same plan's f32 output, the bias segment decodes
    to the kernel's own f32 column sums within one quantisation step (2^-6 of its group's largest magnitude: both
    8-bit codecs scale a group by 2^(133 - E) with max|x| >= 2^(E - 127), and drop at most one unit), the owner shard
    arrives in f32 and nothing else of the bucket or the wire buffer is written."""
    for K, sk in WIRE_KSPLITS:
        case = _wire_case(tile, shape, K)
        M, N = case[:2]
        inp = inputs(case, DEV)
        ref = _plan_reference(case, sk)
        n = WIRE_OFF + M * N + N + WIRE_POST
        shard = (-(-n // WIRE_SHARDS) + 255) // 256 * 256
        lo_w, hi_w, hi_b = WIRE_OFF, WIRE_OFF + M * N, WIRE_OFF + M * N + N
        assert shard < hi_w - lo_w, "the owner shard lies inside W"
        for codec in ("bfp_rne", "bfp_trunc"):
            what = f"wire {codec} M,N,K,bm,bn={case[:5]} split_k={sk}"
            sb = wire.shard_bytes(codec, shard)
            g = torch.full((shard * WIRE_SHARDS,), SENT, device=DEV)
            buf = torch.full((WIRE_SHARDS * sb,), WIRE_FILL, dtype=torch.uint8, device=DEV)
            G.gemm(operand(case, DEV, "At", 64), True, operand(case, DEV, "B", 64), False,
                   g[lo_w:hi_w].view(M, N), G.EPI_WIRE, colsum=g[hi_w:hi_b],
                   wire=(buf, shard, WIRE_OWN, wire.codec_id(codec), 0, WIRE_OFF), split_k=sk, tile=tile)
            torch.cuda.synchronize()
            flat = np.zeros(shard * WIRE_SHARDS, np.float32)
            flat[lo_w:hi_w] = ref.cpu().numpy().reshape(-1)
            exp = O.pack(flat, shard, codec)
            got = buf.cpu().numpy()
            touched = np.zeros(got.size, bool)
            for s in range(WIRE_SHARDS):
                for lo, hi, is_w in ((lo_w, hi_w, True), (hi_w, hi_b, False)):
                    a, b = max(s * shard, lo) - s * shard, min((s + 1) * shard, hi) - s * shard
                    if b <= a:
                        continue
                    mant = slice(s * sb + a, s * sb + b)
                    expo = slice(s * sb + shard + a // 16, s * sb + shard + b // 16)
                    touched[mant] = touched[expo] = True
                    if is_w:
                        assert np.array_equal(got[mant], exp[mant]), f"{what}: shard {s}: W mantissas differ"
                        assert np.array_equal(got[expo], exp[expo]), f"{what}: shard {s}: W exponents differ"
            assert (got[~touched] == WIRE_FILL).all(), f"{what}: wire bytes outside [W | b] written"
            # the bucket: the fused bias gradient in f32, the owner shard of W in f32, everything else untouched
            gh = g.cpu()
            cs = gh[hi_w:hi_b]
            _check(cs, inp["colsum"].cpu(), 2e-5 * inp["colabs"].cpu() + 1e-6, what + " column sums")
            own = torch.zeros(gh.numel(), dtype=torch.bool)
            own[max(lo_w, WIRE_OWN * shard):min(hi_w, (WIRE_OWN + 1) * shard)] = True
            assert torch.equal(gh[own], ref.cpu().reshape(-1)[own[lo_w:hi_w]]), f"{what}: owner shard differs"
            own[hi_w:hi_b] = True
            assert bool((gh[~own] == SENT).all()), f"{what}: wrote the bucket outside the owner shard and the bias"
            dec = torch.from_numpy(O.unpack(got, shard * WIRE_SHARDS, shard, codec)[hi_w:hi_b].copy()).double()
            step = 2.0 ** -6 * cs.abs().view(-1, 16).max(1, keepdim=True)[0].expand(-1, 16).reshape(-1).double()
            _check(dec, cs.double(), step, what + " decoded bias segment")


@pytest.mark.parametrize("tile", WIRE_TILES)
def test_fused_update_on_edge_tiles(C, tile):
    """The fused local update on an edge tile (sliver shape) against the engine's decode + SGD kernel run on the
    wire the same plan stores: master, bf16 copy and momentum bit-identical, no wire stored."""
    rne = wire.codec_id("bfp_rne")
    opt = dict(lr=0.02, weight_decay=1e-3, momentum=0.9)
    for K, sk in WIRE_KSPLITS:
        case = _wire_case(tile, "sliver", K)
        M, N = case[:2]
        what = f"fused update M,N,K,bm,bn={case[:5]} split_k={sk}"
        x, dz = operand(case, DEV, "At", 64), operand(case, DEV, "B", 64)
        n = M * N + N
        n_pad = (n + 255) // 256 * 256
        gen = torch.Generator().manual_seed(7)
        m0 = ((torch.rand(n_pad, generator=gen) * 2 - 1) * 0.05).to(DEV)
        mm0 = ((torch.rand(n_pad, generator=gen) * 2 - 1) * 0.01).to(DEV)
        l0 = m0.to(BF)
        grad = torch.zeros(n_pad, device=DEV)
        buf = torch.zeros(wire.shard_bytes("bfp_rne", n_pad), dtype=torch.uint8, device=DEV)
        G.gemm(x, True, dz, False, grad[:M * N].view(M, N), G.EPI_WIRE, colsum=grad[M * N:n],
               wire=(buf, n_pad, -1, rne), split_k=sk, tile=tile)
        m_ref, l_ref, mm_ref = m0.clone(), l0.clone(), mm0.clone()
        wire.sgd(buf, n_pad, 1, m_ref, codec="bfp_rne", lp=l_ref, mom=mm_ref, n_valid=n, **opt)
        m_f, l_f, mm_f = m0.clone(), l0.clone(), mm0.clone()
        grad2 = torch.zeros(n_pad, device=DEV)
        buf2 = torch.zeros_like(buf)
        G.gemm(x, True, dz, False, grad2[:M * N].view(M, N), G.EPI_WIRE, colsum=grad2[M * N:n],
               wire=(buf2, n_pad, -1, rne), update=G.LocalUpdate(m_f, l_f, mm_f, **opt), split_k=sk, tile=tile)
        torch.cuda.synchronize()
        assert torch.equal(m_f, m_ref), f"{what}: master differs: {(m_f - m_ref).abs().max().item()}"
        assert torch.equal(l_f, l_ref), f"{what}: bf16 copy differs"
        assert torch.equal(mm_f, mm_ref), f"{what}: momentum differs"
        assert bool((buf2 == 0).all()), f"{what}: the fused update stores no wire"
        assert not torch.equal(m_f[:n], m0[:n]), f"{what}: weights not updated"
        assert torch.equal(m_f[n:], m0[n:]), f"{what}: the padding past [W | b] was updated"
