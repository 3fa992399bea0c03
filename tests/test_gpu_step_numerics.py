"""One training step of ``DataParallelTrainer`` at the shapes and model flags that switch its dispatch, each against
an independent reference (tests/test_gpu_e2e_numerics.py does this at the flagship shape alone; this file generalises
its two references and leaves it as it is).

The reference (``reference_step``) is the HIP step's arithmetic in torch: every GEMM summed in float64 and rounded to
float32 (so its summation order is not the trainer's, on either device), rounded to bf16 exactly where the HIP step
rounds (activations after bias + ReLU, the softmax gradient, each dZ after its mask; an f32 model rounds nowhere), the
ReLU wherever ``MLP._relu_at`` puts it (the classifier's too), each flat ``[dW | db]`` bucket zero-padded to a multiple
of 16 and taken through ``bfp_oracle.quantize(.., "bfp_rne")``, the update through ``bfp_oracle.sgd`` with a momentum
plane of the reference's own. With ``relu="all"`` the classifier's mask is the device's (``m.logits > 0``): those logits
are checked per element, and a logit that changes sign under another summation order moves a whole dZ element.
A hidden ReLU's backward mask is the reference's own (z > 0) except at the elements whose pre-activation lies within
the GEMM bound of zero, |z| <= 2e-5 * (|h| @ |w| + |b|) + 1e-6: there the sign is not determined at the precision the
GEMM is held to by (a), and the reference takes the device's (``m.act[i] > 0``), for the same reason. At batch 4096 and
K = 4096 (``wgrad_group``) some hundred of the 1.7e7 pre-activations of a layer change sign between two summation
orders; each moves one of a column's 4096 terms, and with the reference's own mask 3856 elements of layer 1's update
missed (e), the worst by 8.9 steps, while every by-norm check passed. A mask that is wrong anywhere else still fails.

Per step, from the model's current compute weights (``check_step``):
(a) activations and logits per element against the float64 product of the device's own rounded operands,
    2e-5 * (|h| @ |w| + |b|) + 1e-6 (+ 2^-8 |ref| for a bf16 output): the project's GEMM bound; read after ``step``;
(b) loss rows against the float64 cross-entropy of the device's logits, SMX_R / SMX_A of test_gpu_epilogue_numerics.py;
(c) mean loss against the reference's, EMUL_LOSS;
(d) update by norm, the weight and the bias segment of each layer separately, EMUL_BOUND (a bias segment is a few
    per cent of its layer's norm and must not hide inside it);
(e) update per element, no exclusions: |d_hip - d_ref| <= lr * 2 * 2^-6 * max|g|_group + 2^-23 |w|: two worst-case
    BFP-rne steps (one step is 2^(E-133) <= 2^-6 max|group|, test_gpu_e2e_numerics.py) plus the f32 master's ulp; one
    step for an element another summation order moves across a rounding boundary, one for a group whose maximum
    crosses a binade;
(f) state: lp == bf16(master) bit for bit, the masters' and the momentum planes' padding still zero;
(g) against fp32 autograd (hidden or no ReLU only), FP32_BOUND.
Each case first asserts the route it is named for (plans from ``C.gemm_plan``, the trainer's counters, which softmax
ran), with the tuner off so that the static planner decides.

The split-K classifier wider than the folding softmax takes (``wide_fold``, C = 2176 > 2048) raised on every step
before ops/gemm.py asked ``softmax_xent_slabs_supported``; it now keeps the GEMM's own slab reduce, bit-identical to
``fold_logits = False``.

Measured on an MI355X (worst over the steps; (e) in worst-case BFP steps, bound 2; wall time of the test):
  case            (d) weight  (d) bias  (e)    (g)      wall     masks taken from the device (differing)
  wide_fold       2.2e-4      0         0.98   0.0115   1.99 s   84 (0)     (the module's first test: start-up included)
  ragged_fold     2.4e-4      0         1.00   0.0119   0.11 s   151 (0)
  mixed_prepack   2.5e-4      0         0.98   0.0119   0.10 s   157 (0)
  ragged_rows     9.6e-4      0         0.99   0.0328   0.04 s   298 (0)
  fuse0 .. fuse3  <= 3.0e-4   0         0.98   0.0087   0.03 s   <= 81 (0)  ((g) for fuse0, fuse1 only)
  momentum        2.1e-4      0         1.81   0.0093   0.03 s   85 (0)     (Nesterov: a step of g is 1.9 of the update's)
  f32_model       1.2e-4      0         0.92   0.0086   0.03 s   66 (0)
  wgrad_group     2.4e-3      2.5e-3    1.00   0.0334   1.74 s   29914 (66)
  wide_fold bit-identical to fold_logits = False: 0.04 s. With the width condition of ops/gemm.py switched off (the
  parent's behaviour) ``wide_fold`` raises "softmax_xent over split-K slabs: C % 8 == 0, C <= 2048, ..." on step 1.
The same cases on the CPU fallbacks (tests/test_step_numerics_cpu.py): (d) <= 9.6e-4, (e) <= 1.00 (momentum 1.89),
(g) <= 0.0328.
"""
import collections
import contextlib
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_e2e_numerics as E2E
import test_gpu_epilogue_numerics as T
from fpga_ai_nic_amd.ops import gemm_tune
from fpga_ai_nic_amd.ops import nn as NN

pytestmark = pytest.mark.gpu

LR = E2E.LR
EMUL_BOUND, EMUL_LOSS, FP32_BOUND = E2E.EMUL_BOUND, E2E.EMUL_LOSS, E2E.FP32_BOUND
GEMM_R, GEMM_A = 2e-5, 1e-6          # the project's per-element GEMM bound (test_gpu_epilogue_numerics.py)
BFP_STEP = 2.0 ** -6                  # one BFP-rne step <= 2^-6 max|group|
ELEM_STEPS = 2                        # (e): two worst-case steps
F32_ULP = 2.0 ** -23

Case = collections.namedtuple("Case", "name sizes mb dtype bias relu momentum nesterov weight_decay steps",
                              defaults=(torch.bfloat16, True, "hidden", 0.0, False, 0.0, 3))
CASES = {c.name: c for c in [
    Case("wide_fold", [256, 1024, 2176], 128),
    Case("ragged_fold", [1000, 1000, 1000], 128),
    Case("mixed_prepack", [1000, 1008, 1000], 128),
    Case("ragged_rows", [512, 256, 1024, 16], 448),
    Case("fuse0", [256, 512, 256], 256, bias=False, relu="none"),
    Case("fuse1", [256, 512, 256], 256, bias=True, relu="none"),
    Case("fuse2", [256, 512, 256], 256, bias=False, relu="all"),
    Case("fuse3", [256, 512, 256], 256, bias=True, relu="all"),
    Case("momentum", [256, 512, 256], 256, momentum=0.9, nesterov=True, weight_decay=1e-4),
    Case("f32_model", [264, 520, 264, 40], 136, dtype=torch.float32),
    Case("wgrad_group", [1024, 4096, 4096, 1024], 4096, steps=2),
]}


@pytest.fixture(scope="module", autouse=True)
def _static_plans():
    """The static planner decides every plan of this module, so each case's route is determined."""
    gemm_tune.reset(enabled=False)
    yield
    gemm_tune.reset()


def _relu_at(case, i):
    L = len(case.sizes) - 1
    return case.relu == "all" or (case.relu == "hidden" and i + 1 < L)


def _rnd(case, t):
    return t.to(torch.bfloat16).float() if case.dtype == torch.bfloat16 else t


def _mm(a, b):
    """a @ b summed in float64, rounded once to float32."""
    return (a.double() @ b.double()).float()


# ---------------------------------------------------------------------------------------------------------------
# the references


def reference_step(case, W, b, x, y, cls_mask=None, dev_act=None, info=None):
    """The HIP step's arithmetic from compute weights (W, b) (float32 values): (loss rows, per-layer flat gradient
    [dW | db], float32). ``cls_mask``: the classifier's ReLU mask (``relu="all"``). ``dev_act``: the device's
    activations, from which a hidden ReLU's backward mask is taken at the elements whose pre-activation lies within
    the GEMM bound of zero (see the module docstring); ``info["adopted"]`` counts them, ``info["flipped"]`` those where
    the two masks differ."""
    L, mb = len(W), x.shape[0]
    act, mask = [x.float()], [None] * (L + 1)
    for i in range(L):
        z = _mm(act[i], W[i]) + b[i]
        if _relu_at(case, i):
            if i + 1 < L:
                mask[i + 1] = z > 0
                if dev_act is not None:
                    near = z.abs() <= GEMM_R * _mm(act[i].abs(), W[i].abs()) + GEMM_R * b[i].abs() + GEMM_A
                    theirs = dev_act[i + 1] > 0
                    if info is not None:
                        info["adopted"] += int(near.sum())
                        info["flipped"] += int((near & (theirs != mask[i + 1])).sum())
                    mask[i + 1] = torch.where(near, theirs, mask[i + 1])
            z = torch.relu(z)
        act.append(_rnd(case, z) if i + 1 < L else z)  # logits stay f32
    logits = act[L]
    loss_rows = F.cross_entropy(logits, y.long(), reduction="none")
    p = torch.softmax(logits, dim=1)
    p[torch.arange(mb, device=x.device), y.long()] -= 1.0
    dz = _rnd(case, p * (1.0 / mb))
    if _relu_at(case, L - 1):
        dz = dz * cls_mask
    grads = [None] * L
    for i in reversed(range(L)):
        dW = _mm(act[i].t(), dz)
        db = dz.double().sum(0).float() if case.bias else torch.zeros_like(b[i])
        grads[i] = torch.cat([dW.flatten(), db])
        if i > 0:
            dx = _mm(dz, W[i].t())
            dz = _rnd(case, dx * mask[i] if _relu_at(case, i - 1) else dx)
    return loss_rows, grads


def autograd_step(case, W, b, x, y):
    """Plain fp32 autograd from the same weights: (loss, per-layer flat gradient [dW | db])."""
    Ws = [w.clone().requires_grad_(True) for w in W]
    bs = [v.clone().requires_grad_(True) for v in b]
    h = x.float()
    for i in range(len(Ws)):
        h = h @ Ws[i] + bs[i]
        if _relu_at(case, i):
            h = torch.relu(h)
    loss = F.cross_entropy(h, y.long())
    gs = torch.autograd.grad(loss, Ws + bs)
    L = len(Ws)
    return float(loss.detach()), [torch.cat([gs[i].flatten(), gs[L + i] if case.bias else torch.zeros_like(b[i])])
                                  for i in range(L)]


class RefOptimizer:
    """SGD by ``bfp_oracle.sgd`` with momentum planes of its own, one per layer."""

    def __init__(self, case, L):
        self.case, self.mom = case, [None] * L

    def update(self, i, w, g, quantize):
        """(new weights, the per-element max|g| of each element's 16-value group) from float32 numpy w, g [n]."""
        from fpga_ai_nic_amd.ops import bfp_oracle as O

        c, n = self.case, g.size
        g16 = np.zeros(-(-n // 16) * 16, np.float32)
        g16[:n] = g
        gmax = np.repeat(np.abs(g16).reshape(-1, 16).max(1), 16)[:n]
        q = O.quantize(g16, "bfp_rne")[:n] if quantize else g
        if c.momentum and self.mom[i] is None:
            self.mom[i] = np.zeros(n, np.float32)
        w2, m2 = O.sgd(w, q, LR, 1.0, c.weight_decay, c.momentum, self.mom[i], c.nesterov)
        self.mom[i] = m2
        return w2, gmax


# ---------------------------------------------------------------------------------------------------------------
# the trainer under test


def make_trainer(device, case):
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    dev = torch.device(device)
    eng = make_engine(ThreadFabric(1).transport(0), "bfp", rounding="rne",
                      impl="native" if dev.type == "cuda" else "python", device=dev)
    m = MLP(case.sizes, dtype=case.dtype, device=dev, seed=7, pad_fn=lambda n: eng.layout(n).n_pad,
            momentum=bool(case.momentum), bias=case.bias, relu=case.relu)
    tr = DataParallelTrainer(m, eng, lr=LR, momentum=case.momentum, nesterov=case.nesterov,
                             weight_decay=case.weight_decay)
    if case.dtype == torch.bfloat16:
        for l in m.layers:  # the f32 masters start at the bf16 values the forward computes with
            l.master[: l.n].copy_(l.lp[: l.n].float())
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(case.mb, case.sizes[0], generator=g) * 2 - 1).to(dev, case.dtype)
    y = torch.randint(0, case.sizes[-1], (case.mb,), generator=g, dtype=torch.int32).to(dev)
    return m, tr, x, y


@contextlib.contextmanager
def count_calls(counts):
    """Count which loss / reduction entry points of ops/nn.py the model calls (it calls them as ``NN.<name>``)."""
    names = ("softmax_xent", "softmax_xent_slabs", "col_sum")
    saved = {k: getattr(NN, k) for k in names}

    def wrap(k):
        def f(*a, **kw):
            counts[k] += 1
            return saved[k](*a, **kw)
        return f

    for k in names:
        setattr(NN, k, wrap(k))
    try:
        yield
    finally:
        for k in names:
            setattr(NN, k, saved[k])


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _rel(err, ref):
    """||err|| / ||ref||; a reference segment that is exactly zero (a bias-free model's) admits no error at all."""
    e, r = float(err.norm()), float(ref.norm())
    return e / r if r > 0 else (0.0 if e == 0 else float("inf"))


def check_step(case, m, snap, ref, stats, what):
    """Checks (a) .. (g) of one step. ``snap``: the planes before the step; ``ref``: the references' results."""
    L, dev = m.L, m.device
    Wl, bl = snap["W"], snap["b"]
    # (a) every layer's output against the float64 product of the device's own operands
    for i in range(L):
        h, out = m.act[i].double(), (m.act[i + 1] if i + 1 < L else m.logits)
        want = h @ Wl[i].double() + bl[i].double()
        bound = GEMM_R * (h.abs() @ Wl[i].double().abs() + bl[i].double().abs()) + GEMM_A
        if _relu_at(case, i):
            want = torch.relu(want)
        if out.dtype == torch.bfloat16:
            bound = bound + T.HALF_ULP_BF16 * want.abs()
        T._check(out, want, bound, f"{what} (a) " + (f"layer {i} activations" if i + 1 < L else "logits"))
    # (b) loss rows against the float64 cross-entropy of the device's logits
    sm = T.softmax_reference(m.logits, snap["y"])
    T._check(m.loss_rows, sm["loss"], T.SMX_R * sm["loss"].abs() + T.SMX_A * sm["loss_scale"], f"{what} (b) loss rows")
    # (c) mean loss against the reference's
    hl, el = float(m.loss_rows.double().mean()), float(ref["loss_rows"].double().mean())
    stats["loss"].append(abs(hl - el) / el)
    assert stats["loss"][-1] <= EMUL_LOSS, f"{what} (c) mean loss {hl!r} vs the reference's {el!r}"
    for i, l in enumerate(m.layers):
        k = l.cin * l.cout
        d_hip = l.master[: l.n].double() - snap["master"][i][: l.n].double()
        d_ref = torch.from_numpy(ref["w_new"][i].astype(np.float64)).to(dev) - snap["master"][i][: l.n].double()
        # (d) by norm, per segment
        for name, sl in (("weight", slice(0, k)), ("bias", slice(k, l.n))):
            r = _rel(d_hip[sl] - d_ref[sl], d_ref[sl])
            stats[name].append(r)
            assert r <= EMUL_BOUND, f"{what} (d) layer {i} {name} segment: update off by {r:.3e} of its norm"
        # (e) per element
        gmax = torch.from_numpy(ref["gmax"][i].astype(np.float64)).to(dev)
        err = (d_hip - d_ref).abs()
        unit, ulp = LR * BFP_STEP * gmax, F32_ULP * snap["master"][i][: l.n].double().abs()
        bound = ELEM_STEPS * unit + ulp
        over = (err - ulp).clamp(min=0)  # measured in worst-case steps of the element's group (an all-zero group: 0)
        inf = torch.full_like(over, float("inf"))
        stats["elem"].append(float(torch.where(unit > 0, over / unit, torch.where(over > 0, inf, 0 * over)).max()))
        bad = (err > bound) | ~torch.isfinite(d_hip)
        if bool(bad.any()):
            j = int((err - bound).argmax())
            raise AssertionError(f"{what} (e) layer {i} update per element: {int(bad.sum())} of {bad.numel()} out of "
                                 f"bound, worst at flat index {j} ({'weight' if j < k else 'bias'}): "
                                 f"{float(d_hip[j])!r} vs {float(d_ref[j])!r}, bound {float(bound[j]):.3g}")
        # (f) state
        if l.lp is not None:
            same = l.lp[: l.n].view(torch.int16) == l.master[: l.n].to(torch.bfloat16).view(torch.int16)
            assert bool(same.all()), (f"{what} (f) layer {i}: lp is not bf16(master) at {int((~same).sum())} "
                                      f"elements")
            assert not bool((l.lp[l.n:] != 0).any()), f"{what} (f) layer {i}: lp padding not zero"
        assert not bool((l.master[l.n: l.n_pad] != 0).any()), f"{what} (f) layer {i}: master padding not zero"
        if l.mom is not None:
            assert not bool((l.mom[l.n:] != 0).any()), f"{what} (f) layer {i}: momentum padding not zero"
        # (g) against fp32 autograd
        if case.relu != "all":
            d_fp = torch.from_numpy(ref["w_fp32"][i].astype(np.float64)).to(dev) - snap["master"][i][: l.n].double()
            r = _rel(d_hip - d_fp, d_fp)
            stats["fp32"].append(r)
            assert r <= FP32_BOUND, f"{what} (g) layer {i}: update off fp32 autograd's by {r:.4f} of its norm"


def run_case(device, case, steps=None, tamper=None, before=None):
    """Train ``case`` for ``steps`` steps on ``device`` ('cuda' or 'cpu'), each step through every check; returns the
    measured worst values, the trainer and the call counts. ``before(tr)``: adjust the trainer first. ``tamper(step,
    m, snap, prev)``: alter the model's state after a step, before it is checked (``prev``: the step before's
    logits) — the planted mistakes of tests/test_step_numerics_cpu.py."""
    steps = case.steps if steps is None else steps
    m, tr, x, y = make_trainer(device, case)
    if before is not None:
        before(tr)
    dev = m.device
    opt, opt32 = RefOptimizer(case, m.L), RefOptimizer(case, m.L)
    stats = collections.defaultdict(list)
    counts = collections.Counter()
    prev = None
    t0 = time.perf_counter()
    with count_calls(counts):
        for s in range(steps):
            snap = dict(W=[l.w.float().clone() for l in m.layers], b=[l.b.float().clone() for l in m.layers],
                        master=[l.master.clone() for l in m.layers], y=y)
            tr.step(x, y)
            tr.finish()
            _sync(dev)
            mask = (m.logits > 0) if _relu_at(case, m.L - 1) else None
            loss_rows, grads = reference_step(case, snap["W"], snap["b"], x, y, mask, dev_act=m.act, info=counts)
            ref = dict(loss_rows=loss_rows, w_new=[], gmax=[], w_fp32=[])
            g32 = autograd_step(case, snap["W"], snap["b"], x, y)[1] if case.relu != "all" else None
            for i, l in enumerate(m.layers):
                w = snap["master"][i][: l.n].cpu().numpy()
                w2, gmax = opt.update(i, w, grads[i].cpu().numpy(), quantize=True)
                ref["w_new"].append(w2)
                ref["gmax"].append(gmax)
                if g32 is not None:
                    ref["w_fp32"].append(opt32.update(i, w, g32[i].cpu().numpy(), quantize=False)[0])
            logits = m.logits.clone()
            if tamper is not None:
                tamper(s, m, snap, prev)
            prev = logits
            check_step(case, m, snap, ref, stats, f"{case.name} step {s}")
    worst = {k: max(v) for k, v in stats.items()}
    print(f"\n{case.name} on {dev.type}: {steps} steps in {time.perf_counter() - t0:.2f} s; vs the emulating "
          f"reference: weight segments {['%.2e' % v for v in stats['weight']]}, bias segments "
          f"{['%.2e' % v for v in stats['bias']]}, mean loss {['%.1e' % v for v in stats['loss']]}, per element "
          f"{['%.2f' % v for v in stats['elem']]} worst-case BFP steps; vs fp32 autograd "
          f"{['%.4f' % v for v in stats['fp32']]}; calls {dict(counts)}")
    return dict(worst=worst, tr=tr, m=m, counts=counts, steps=steps)


# ---------------------------------------------------------------------------------------------------------------
# the cases, each with its route


def _classifier_plan(C, case):
    return tuple(C.gemm_plan(case.mb, case.sizes[-1], case.sizes[-2], 0, 0, 0, 0))


def test_wide_fold(C):
    """A split-K classifier wider than the folding softmax takes keeps the GEMM's slab reduce."""
    case = CASES["wide_fold"]
    plan = _classifier_plan(C, case)
    assert plan[2] > 1 and case.sizes[-1] > 2048, plan
    assert not NN.softmax_xent_slabs_supported(case.sizes[-1]) and not C.softmax_xent_slabs_supported(case.sizes[-1])
    r = run_case("cuda", case)
    assert r["tr"].fold_logits, "the default: a split-K classifier folds where the softmax takes it"
    assert r["counts"]["softmax_xent_slabs"] == 0 and r["counts"]["softmax_xent"] == r["steps"], r["counts"]


def test_wide_fold_bit_identical_to_unfolded():
    """(tests/test_gpu_fold_logits.py test_trainer_fold_logits_bit_identical at the width the softmax cannot fold)"""
    case, res = CASES["wide_fold"], []
    for fold in (False, True):
        m, tr, x, y = make_trainer("cuda", case)
        tr.fold_logits = fold
        for _ in range(case.steps):
            tr.step(x, y)
        tr.finish()
        res.append((m.logits.cpu(), m.loss_rows.cpu(), [(l.master.cpu(), l.lp.cpu()) for l in m.layers]))
    assert torch.equal(res[0][0], res[1][0]), "logits differ"
    assert torch.equal(res[0][1], res[1][1]), "loss rows differ"
    for a, b in zip(res[0][2], res[1][2]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ragged_fold(C):
    """Ragged widths: the classifier's ragged split-K plan folded by the slab softmax at C = 1000; no layer has a
    prepack target, so every update goes bwd-weight GEMM -> engine."""
    case = CASES["ragged_fold"]
    assert _classifier_plan(C, case)[2] == 2, _classifier_plan(C, case)
    r = run_case("cuda", case)
    assert r["counts"]["softmax_xent_slabs"] == r["steps"] and r["counts"]["softmax_xent"] == 0, r["counts"]
    assert r["tr"].prepack and r["tr"].fused_updates == 0


def test_mixed_prepack():
    """Layer 0 (1008 outputs) takes the fused update, layer 1 (1000) goes through the engine, in one backward."""
    r = run_case("cuda", CASES["mixed_prepack"])
    assert r["tr"].fused_update and r["tr"].fused_updates == r["steps"]


def test_ragged_rows():
    """A batch that is no tile multiple and a 16-class head."""
    r = run_case("cuda", CASES["ragged_rows"])
    assert r["tr"].prepack and r["tr"].fused_update


@pytest.mark.parametrize("name", ["fuse0", "fuse1", "fuse2", "fuse3"])
def test_fuse_types(name):
    """The reference's four fuse types: (bias, relu) = (F, none), (T, none), (F, all), (T, all)."""
    case = CASES[name]
    r = run_case("cuda", case)
    assert r["tr"].fused_update and r["tr"].fused_updates == r["steps"] * r["m"].L
    if case.relu == "all":  # a ReLU on the classifier: its epilogue is not the one the softmax folds
        assert r["counts"]["softmax_xent_slabs"] == 0 and r["counts"]["softmax_xent"] == r["steps"], r["counts"]


def test_momentum():
    """Momentum, Nesterov and weight decay inside the GEMM-fused LocalUpdate."""
    case = CASES["momentum"]
    r = run_case("cuda", case)
    assert r["tr"].fused_update and r["tr"].fused_updates == r["steps"] * r["m"].L
    assert all(l.mom is not None and bool(l.mom.any()) for l in r["m"].layers)


def test_f32_model():
    """gemm_f32 and the standalone col_sum."""
    case = CASES["f32_model"]
    r = run_case("cuda", case)
    assert not r["tr"].prepack and r["tr"].fused_updates == 0
    assert r["counts"]["col_sum"] == r["steps"] * r["m"].L, r["counts"]


def test_wgrad_group():
    """The grouped split-K bwd-weight launch (it needs K / s >= 1024: batch 4096 at the flagship widths)."""
    case = CASES["wgrad_group"]
    r = run_case("cuda", case)
    assert r["tr"].wgrad_groups == r["steps"], r["tr"].wgrad_groups
    assert r["tr"].fused_updates == r["steps"] * r["m"].L
