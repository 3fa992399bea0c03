"""Grouped split-K bwd-weight launch (csrc/gemm/gemm_group.hip launch_gemm_wgrad_splitk_group) and the trainer
schedule built on it (DataParallelTrainer wgrad_pair).

Several wire bwd-weight GEMMs on 256x256 tiles run as ONE dispatch at a common split-K count and ONE slab reduce
(splitk_reduce_wire4_group_kernel), which also carries the bias-gradient reduces queued on the stream. Every workgroup
runs the single launch's (tile, split) unit and every value takes the single reduce's operations in its order, so:

* op level: every output plane (wire bytes / f32 dW, or master, bf16 copy, momentum; the bias gradient) is
  BIT-IDENTICAL to the same GEMMs launched one at a time with ``tile=(256, 256), split_k=s``; and dW / db stay inside
  the per-element fp64 bound tests/test_gpu_kernels.py uses for split-K GEMMs (2e-5 * sum_k |a b| + 1e-6);
* trainer level ([1024, 4096, 4096, 1024] at 4096 rows, the smallest batch at which the rule engages): the grouped
  schedule is bit-identical to the same GEMMs issued singly at split 2 after the other layers; wgrad_pair=False issues
  the parent schedule's launches and results; pair on vs off (split 2 vs 4: another summation order) agree within the
  tolerance tests/test_gpu_e2e_numerics.py uses between schedules computing from the same weights (each layer's
  update within 1e-2 relative, the loss within 1e-5).
"""
import pytest
import torch

from fpga_ai_nic_amd import _ext
from fpga_ai_nic_amd.ops import gemm as G
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

pytestmark = pytest.mark.gpu

RNE = wire.codec_id("bfp_rne")
OWN_ALL = -2  # GemmArgs::wire_own kWireOwnAll: every shard also written to C in f32

GROUPS = [([(256, 512), (512, 256)], 512),                # 4 K-tiles per split
          ([(256, 512), (512, 256)], 256),                # 2 K-tiles per split (the short prologue)
          ([(256, 768), (256, 256), (512, 256)], 512)]    # 6, 2 and 4 units: XCD padding, problem lookup


def _problem(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(K, M, generator=g) * 2 - 1) * 0.5).to("cuda", torch.bfloat16)
    dz = ((torch.rand(K, N, generator=g) * 2 - 1) * 0.1).to("cuda", torch.bfloat16)
    n = M * N + N
    n_pad = (n + 255) // 256 * 256
    master = ((torch.rand(n_pad, generator=g) * 2 - 1) * 0.05).cuda()
    mom = ((torch.rand(n_pad, generator=g) * 2 - 1) * 0.01).cuda()
    return dict(x=x, dz=dz, M=M, N=N, n=n, n_pad=n_pad, master=master, mom=mom)


_cache: dict = {}


def _problems(shapes, K):
    key = (tuple(shapes), K)
    if key not in _cache:
        _cache[key] = [_problem(M, N, K, 100 * K + 7 * i + M + N) for i, (M, N) in enumerate(shapes)]
    return _cache[key]


def _state(P, mode):
    """Fresh output planes of problem P: (grad, wire buffer, master, lp, mom) and the wire / update arguments."""
    grad = torch.zeros(P["n_pad"], device="cuda")
    buf = torch.zeros(wire.shard_bytes("bfp_rne", P["n_pad"]), dtype=torch.uint8, device="cuda")
    master = P["master"].clone()
    lp = master.to(torch.bfloat16)
    mom = P["mom"].clone() if mode == "upd_mom" else None
    if mode == "wire":
        w, upd = (buf, P["n_pad"], OWN_ALL, RNE), None
    else:
        opt = dict(lr=0.02, momentum=0.9, weight_decay=1e-3) if mode == "upd_mom" else dict(lr=0.05)
        w, upd = (buf, P["n_pad"], -1, RNE), G.LocalUpdate(master, lp, mom, **opt)
    M, N = P["M"], P["N"]
    planes = [grad, buf, master, lp] + ([mom] if mom is not None else [])
    return planes, (P["x"], P["dz"], grad[: M * N].view(M, N), grad[M * N: P["n"]], w, upd)


def _queue_bias_reduce(Q):
    """An unsplit fused-update GEMM that queues its bias-gradient reduce on the stream; returns its planes."""
    planes, (x, dz, C, cs, w, upd) = _state(Q, "upd")
    G.gemm(x, True, dz, False, C, G.EPI_WIRE, colsum=cs, wire=w, update=upd, defer_colsum=True, split_k=1,
           tile=(256, 256))
    assert G.pending_colsum() == 1
    return planes


def _run_both(probs, split, mode, qcs):
    """(planes of the single launches, planes of the grouped launch), each with the queued layer's planes first."""
    out = []
    Q = _problems([(256, 256)], 512)[0] if qcs else None
    for grouped in (False, True):
        planes = [_queue_bias_reduce(Q)] if qcs else []
        args = []
        for P in probs:
            pl, a = _state(P, mode)
            planes.append(pl)
            args.append(a)
        if grouped:
            G.gemm_wgrad_splitk_group(args, split)
        else:
            for x, dz, C, cs, w, upd in args:
                G.gemm(x, True, dz, False, C, G.EPI_WIRE, colsum=cs, wire=w, update=upd, split_k=split,
                       tile=(256, 256))
        assert G.pending_colsum() == 0, "the split reduce runs the queued bias-gradient reduce"
        out.append(planes)
    torch.cuda.synchronize()
    return out


def _assert_identical(single, grouped, probs, mode, qcs):
    for k, (a, b) in enumerate(zip(single, grouped)):
        for u, v in zip(a, b):
            assert torch.equal(u, v), f"problem {k - int(qcs)}: a plane differs from the single launch's"
    for P, pl in zip(probs, grouped[int(qcs):]):
        if mode == "wire":
            assert pl[1].any() and pl[0][: P["n"]].any(), "no wire / f32 gradient written"
        else:
            assert not torch.equal(pl[2], P["master"]), "weights not updated"
            assert not pl[1].any(), "the fused update stores no wire"
    if qcs:
        Q = _problems([(256, 256)], 512)[0]
        k = Q["M"] * Q["N"]
        assert not torch.equal(grouped[0][2][k: Q["n"]], Q["master"][k: Q["n"]]), "queued bias update did not run"


@pytest.mark.parametrize("qcs", [False, True])
@pytest.mark.parametrize("mode", ["wire", "upd", "upd_mom"])
@pytest.mark.parametrize("shapes,K", GROUPS)
def test_group_bit_identical_to_single_launches(shapes, K, mode, qcs):
    probs = _problems(shapes, K)
    single, grouped = _run_both(probs, 2, mode, qcs)
    _assert_identical(single, grouped, probs, mode, qcs)


@pytest.mark.parametrize("shapes,K", GROUPS)
def test_group_within_fp64_bound(shapes, K):
    probs = _problems(shapes, K)
    states = [_state(P, "wire") for P in probs]
    G.gemm_wgrad_splitk_group([a for _, a in states], 2)
    torch.cuda.synchronize()
    for P, (_, (x, dz, C, cs, _, _)) in zip(probs, states):
        xd, dd = x.double(), dz.double()
        err = (C.double() - xd.t() @ dd).abs()
        bound = 2e-5 * (xd.abs().t() @ dd.abs()) + 1e-6
        assert bool((err <= bound).all()), f"dW {P['M']}x{P['N']}: max err {err.max().item()}"
        eb = (cs.double() - dd.sum(0)).abs()
        assert bool((eb <= 2e-5 * dd.abs().sum(0) + 1e-6).all()), f"db: max err {eb.max().item()}"


@pytest.mark.parametrize("mode", ["wire", "upd_mom"])
def test_group_split4(mode):
    probs = _problems([(256, 256), (256, 256)], 1024)
    single, grouped = _run_both(probs, 4, mode, False)
    _assert_identical(single, grouped, probs, mode, False)


def test_group_rejections():
    C = _ext.require()
    ok = C.gemm_wgrad_splitk_group_supported
    assert ok([(256, 512, 512), (512, 256, 512)], 2) and ok([(256, 256, 1024)] * 8, 4)
    assert not ok([(256, 512, 512), (512, 256, 448)], 2), "K % (64 * split)"
    assert not ok([(256, 512, 512), (512, 256, 640)], 4), "K % (64 * split)"
    assert not ok([(256, 384, 512), (512, 256, 512)], 2), "N % 256"
    assert not ok([(128, 512, 512), (512, 256, 512)], 2), "M % 256"
    assert not ok([(256, 256, 512)] * 9, 2), "more than kGroupMax problems"
    assert not ok([(256, 512, 512), (512, 256, 512)], 3), "split 2 or 4"
    # the launch refuses what the predicate refuses
    bad = [_state(P, "upd")[1] for P in (_problem(256, 384, 512, 1), _problem(512, 256, 512, 2))]
    with pytest.raises(RuntimeError, match="unsupported"):
        G.gemm_wgrad_splitk_group(bad, 2)
    # the trainer's rule: the planner's limits for a split (K / s >= 1024), two or more problems
    e = lambda K, M, N: (torch.empty(K, M, device="cuda", dtype=torch.bfloat16),  # noqa: E731
                         torch.empty(K, N, device="cuda", dtype=torch.bfloat16))
    assert G.wgrad_group_split([e(4096, 1024, 4096), e(4096, 4096, 1024)]) == 2
    assert G.wgrad_group_split([e(1024, 1024, 4096), e(1024, 4096, 1024)]) == 0, "K / s < 1024"
    assert G.wgrad_group_split([e(4096, 1024, 4096)]) == 0, "a lone problem"
    assert G.wgrad_group_split([e(4096, 1024, 1024), e(4096, 1024, 1024)]) == 0, "s = 8: not a launcher split"
    assert G.wgrad_static_split(*e(2048, 1024, 4096)) == 0, "below 4096 rows the plan is not 256x256 split-K"
    assert G.wgrad_static_split(*e(4096, 1024, 4096)) == 4
    assert G.wgrad_static_split(*e(4096, 4096, 4096)) == 0, "unsplit plan"


# ------------------------------------------------------------------------------------------------ trainer level
SIZES, MB, STEPS = [1024, 4096, 4096, 1024], 4096, 3


def _trainer(pair):
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine

    eng = make_engine(ThreadFabric(1).transport(0), "bfp", impl="native")
    m = MLP(SIZES, dtype=torch.bfloat16, device="cuda", seed=3, momentum=True,
            pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(m, eng, lr=0.02, momentum=0.9, wgrad_pair=pair)
    assert tr.fused_update
    return tr


def _batch():
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(MB, SIZES[0], generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    y = torch.randint(0, SIZES[-1], (MB,), generator=g, dtype=torch.int32).cuda()
    return x, y


def _planes(tr):
    return [(l.master.clone(), l.lp.clone(), l.mom.clone(), l.gb.clone()) for l in tr.m.layers]


def _parent_step(tr, x, y):
    """The schedule before the grouped launch, written out: per layer L-1..0 bwd-data, then the fused-update
    bwd-weight GEMM at its own plan; the queued bias-gradient reduces flushed at the end."""
    m = tr.m
    tr.forward_pass(x)
    m.loss_backward(y, grad_scale=tr.loss_scale / x.shape[0])
    for i in reversed(range(m.L)):
        l = m.layers[i]
        m.backward_data(i)
        upd = G.LocalUpdate(l.master, l.lp, l.mom, lr=tr.lr, grad_scale=tr.grad_scale, weight_decay=tr.wd,
                            momentum=tr.momentum, nesterov=tr.nesterov)
        m.backward_weight(i, wire=tr.engine.prepack_target(l.grad, l.n, None), update=upd, defer_colsum=True)
    G.flush_colsum()
    return m.loss_rows


class _Spy:
    """Records the extension's GEMM-side launches (name, operand shapes, epilogue, split, tile) while active."""

    NAMES = ("gemm", "gemm_wgrad_splitk_group", "gemm_flush_colsum")

    def __init__(self, monkeypatch):
        self.calls = []
        C = _ext.require()
        for name in self.NAMES:
            monkeypatch.setattr(C, name, self._wrap(name, getattr(C, name)))

    def _wrap(self, name, fn):
        def f(*a, **kw):
            if name == "gemm":
                self.calls.append((name, tuple(a[0].shape), a[1], tuple(a[2].shape), a[3], a[5], a[9], a[11], a[12],
                                   bool(kw.get("defer_colsum", False)), kw.get("upd_master") is not None))
            elif name == "gemm_wgrad_splitk_group":
                self.calls.append((name, tuple(tuple(x.shape) for x in a[0]), a[4]))
            else:
                self.calls.append((name,))
            return fn(*a, **kw)
        return f


def test_trainer_pair_bit_identical_to_singles_at_split_2():
    x, y = _batch()
    res = []
    for pair in ("single", True):
        tr = _trainer(pair)
        losses = [tr.step(x, y).float().mean().item() for _ in range(STEPS)]
        assert G.pending_colsum() == 0, "every queued bias update lands within its step"
        tr.finish()
        assert tr.fused_updates == STEPS * tr.m.L, "one fused update per layer and step"
        assert tr.wgrad_groups == (STEPS if pair is True else 0)
        res.append((losses, _planes(tr)))
    assert res[0][0] == res[1][0], "losses differ"
    for a, b in zip(res[0][1], res[1][1]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_trainer_pair_off_is_the_parent_schedule(monkeypatch):
    x, y = _batch()
    spy = _Spy(monkeypatch)
    res = []
    for parent in (True, False):
        tr = _trainer(False)
        losses = []
        for step in range(STEPS):
            if step == 1:  # (a first step may hold the plan tuner's trial launches)
                spy.calls.clear()
            loss = _parent_step(tr, x, y) if parent else tr.step(x, y)
            losses.append(loss.float().mean().item())
        tr.finish()
        assert tr.wgrad_groups == 0
        res.append((losses, _planes(tr), list(spy.calls)))
    assert res[0][2] == res[1][2], "launch sequence differs from the parent schedule's"
    assert not any(c[0] == "gemm_wgrad_splitk_group" for c in res[1][2])
    assert res[0][0] == res[1][0], "losses differ"
    for a, b in zip(res[0][1], res[1][1]):
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_trainer_pair_launch_sequence(monkeypatch):
    """Pair on: per step the narrow layers' two split-4 GEMMs are replaced by one grouped launch at split 2 that ends
    the backward; nothing is left for flush_colsum to launch."""
    x, y = _batch()
    spy = _Spy(monkeypatch)
    tr = _trainer(True)
    tr.step(x, y)
    spy.calls.clear()
    tr.step(x, y)
    tr.finish()
    wires = [c for c in spy.calls if c[0] == "gemm" and c[5] == G.EPI_WIRE]
    assert [c[1] for c in wires] == [(MB, 4096)] and wires[0][3] == (MB, 4096), "only layer 1's GEMM runs singly"
    groups = [c for c in spy.calls if c[0] == "gemm_wgrad_splitk_group"]
    assert groups == [("gemm_wgrad_splitk_group", ((MB, 4096), (MB, 1024)), 2)]
    last_gemm = max(i for i, c in enumerate(spy.calls) if c[0] == "gemm")
    assert spy.calls.index(groups[0]) > last_gemm, "the group runs after every bwd-data GEMM"


def test_trainer_pair_on_vs_off_within_schedule_tolerance():
    """Split 2 (pair on) vs split 4 (off) for the narrow layers: from the same weights every step, the same loss and
    each layer's update within the tolerance between schedules (tests/test_gpu_e2e_numerics.py: 1e-2 relative,
    loss 1e-5)."""
    x, y = _batch()
    on, off = _trainer(True), _trainer(False)
    for step in range(STEPS):
        for a, b in zip(on.m.layers, off.m.layers):  # both step from the pair-off trainer's weights
            a.master.copy_(b.master)
            a.lp.copy_(b.lp)
            a.mom.copy_(b.mom)
        before = [l.master.clone() for l in off.m.layers]
        l_on = on.step(x, y).float().mean().item()
        l_off = off.step(x, y).float().mean().item()
        on.finish()
        off.finish()
        assert abs(l_on - l_off) <= 1e-5 * abs(l_off)
        for i, (a, b, w0) in enumerate(zip(on.m.layers, off.m.layers, before)):
            ua, ub = a.master - w0, b.master - w0
            rel = float((ua - ub).norm() / ub.norm())
            print(f"step {step} layer {i}: update rel diff {rel:.2e}")
            assert ub.norm() > 0 and rel <= 1e-2
    assert on.wgrad_groups == STEPS and off.wgrad_groups == 0
