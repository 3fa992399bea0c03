"""The checks of tests/test_gpu_step_numerics.py can be met and are not empty — shown without a GPU: the same
``run_case`` on the CPU fallbacks with the Python engine. (a) every case but the large one passes every check (the
reference sums its GEMMs in float64, the fallbacks in float32, so the two do not agree by construction); (b) a
trainer state with the mistakes a step can make — a layer's bias update dropped, one 16-value group of an update moved
by 4 BFP steps, the last 8 columns of a ragged dW update missing, a stale bf16 copy, stale logits, a momentum plane
written past its bucket — fails the check meant for it. Also: ops/nn.py's ``softmax_xent_slabs_supported`` (what
ops/gemm.py asks before it leaves a classifier's slabs to the softmax) agrees with the native one."""
import pytest
import test_gpu_step_numerics as S
import torch

CPU = "cpu"
SMALL = [n for n in S.CASES if n != "wgrad_group"]
# a small momentum case whose buckets end inside their padding (the GPU file's momentum case fills its buckets)
MOM_RAGGED = S.Case("momentum_ragged", [72, 40, 24], 16, momentum=0.9, nesterov=True, weight_decay=1e-4)


# ---------------------------------------------------------------------------------------------------------------
# (a) the fallbacks pass


@pytest.mark.parametrize("name", SMALL)
def test_cpu_step_passes(name):
    r = S.run_case(CPU, S.CASES[name])
    assert r["steps"] == 3 and r["worst"]["elem"] <= S.ELEM_STEPS


def test_cpu_momentum_ragged_passes():
    r = S.run_case(CPU, MOM_RAGGED)
    assert all(l.n < l.n_pad for l in r["m"].layers)


def test_slab_support_agrees_with_the_native_check(C):
    from fpga_ai_nic_amd.ops import nn as NN

    for c in list(range(0, 2100)) + [2176, 4096, 1 << 20]:
        assert NN.softmax_xent_slabs_supported(c) == C.softmax_xent_slabs_supported(c), c
    assert NN.softmax_xent_slabs_supported(1000, 1000) and not NN.softmax_xent_slabs_supported(1000, 1004)


# ---------------------------------------------------------------------------------------------------------------
# (b) planted mistakes fail


def _restore(l, snap_master, sl):
    """Layer l's master (and bf16 copy) over ``sl`` back at its value before the step."""
    l.master[sl] = snap_master[sl]
    if l.lp is not None:
        l.lp[sl] = l.master[sl].to(torch.bfloat16)


def test_dropped_bias_update_fails():
    def tamper(s, m, snap, prev):
        l = m.layers[0]
        _restore(l, snap["master"][0], slice(l.cin * l.cout, l.n))

    with pytest.raises(AssertionError, match=r"\(d\) layer 0 bias segment"):
        S.run_case(CPU, S.CASES["mixed_prepack"], steps=1, tamper=tamper)


def test_group_moved_by_four_steps_fails():
    """One group of 16 among a million elements: invisible to the norm, caught per element."""
    case = S.CASES["mixed_prepack"]
    seen = {}

    def tamper(s, m, snap, prev):
        l = m.layers[1]
        g0 = 16 * 1234
        d = (l.master[g0:g0 + 16] - snap["master"][1][g0:g0 + 16]).abs().max()  # lr max|q(g)| of the group
        seen["rel"] = float(4 * S.BFP_STEP * d / (l.master[: l.n] - snap["master"][1][: l.n]).norm())
        l.master[g0:g0 + 16] += 4 * S.BFP_STEP * d
        l.lp[g0:g0 + 16] = l.master[g0:g0 + 16].to(torch.bfloat16)

    with pytest.raises(AssertionError, match=r"\(e\) layer 1 update per element: 1[0-6] of"):
        S.run_case(CPU, case, steps=1, tamper=tamper)
    assert 4 * seen["rel"] < S.EMUL_BOUND, "the planted error must be far below what the norm check sees"


def test_last_columns_of_ragged_update_missing_fails():
    def tamper(s, m, snap, prev):
        l = m.layers[1]
        w0 = snap["master"][1][: l.cin * l.cout].view(l.cin, l.cout)
        l.w_master[:, -8:] = w0[:, -8:]
        l.lp[: l.n] = l.master[: l.n].to(torch.bfloat16)

    with pytest.raises(AssertionError, match=r"\(d\) layer 1 weight segment"):
        S.run_case(CPU, S.CASES["ragged_fold"], steps=1, tamper=tamper)


def test_stale_lp_fails():
    def tamper(s, m, snap, prev):
        l = m.layers[0]
        l.lp[: l.cin * l.cout] = snap["W"][0].flatten().to(torch.bfloat16)

    with pytest.raises(AssertionError, match=r"\(f\) layer 0: lp is not bf16\(master\)"):
        S.run_case(CPU, S.CASES["fuse1"], steps=1, tamper=tamper)


def test_stale_logits_fail():
    def tamper(s, m, snap, prev):
        if s == 1:
            m.logits.copy_(prev)

    with pytest.raises(AssertionError, match=r"step 1 \(a\) logits"):
        S.run_case(CPU, S.CASES["fuse1"], steps=2, tamper=tamper)


def test_momentum_padding_written_fails():
    def tamper(s, m, snap, prev):
        l = m.layers[1]
        l.mom[l.n] = 1e-3

    with pytest.raises(AssertionError, match=r"\(f\) layer 1: momentum padding not zero"):
        S.run_case(CPU, MOM_RAGGED, steps=1, tamper=tamper)
