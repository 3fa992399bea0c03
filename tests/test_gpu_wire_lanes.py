"""``C.wire_reduce`` in both lane layouts of the BFP codecs (bfp_format.h Lanes16: a 16-value group per lane; Lanes4: 4
values per lane, 4 lanes a group; ``C.set_wire_reduce4``) against the NumPy oracle, bit for bit.

The two layouts are one kernel body instantiated twice, so they must agree with the oracle and with each other on the
f32 sum, on every byte of the re-encoded wire shard, and on leaving the bytes past the shard alone. The cases run in a
child process with ``FAN_WIRE_MAX_BLOCKS=1`` (the cap is read once per process): one workgroup of 256 lanes covers
1024 elements per trip in the 4-value layout and 4096 in the 16-value layout, so

* ``n_s = 256`` (the smallest legal shard) fills part of one trip (64 / 16 active lanes), and
* ``n_s = 4352`` (17 x 256) takes 4 full trips and a quarter trip / one full trip and a trip of 16 lanes:

the smallest shapes that run the grid-stride loop, a partial last trip and the "a 16-lane segment (a quad) is all in
or all out of range" assumption of the exponent stores. Crossed with both codecs, 1 and 2 slots, the dense operand at
the first and the last slot, as f32, as bf16 and absent, and the wire / f32 / both outputs.

Inputs: slot r is ``_special_vector`` (test_gpu_kernels.py: an all-zero group, denormals, one huge value that flushes
its group, the -1 edge of the truncating codec, 2^-126 in the first 96 elements, then normals scaled by 2^-30..2^29)
times 2^(-3r). With at most two slots the largest sum is 3e38 * (1 + 1/8) < FLT_MAX, so every sum is finite (asserted
on the oracle's result): a NaN or infinity would only test payload conventions."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = (256, 4352)


def _cases():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_kernels import _special_vector

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import bfp_oracle as O
    from fpga_ai_nic_amd.ops import wire

    C = _ext.require()
    why, n_cases = [], 0
    try:
        for codec, n_s in itertools.product(("bfp_trunc", "bfp_rne"), SHAPES):
            sb = O.shard_bytes(codec, n_s)
            parts = [_special_vector(n_s, seed=r) * np.float32(2.0 ** (-3 * r)) for r in range(2)]
            packed = [O.pack(p, n_s, codec) for p in parts]
            slots_dev = torch.from_numpy(np.concatenate(packed)).cuda()
            for n_slots, local_kind in itertools.product((1, 2), ("f32", "bf16", None)):
                for self_pos in sorted({0, n_slots - 1}):
                    local = None
                    if local_kind is not None:
                        local = torch.from_numpy(parts[self_pos]).to(
                            torch.float32 if local_kind == "f32" else torch.bfloat16)
                    acc = O.reduce_slots(packed[:n_slots], None if local is None else local.float().numpy(), self_pos,
                                         codec, n_s)
                    assert np.isfinite(acc).all(), "the test's inputs must sum to finite values"
                    ref_wire = O.pack(acc, n_s, codec)
                    local_dev = None if local is None else local.cuda()
                    for outs, lane4 in itertools.product(("wire", "f32", "both"), (0, 1)):
                        n_cases += 1
                        tag = f"{codec} n_s={n_s} slots={n_slots} self={self_pos} local={local_kind} out={outs} " \
                              f"lane4={lane4}"
                        ow = of = None
                        if outs != "f32":
                            ow = torch.full((sb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                        if outs != "wire":
                            of = torch.full((n_s,), float("nan"), dtype=torch.float32, device="cuda")
                        C.set_wire_reduce4(lane4)
                        C.wire_reduce(slots_dev, n_slots, self_pos, local_dev, ow, of, n_s, wire.codec_id(codec))
                        if of is not None and not np.array_equal(of.cpu().numpy().view(np.uint32),
                                                                 acc.view(np.uint32)):
                            why.append(f"{tag}: f32 sum differs from the oracle")
                        if ow is not None:
                            got = ow.cpu().numpy()
                            if not np.array_equal(got[:sb], ref_wire):
                                why.append(f"{tag}: wire output differs from the oracle")
                            if not (got[sb:] == 0xA5).all():
                                why.append(f"{tag}: bytes past the shard were written")
    finally:
        C.set_wire_reduce4(1)
    return {"ok": not why, "why": why[:20], "cases": n_cases}


def test_wire_reduce_both_lane_layouts_bit_exact():
    env = dict(os.environ, FAN_WIRE_MAX_BLOCKS="1")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out\n{(e.stderr or '')[-3000:]}")
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(recs) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert recs[0]["ok"], recs[0]["why"]
    # 2 codecs x 2 shapes x (1 slot: 1 position; 2 slots: 2 positions) x 3 local operands x 3 outputs x 2 layouts
    assert recs[0]["cases"] == 2 * 2 * 3 * 3 * 3 * 2, recs[0]


if __name__ == "__main__":
    print(json.dumps(_cases()), flush=True)
