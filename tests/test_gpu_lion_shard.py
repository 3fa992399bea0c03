"""Sharded weight update with Lion (engine ``shard_update``): the owner of each mesh shard fuses its reduce with the
codec round trip + Lion of that shard (bfp_kernels.hip wire_reduce_sgd_kernel with LionParams, in the Lanes16 or Lanes4
lane layout) and the ranks all-gather the updated bf16 weights.

As with SGD and AdamW (test_gpu_shard_update.py, test_gpu_adamw_shard.py) it must train bit-identically to the
unsharded schedule: per rank, the weights it writes (``lp``) and, once gathered from their owners (``gather_owned``),
its master and its one moment plane equal the unsharded engine's — over the direct P2P transport and the copying
loopback fabric, in both lane layouts of the owner kernel and with the 4-bit codec. Each case runs in a child process
with one hardware queue per stream, under a 150 s limit, once."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpga_ai_nic_amd import _ext  # noqa: E402
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce  # noqa: E402

pytestmark = pytest.mark.gpu


def _case(world, fabric, codec="bfp_rne", n=50000 - 48, steps=2):
    C = _ext.require()
    rng = np.random.default_rng(7 + world)
    w0 = rng.standard_normal(n).astype(np.float32)
    grads = [[(rng.standard_normal(n) * (1 + r)).astype(np.float32) for r in range(world)] for _ in range(steps)]

    def comms():
        if fabric == "p2p":
            cs = [C.P2PComm(r, world, 0, 2 << 20, 2) for r in range(world)]
            C.P2PComm.connect_local(cs)
            return cs
        f = C.LoopbackFabric(world, 60.0)
        return [f.comm(r) for r in range(world)]

    arms = {}
    for shard in (False, True):
        cs = comms()
        arms[shard] = ([NativeAllReduce(None, codec=codec, algo="mesh", comm=cs[r], shard_update=shard)
                        for r in range(world)], cs)
    assert all(e.shard_update for e in arms[True][0]) and not any(e.shard_update for e in arms[False][0])
    res = {False: [None] * world, True: [None] * world}
    errs = []

    def run(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for shard in (False, True):
                    eng = arms[shard][0][r]
                    L = eng.layout(n)
                    w = torch.zeros(L.n_pad, device="cuda")
                    w[:n] = torch.from_numpy(w0).cuda()
                    lp = w.to(torch.bfloat16)
                    mom = torch.zeros(L.n_pad, device="cuda")
                    for k in range(steps):
                        g = torch.zeros(L.n_pad, device="cuda")
                        g[:n] = torch.from_numpy(grads[k][r]).cuda()
                        kw = {}
                        tgt = eng.prepack_target(g, n) if k == 1 else None
                        if tgt is not None:  # the producer's encoding as the input (second step; BFP codecs)
                            C.wire_pack_range(g, tgt[0], tgt[1], 0, n // 16 * 16, tgt[3])
                            kw["prepacked"] = (tgt[0], n // 16 * 16)
                        out = torch.zeros_like(lp) if shard else lp  # the sharded request writes the NEXT buffer
                        h = eng.allreduce_sgd(g, w, out, mom, n_valid=n, lr=1e-3, grad_scale=1.0 / world,
                                              weight_decay=1e-3, defer=True, opt="lion", **kw)
                        h.commit_after_current()
                        h.synchronize(60)
                        lp = out
                    s.synchronize()
                    for plane in (w, mom):
                        eng.gather_owned(plane, n)
                    res[shard][r] = (w.cpu().numpy(), lp.float().cpu().numpy(), mom.cpu().numpy(),
                                     eng.counters()["sharded_updates"])
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e!r}")

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    why = list(errs)
    if any(t.is_alive() for t in ts):
        why.append("virtual rank thread hung")
    if not why:
        for r in range(world):
            wa, la, ma, _ = res[False][r]
            wb, lb, mb, cnt = res[True][r]
            if cnt != steps:
                why.append(f"rank {r}: {cnt} sharded updates, expected {steps}")
            if not (np.any(mb[:n] != 0) and np.any(wb[:n] != w0)):
                why.append(f"rank {r}: the update did not run")
            for name, a, b in (("master", wa, wb), ("weights", la, lb), ("moment", ma, mb)):
                if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                    why.append(f"rank {r}: {name} differ from the unsharded schedule")
            for name, k in (("master", 0), ("weights", 1), ("moment", 2)):
                if not np.array_equal(res[True][0][k].view(np.uint32), res[True][r][k].view(np.uint32)):
                    why.append(f"rank {r}: {name} differ from rank 0's")
    return {"ok": not why, "why": why}


def _child(world, fabric, codec="bfp_rne", **extra_env):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="32", **extra_env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(world), fabric, codec], env=env,
                           capture_output=True, text=True, timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"world {world} {fabric}: child timed out\n{(e.stderr or '')[-3000:]}")
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(recs) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert recs[0]["ok"], recs[0]["why"]


@pytest.mark.parametrize("world,fabric", [(2, "p2p"), (3, "p2p"), (3, "loopback")])
def test_lion_shard_update_bit_identical_to_unsharded(world, fabric):
    _child(world, fabric)


def test_lion_shard_update_group_per_lane_reduce():
    """The owner reduce + Lion kernel in its one-group-per-lane form (FAN_WIRE_REDUCE4=0)."""
    _child(2, "p2p", FAN_WIRE_REDUCE4="0")


def test_lion_shard_update_bfp4():
    """bfp4_rne on the wire, over the copying loopback fabric."""
    _child(3, "loopback", codec="bfp4_rne")


if __name__ == "__main__":
    print(json.dumps(_case(int(sys.argv[1]), sys.argv[2], sys.argv[3])), flush=True)
