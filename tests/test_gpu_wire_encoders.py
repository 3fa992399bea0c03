"""The three encoder forms of the mesh schedule's two kernels (bfp_kernels.hip ``wire_pack_to_kernel`` /
``wire_reduce_to_kernel`` over EncPlain / EncFeedback / EncStochastic) side by side against the NumPy oracle, byte for
byte: the forms share one traversal per kernel, so what the traversal does wrong shows in all of them.

The cases run in a child process with ``FAN_WIRE_MAX_BLOCKS=1`` (the cap is read once per process), as
test_gpu_wire_lanes.py: one workgroup of 256 lanes covers 4096 elements per trip with a group per lane and 1024 with 4
values per lane, so ``n_s = 256`` (the smallest legal shard) fills part of one trip and ``n_s = 4352`` (17 x 256) takes
full trips and a partial one in both lane layouts.

* Senders, 3 shards, f32 and bf16 input, every codec the form is instantiated for: ``C.wire_pack_to`` (the plain form
  through a destination table, which only the engine reaches otherwise) against ``O.pack``, ``wire.pack_ef`` against
  ``O.ef_pack``, ``wire.pack_sr`` against ``O.sr_pack``. Shard 1's destination is null (its bytes never exist, its
  residual stays), shard 2 is ``self_shard`` of the two forms that have one (plain bytes, its residual stays); every
  destination buffer ends in a 64-byte guard that must stay as it was.
* Owners, ``n_slots`` in {1, 2, 3, 8} (both lane layouts at the default flag), the dense operand at the first and the
  last slot, two destinations, the second null or not: ``wire.reduce_ef`` / ``wire.reduce_sr`` against
  ``O.ef_reduce`` / ``O.sr_reduce``; both destinations receive the same bytes.
* Identities between the forms: error feedback with an all-zero residual writes the plain form's bytes and leaves
  x - dec(enc(x)); stochastic rounding of values the codec represents exactly (dec(O.pack(x))) writes the plain form's
  bytes under every seed tried.

Inputs: ``_special_vector`` (test_gpu_kernels.py). Slot r is scaled by 2^(-3r) as in test_gpu_wire_lanes.py and, since
that test stops at two slots and 3e38 * (1 + 1/8 + 1/64) is past FLT_MAX, negated for odd r: the partial sums of
3e38 * (1 - 1/8 + 1/64 - ...) stay below 3e38 * 1.002. Residuals are a special vector times 2^-12. Every sum is finite
(asserted on the oracle's results): a NaN or infinity would only test payload conventions. No tolerance anywhere."""
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
ALL_CODECS = ("bfp_trunc", "bfp_rne", "raw_f32", "raw_bf16", "bfp4_rne")
EF_CODECS = ("bfp_trunc", "bfp_rne", "bfp4_rne")
SR_CODECS = ("bfp_rne", "bfp4_rne")
SEED, RANK = 0x9E3779B97F4A7C15, 5
SLOT_POS = [(n, p) for n in (1, 2, 3, 8) for p in sorted({0, n - 1})]  # 7 (n_slots, self_pos) pairs


def _cases():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_kernels import _special_vector

    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import bfp_oracle as O
    from fpga_ai_nic_amd.ops import wire

    C = _ext.require()
    why, count = [], {"senders": 0, "owners": 0, "identities": 0}

    def bufs(sb, present):
        return [torch.full((sb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if p else None for p in present]

    def check_dst(tag, d, ref, sb):
        got = d.cpu().numpy()
        if not np.array_equal(got[:sb], ref):
            why.append(f"{tag}: bytes differ from the oracle")
        if not (got[sb:] == 0xA5).all():
            why.append(f"{tag}: the guard after the destination was written")

    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

    # ---- senders: shard 0 takes the form, shard 1 has a null destination, shard 2 is self_shard
    for n_s, dt in itertools.product(SHAPES, (torch.float32, torch.bfloat16)):
        x_t = torch.from_numpy(_special_vector(3 * n_s, seed=11)).to(dt)
        x = x_t.float().numpy()  # what the kernel sees
        x_dev = x_t.cuda()
        e0 = _special_vector(3 * n_s, seed=12) * np.float32(2.0 ** -12)
        shard = [slice(q * n_s, (q + 1) * n_s) for q in range(3)]
        for codec in ALL_CODECS:
            sb = O.shard_bytes(codec, n_s)
            tag = f"pack plain {codec} n_s={n_s} {dt}"
            count["senders"] += 1
            d = bufs(sb, (True, False, True))
            C.wire_pack_to(x_dev, d, n_s, wire.codec_id(codec))
            ref = O.pack(x, n_s, codec)
            for q in (0, 2):
                check_dst(f"{tag} shard {q}", d[q], ref[q * sb:(q + 1) * sb], sb)
            if codec in EF_CODECS:
                tag = f"pack ef {codec} n_s={n_s} {dt}"
                count["senders"] += 1
                d = bufs(sb, (True, False, True))
                e_dev = torch.from_numpy(e0).cuda()
                wire.pack_ef(x_dev, e_dev, d, n_s, codec, self_shard=2)
                ref_w, ref_e = O.ef_pack(x[shard[0]], e0[shard[0]], n_s, codec)
                assert np.isfinite(ref_e).all(), "the test's inputs must stay finite"
                check_dst(f"{tag} shard 0", d[0], ref_w, sb)
                check_dst(f"{tag} self_shard", d[2], O.pack(x[shard[2]], n_s, codec), sb)
                e = e_dev.cpu().numpy()
                if not np.array_equal(bits(e[shard[0]]), bits(ref_e)):
                    why.append(f"{tag}: residual of shard 0 differs from the oracle")
                if not np.array_equal(bits(e[shard[1]]), bits(e0[shard[1]])):
                    why.append(f"{tag}: the null destination's residual was touched")
                if not np.array_equal(bits(e[shard[2]]), bits(e0[shard[2]])):
                    why.append(f"{tag}: self_shard's residual was touched")
                # identity: an all-zero residual gives the plain form's bytes and leaves x - dec(enc(x))
                count["identities"] += 1
                dz, dp = bufs(sb, (True, True, True)), bufs(sb, (True, True, True))
                z_dev = torch.zeros(3 * n_s, dtype=torch.float32, device="cuda")
                wire.pack_ef(x_dev, z_dev, dz, n_s, codec)
                C.wire_pack_to(x_dev, dp, n_s, wire.codec_id(codec))
                for q in range(3):
                    if not torch.equal(dz[q], dp[q]):
                        why.append(f"{tag}: zero residual, shard {q} differs from the plain form")
                with np.errstate(over="ignore", invalid="ignore"):
                    drop = (x - O.quantize(x, codec)).astype(np.float32)
                if not np.array_equal(bits(z_dev.cpu().numpy()), bits(drop)):
                    why.append(f"{tag}: zero residual does not leave x - dec(enc(x))")
            if codec in SR_CODECS:
                tag = f"pack sr {codec} n_s={n_s} {dt}"
                count["senders"] += 1
                d = bufs(sb, (True, False, True))
                wire.pack_sr(x_dev, d, n_s, codec, SEED, RANK, self_shard=2, base=512)
                check_dst(f"{tag} shard 0", d[0], O.sr_pack(x[shard[0]], n_s, codec, SEED, RANK, base=512), sb)
                check_dst(f"{tag} self_shard", d[2], O.pack(x[shard[2]], n_s, codec), sb)
                # identity: values the codec represents exactly keep the plain form's bytes under every seed
                xq = O.quantize(x, codec)
                xq_dev = torch.from_numpy(xq).to(dt).cuda()  # (exact in bf16 too: at most 8 significant bits)
                if not np.array_equal(bits(xq_dev.float().cpu().numpy()), bits(xq)):
                    why.append(f"{tag}: the codec's values are not exact in {dt}")
                dp = bufs(sb, (True, True, True))
                C.wire_pack_to(xq_dev, dp, n_s, wire.codec_id(codec))
                for seed in (0, 1, SEED):
                    count["identities"] += 1
                    ds_ = bufs(sb, (True, True, True))
                    wire.pack_sr(xq_dev, ds_, n_s, codec, seed, RANK)
                    for q in range(3):
                        if not torch.equal(ds_[q], dp[q]):
                            why.append(f"{tag}: exact input, seed {seed}, shard {q} differs from the plain form")

    # ---- owners
    for n_s, codec in itertools.product(SHAPES, EF_CODECS):
        sb = O.shard_bytes(codec, n_s)
        parts = [_special_vector(n_s, seed=r) * np.float32((-1.0) ** r * 2.0 ** (-3 * r)) for r in range(8)]
        packed = [O.pack(p, n_s, codec) for p in parts]
        slots_dev = torch.from_numpy(np.concatenate(packed)).cuda()
        e0 = _special_vector(n_s, seed=13) * np.float32(2.0 ** -12)
        for (n_slots, self_pos), dt, second in itertools.product(SLOT_POS, (torch.float32, torch.bfloat16),
                                                                 (False, True)):
            local_t = torch.from_numpy(parts[self_pos]).to(dt)
            local, local_dev = local_t.float().numpy(), local_t.cuda()
            acc = O.reduce_slots(packed[:n_slots], local, self_pos, codec, n_s)
            assert np.isfinite(acc).all(), "the test's inputs must sum to finite values"
            tag = f"{codec} n_s={n_s} slots={n_slots} self={self_pos} {dt} second={second}"
            count["owners"] += 1
            d = bufs(sb, (True, second))
            e_dev = torch.from_numpy(e0).cuda()
            wire.reduce_ef(slots_dev, n_slots, self_pos, local_dev, e_dev, d, n_s, codec)
            ref_w, ref_e = O.ef_reduce(packed[:n_slots], local, self_pos, e0, codec, n_s)
            assert np.isfinite(ref_e).all(), "the test's inputs must stay finite"
            for q in range(1 + second):
                check_dst(f"reduce ef {tag} destination {q}", d[q], ref_w, sb)
            if not np.array_equal(bits(e_dev.cpu().numpy()), bits(ref_e)):
                why.append(f"reduce ef {tag}: residual differs from the oracle")
            if codec in SR_CODECS:
                count["owners"] += 1
                d = bufs(sb, (True, second))
                wire.reduce_sr(slots_dev, n_slots, self_pos, local_dev, d, n_s, codec, SEED, RANK, base=3 * n_s)
                ref_w = O.sr_reduce(packed[:n_slots], local, self_pos, codec, n_s, SEED, RANK, base=3 * n_s)
                for q in range(1 + second):
                    check_dst(f"reduce sr {tag} destination {q}", d[q], ref_w, sb)
            if second:
                continue
            # identities (once per slot count, position and dtype): a zero residual gives the plain bytes of the sum
            # and leaves acc - dec(enc(acc))
            count["identities"] += 1
            d = bufs(sb, (True,))
            z_dev = torch.zeros(n_s, dtype=torch.float32, device="cuda")
            wire.reduce_ef(slots_dev, n_slots, self_pos, local_dev, z_dev, d, n_s, codec)
            check_dst(f"reduce ef {tag} zero residual", d[0], O.pack(acc, n_s, codec), sb)
            with np.errstate(over="ignore", invalid="ignore"):
                drop = (acc - O.quantize(acc, codec)).astype(np.float32)
            if not np.array_equal(bits(z_dev.cpu().numpy()), bits(drop)):
                why.append(f"reduce ef {tag}: zero residual does not leave y - dec(enc(y))")
        if codec in SR_CODECS:
            # one slot, the dense operand exact in the codec: the sum is the operand, every seed keeps the plain bytes
            xq = O.quantize(parts[0], codec)
            for dt, seed in itertools.product((torch.float32, torch.bfloat16), (0, 1, SEED)):
                count["identities"] += 1
                d = bufs(sb, (True,))
                wire.reduce_sr(slots_dev, 1, 0, torch.from_numpy(xq).to(dt).cuda(), d, n_s, codec, seed, RANK)
                check_dst(f"reduce sr {codec} n_s={n_s} {dt} exact input, seed {seed}", d[0], O.pack(xq, n_s, codec),
                          sb)
    return {"ok": not why, "why": why[:20], "count": count}


def test_encoder_forms_bit_exact():
    env = dict(os.environ, FAN_WIRE_MAX_BLOCKS="1")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                           timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"child timed out\n{(e.stderr or '')[-3000:]}")
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(recs) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert recs[0]["ok"], recs[0]["why"]
    shapes_dtypes = len(SHAPES) * 2
    assert recs[0]["count"] == {
        "senders": shapes_dtypes * (len(ALL_CODECS) + len(EF_CODECS) + len(SR_CODECS)),
        "owners": shapes_dtypes * len(SLOT_POS) * 2 * (len(EF_CODECS) + len(SR_CODECS)),
        "identities": shapes_dtypes * (len(EF_CODECS) + 3 * len(SR_CODECS))            # senders
        + shapes_dtypes * len(SLOT_POS) * len(EF_CODECS) + shapes_dtypes * 3 * len(SR_CODECS),  # owners
    }, recs[0]


if __name__ == "__main__":
    print(json.dumps(_cases()), flush=True)
