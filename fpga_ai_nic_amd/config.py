"""Typed run configuration (replaces the reference's positional CLI + compile-time constants).

Reference knobs and where they went:
  iters / MB / fuse_type / type / bn bk bc / C1..CN  -> positional CLI, kept (sw/mlp_mpi_example_f32.cpp:270-320)
  NUM_NODES=3 (sw:38)                               -> world size from the launcher (any N >= 1)
  `BFP_EN (hw/all_reduce.sv:13)                     -> compress = bfp | bfp4 | sign | raw | rccl | local | powersgd |
                                                        topk | sketch | drive
  NUM_FP=16, MANT_SIZE=8 (hw/bfp_adapter.sv:34-36)   -> group of 16; 8-bit mantissas (bfp; rounding = rne | trunc, the
                                                        bit-exact ref) or 4-bit (bfp4, rne only)
  BUF_SIZE=512 CL slice (hw/all_reduce.sv:102)      -> slice_elems (ring)
  lr 0.1 hard-coded (hw/weight_update.sv:444)        -> lr, momentum, weight_decay
  loss_weight 0.1 (sw:250)                           -> loss_scale
"""
from __future__ import annotations

import argparse
import dataclasses
from dataclasses import dataclass, field


@dataclass
class TrainConfig:
    iters: int = 10
    global_mb: int = 32
    fuse_type: int = 0
    type: str = "A"
    bn: int = 64
    bk: int = 64
    bc: int = 64
    sizes: list = field(default_factory=lambda: [1024, 4096, 4096, 1024])
    dtype: str = "bf16"            # bf16 | f32
    f32_gemm: str = "mfma"         # --dtype f32: mfma (exact f32 MFMA GEMM) | bf16x3 (split precision, 3 bf16 MFMAs)
    compress: str = "bfp"          # bfp | bfp4 | sign | raw | raw_bf16 | rccl | local | powersgd | topk | sketch |
                                   # drive
    rank: int = 4                  # powersgd: the rank of the approximation, 1..16
    lowrank_seed: int = 0          # powersgd: seed of the initial Q factors (the same on every rank)
    lowrank_orth: str = "mgs"      # powersgd: mgs (modified Gram-Schmidt) | cholqr2 (multi-workgroup CholeskyQR2)
    density: float = 0.01          # topk, sketch: the fraction of a bucket that is sent / recovered, in (0, 1]
    sketch_rows: int = 5           # sketch: rows of the count sketch, 1 | 3 | 5
    sketch_cols: int = 65536       # sketch: columns of the count sketch, a multiple of 1024 in 1024 .. 2^22
    sketch_seed: int = 0           # sketch: seed of the hashes (the same on every rank), an int in [0, 2^64)
    drive_seed: int = 0            # drive: seed of the rotation's signs (the same on every rank), in [0, 2^64)
    rounding: str = "rne"          # rne | trunc
    algo: str = "mesh"             # mesh | ring
    rings: int = 1
    slice_elems: int = 1 << 22
    transport: str = "torch"       # torch | native | p2p
    engine: str = "native"         # native (C++ engine, GPU) | python; CPU runs always use python
    compat_owner_fp32: bool = False
    lr: float = 0.1
    momentum: float = 0.0
    weight_decay: float = 0.0
    optimizer: str = "sgd"         # sgd | adamw | lion | adafactor
    trust_ratio: bool = False      # adamw: layer-wise trust ratio (LAMB)
    clip_grad_norm: float = 0.0    # > 0: clip the reduced gradient of all layers to this 2-norm (0: off)
    error_feedback: bool = False   # BFP mesh: each encoder keeps what it drops and adds it to the next step's input
    stochastic_rounding: bool = False  # rne BFP mesh: each encoder rounds up with probability = the dropped fraction
    sr_seed: int = 0               # the run's base seed of the stochastic rounding, an int in [0, 2^64)
    moment_codec: str = "f32"      # adamw: f32 | bfp8 (both moments in 8-bit block floating point, 2.125 B / parameter)
    beta1: float | None = None     # None: the optimizer's default (adamw 0.9, lion 0.9)
    beta2: float | None = None     # None: the optimizer's default (adamw 0.999, lion 0.99)
    eps: float = 1e-8
    loss_scale: float = 1.0
    warmup: int = 2
    seed: int = 1
    profile: bool = False
    checkpoint: str = ""
    resume: str = ""
    metrics_jsonl: str = ""
    timeout_s: float = 600.0
    device: str = "auto"           # auto | cpu | cuda

    def to_dict(self):
        return dataclasses.asdict(self)

    def betas(self):
        """(beta1, beta2) with the optimizer's defaults filled in: AdamW's (0.9, 0.999), Lion's (0.9, 0.99); None for
        Adafactor, which has none (a --beta1 / --beta2 given with it is passed on and refused)."""
        if self.optimizer == "adafactor" and self.beta1 is None and self.beta2 is None:
            return None
        d1, d2 = (0.9, 0.99) if self.optimizer == "lion" else (0.9, 0.999)
        return (d1 if self.beta1 is None else self.beta1, d2 if self.beta2 is None else self.beta2)


def add_named_flags(ap: argparse.ArgumentParser):
    d = TrainConfig()
    ap.add_argument("--dtype", default=d.dtype, choices=["bf16", "f32"])
    ap.add_argument("--f32-gemm", default=d.f32_gemm, choices=["mfma", "bf16x3"],
                    help="--dtype f32: the GEMM of every layer product; mfma = the exact f32 MFMA kernel, bf16x3 = "
                         "f32 operands split in registers into two bf16 pieces each, three bf16 MFMAs per product "
                         "(about 2^-14.4 relative per product)")
    ap.add_argument("--compress", default=d.compress,
                    choices=["bfp", "bfp4", "sign", "raw", "raw_bf16", "rccl", "local", "powersgd", "topk", "sketch",
                             "drive"],
                    help="wire format of the all-reduce: bfp = 8-bit mantissas (17 B per 16 values), bfp4 = 4-bit "
                         "mantissas (9 B per 16 values, --rounding rne only; meant for use with --error-feedback), "
                         "sign = one sign bit per value and a power-of-two scale per group (codec sign1, 3 B per 16 "
                         "values; needs --error-feedback, --rounding rne only), powersgd = PowerSGD low-rank compression "
                         "(each layer crosses the transport as (rows + cols) x --rank f32 numbers; engine-less trainer "
                         "over the chosen transport, own residual: not with --error-feedback or "
                         "--stochastic-rounding; layer widths multiples of 16; its residual and factors are not "
                         "checkpointed: --resume restarts them at zero and from --lowrank-seed), topk = top-k "
                         "sparsification with memory (each rank sends the --density largest-magnitude fraction of "
                         "every bucket as 8 B index/value pairs, one all-gather per bucket; engine-less trainer, own "
                         "residual, not checkpointed: not with --error-feedback or --stochastic-rounding; at most 16 "
                         "ranks), sketch = count-sketch compression (each rank all-reduces a --sketch-rows x "
                         "--sketch-cols f32 sketch of every bucket, every rank recovers the same --density fraction "
                         "of indices from the sum, and a second all-reduce carries their exact values: 4 * (rows * "
                         "cols + k) B per bucket whatever the world size; engine-less trainer, own residual, not "
                         "checkpointed: not with --error-feedback or --stochastic-rounding), drive = rotated "
                         "one-bit compression (DRIVE: every block of 4096 values is rotated by a randomised Hadamard "
                         "transform and sent as one sign bit per value and one f32 scale, 516 B per 4096 values, one "
                         "all-gather per bucket; engine-less trainer, own residual in rotated coordinates, not "
                         "checkpointed: not with --error-feedback or --stochastic-rounding; at most 16 ranks)")
    ap.add_argument("--rank", type=int, default=d.rank, help="--compress powersgd: rank of the approximation, 1..16")
    ap.add_argument("--lowrank-seed", type=int, default=d.lowrank_seed,
                    help="--compress powersgd: seed of the initial Q factors")
    ap.add_argument("--lowrank-orth", default=d.lowrank_orth, choices=["mgs", "cholqr2"],
                    help="--compress powersgd: how P is orthogonalised: mgs = modified Gram-Schmidt in one workgroup, "
                         "cholqr2 = CholeskyQR2 spread over 256-row strips (three launches; other bits than mgs)")
    ap.add_argument("--density", type=float, default=d.density,
                    help="--compress topk: fraction of every bucket each rank sends, in (0, 1]; --compress sketch: "
                         "fraction of every bucket recovered from the summed sketch")
    ap.add_argument("--sketch-rows", type=int, default=d.sketch_rows, choices=[1, 3, 5],
                    help="--compress sketch: rows of the count sketch (the estimate is their median)")
    ap.add_argument("--sketch-cols", type=int, default=d.sketch_cols,
                    help="--compress sketch: columns of the count sketch, a multiple of 1024 in 1024 .. 2^22")
    ap.add_argument("--sketch-seed", type=int, default=d.sketch_seed,
                    help="--compress sketch: seed of the bucket and sign hashes, an int in [0, 2^64)")
    ap.add_argument("--drive-seed", type=int, default=d.drive_seed,
                    help="--compress drive: seed of the rotation's signs, an int in [0, 2^64)")
    ap.add_argument("--rounding", default=d.rounding, choices=["rne", "trunc"])
    ap.add_argument("--algo", default=d.algo, choices=["mesh", "ring"])
    ap.add_argument("--rings", type=int, default=d.rings)
    ap.add_argument("--slice-elems", type=int, default=d.slice_elems)
    ap.add_argument("--transport", default=d.transport, choices=["torch", "native", "p2p"])
    ap.add_argument("--engine", default=d.engine, choices=["python", "native"],
                    help="request path: Python-issued engine (any transport) or the C++ engine (GPU)")
    ap.add_argument("--compat-owner-fp32", action="store_true")
    ap.add_argument("--lr", type=float, default=d.lr)
    ap.add_argument("--momentum", type=float, default=d.momentum)
    ap.add_argument("--weight-decay", type=float, default=d.weight_decay)
    ap.add_argument("--optimizer", default=d.optimizer, choices=["sgd", "adamw", "lion", "adafactor"],
                    help="weight update fused into the all-reduce epilogue; lion: sign of the interpolated momentum "
                         "with decoupled decay, one f32 moment plane (SGD-momentum's bytes and state); not with "
                         "--momentum, --trust-ratio or --moment-codec bfp8; adafactor: factored second moment "
                         "(rows + cols floats of state per layer), absolute --lr, update clipping at 1; mesh schedule "
                         "only, not with --momentum, --trust-ratio, --clip-grad-norm or --moment-codec bfp8")
    ap.add_argument("--trust-ratio", action="store_true",
                    help="AdamW: scale each layer's step by ||w|| / ||update|| (LAMB; two-pass epilogue)")
    ap.add_argument("--clip-grad-norm", type=float, default=d.clip_grad_norm,
                    help="clip the step's reduced gradient (all layers, one vector) to this 2-norm (0: off; at most 8 "
                         "layers)")
    ap.add_argument("--error-feedback", action="store_true",
                    help="compressed mesh all-reduce (BFP codecs): every encoder keeps what it drops in a per-rank f32 "
                         "residual plane per layer and adds it to the next step's input; the engine then packs the "
                         "gradients itself (no GEMM-fused encode); --compress local takes the one-slot round trip "
                         "of the --rounding codec. The planes are not checkpointed: --resume restarts them at zero")
    ap.add_argument("--stochastic-rounding", action="store_true",
                    help="compressed mesh all-reduce (--compress bfp | bfp4, --rounding rne): every encoder rounds up "
                         "with probability equal to the dropped fraction, so each encode is unbiased; stateless (no "
                         "plane, no extra traffic), not with --error-feedback; the engine then packs the gradients "
                         "itself (no GEMM-fused encode). The update counter its seeds come from is checkpointed")
    ap.add_argument("--sr-seed", type=int, default=d.sr_seed,
                    help="base seed of --stochastic-rounding, an int in [0, 2^64)")
    ap.add_argument("--moment-codec", default=d.moment_codec, choices=["f32", "bfp8"],
                    help="--optimizer adamw: keep both moments in 8-bit block floating point (2.125 B per parameter "
                         "instead of 8; stored with stochastic rounding under --sr-seed, the second as sqrt(v)); not "
                         "with --trust-ratio. Checkpointed with the codec's name: --resume needs the same codec")
    ap.add_argument("--beta1", type=float, default=d.beta1,
                    help="AdamW first-moment decay / Lion's update interpolation (default 0.9)")
    ap.add_argument("--beta2", type=float, default=d.beta2,
                    help="AdamW second-moment decay (default 0.999) / Lion's momentum decay (default 0.99)")
    ap.add_argument("--eps", type=float, default=d.eps, help="AdamW denominator term")
    ap.add_argument("--loss-scale", type=float, default=d.loss_scale)
    ap.add_argument("--warmup", type=int, default=d.warmup)
    ap.add_argument("--seed", type=int, default=d.seed)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--checkpoint", default="")
    ap.add_argument("--resume", default="")
    ap.add_argument("--metrics-jsonl", default="")
    ap.add_argument("--timeout-s", type=float, default=d.timeout_s)
    ap.add_argument("--device", default=d.device, choices=["auto", "cpu", "cuda"])
    return ap


def wire_codec(compress: str, rounding: str = "rne") -> str:
    """The wire codec name of a --compress / --rounding pair (the engine kinds of ``parallel.dp.make_engine``)."""
    if compress == "bfp4":
        if rounding != "rne":
            raise ValueError(f"--compress bfp4 has no {rounding!r} rounding: the 4-bit codec is bfp4_rne only (the "
                             f"reference ships no 4-bit configuration to be bit-exact to)")
        return "bfp4_rne"
    if compress == "sign":
        if rounding != "rne":
            raise ValueError(f"--compress sign has no {rounding!r} rounding: the sign1 codec keeps no mantissa to "
                             f"truncate")
        return "sign1"
    return {"bfp": f"bfp_{rounding}", "raw": "raw_f32", "raw_bf16": "raw_bf16"}[compress]


def config_from_args(a, positional_sizes=None) -> TrainConfig:
    c = TrainConfig()
    for f in dataclasses.fields(TrainConfig):
        key = f.name
        if hasattr(a, key):
            setattr(c, key, getattr(a, key))
    if positional_sizes:
        c.sizes = list(positional_sizes)
    if c.f32_gemm != "mfma" and c.dtype != "f32":
        raise ValueError(f"--f32-gemm {c.f32_gemm} selects the GEMM of the f32 path: it needs --dtype f32")
    if c.compress in ("bfp4", "sign"):
        wire_codec(c.compress, c.rounding)  # (--rounding trunc: a ValueError)
    if c.compress == "sign" and not c.error_feedback:
        raise ValueError("--compress sign: sign1 needs error feedback (--error-feedback): one bit per value converges "
                         "only with the residual carried over")
    if c.lowrank_orth not in ("mgs", "cholqr2"):
        raise ValueError(f"--lowrank-orth must be mgs or cholqr2, got {c.lowrank_orth!r}")
    if c.lowrank_orth != "mgs" and c.compress != "powersgd":
        raise ValueError(f"--lowrank-orth {c.lowrank_orth} selects PowerSGD's orthogonalisation: it needs --compress "
                         f"powersgd")
    if c.compress == "powersgd":
        if not 1 <= c.rank <= 16:
            raise ValueError(f"--rank must lie in 1..16, got {c.rank}")
        if c.error_feedback or c.stochastic_rounding:
            raise ValueError("--compress powersgd keeps its own residual: not with --error-feedback or "
                             "--stochastic-rounding")
    d = TrainConfig()
    if c.compress != "sketch" and (c.sketch_rows, c.sketch_cols, c.sketch_seed) != (d.sketch_rows, d.sketch_cols,
                                                                                    d.sketch_seed):
        raise ValueError("--sketch-rows, --sketch-cols and --sketch-seed shape the count sketch: they need --compress "
                         "sketch")
    if c.compress == "sketch":
        if not 0.0 < c.density <= 1.0:
            raise ValueError(f"--density must lie in (0, 1], got {c.density}")
        if c.sketch_rows not in (1, 3, 5):
            raise ValueError(f"--sketch-rows must be 1, 3 or 5, got {c.sketch_rows}")
        if c.sketch_cols % 1024 or not 1024 <= c.sketch_cols <= 1 << 22:
            raise ValueError(f"--sketch-cols must be a multiple of 1024 in 1024 .. 2^22, got {c.sketch_cols}")
        if not 0 <= c.sketch_seed < 1 << 64:
            raise ValueError(f"--sketch-seed must lie in [0, 2^64), got {c.sketch_seed}")
        if c.error_feedback or c.stochastic_rounding:
            raise ValueError("--compress sketch keeps its own residual: not with --error-feedback or "
                             "--stochastic-rounding")
    if c.compress != "drive" and c.drive_seed != d.drive_seed:
        raise ValueError("--drive-seed seeds the rotation of --compress drive: it needs --compress drive")
    if c.compress == "drive":
        if not 0 <= c.drive_seed < 1 << 64:
            raise ValueError(f"--drive-seed must lie in [0, 2^64), got {c.drive_seed}")
        if c.error_feedback or c.stochastic_rounding:
            raise ValueError("--compress drive keeps its own residual: not with --error-feedback or "
                             "--stochastic-rounding")
    if c.compress == "topk":
        if not 0.0 < c.density <= 1.0:
            raise ValueError(f"--density must lie in (0, 1], got {c.density}")
        if c.error_feedback or c.stochastic_rounding:
            raise ValueError("--compress topk keeps its own residual: not with --error-feedback or "
                             "--stochastic-rounding")
    return c
