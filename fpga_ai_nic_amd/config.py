"""Typed run configuration (replaces the reference's positional CLI + compile-time constants).

Reference knobs and where they went:
  iters / MB / fuse_type / type / bn bk bc / C1..CN  -> positional CLI, kept (sw/mlp_mpi_example_f32.cpp:270-320)
  NUM_NODES=3 (sw:38)                               -> world size from the launcher (any N >= 1)
  `BFP_EN (hw/all_reduce.sv:13)                     -> compress = bfp | bfp4 | raw | rccl | local
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
    compress: str = "bfp"          # bfp | bfp4 | raw | raw_bf16 | rccl | local
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
    optimizer: str = "sgd"         # sgd | adamw | lion
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
        """(beta1, beta2) with the optimizer's defaults filled in: AdamW's (0.9, 0.999), Lion's (0.9, 0.99)."""
        d1, d2 = (0.9, 0.99) if self.optimizer == "lion" else (0.9, 0.999)
        return (d1 if self.beta1 is None else self.beta1, d2 if self.beta2 is None else self.beta2)


def add_named_flags(ap: argparse.ArgumentParser):
    d = TrainConfig()
    ap.add_argument("--dtype", default=d.dtype, choices=["bf16", "f32"])
    ap.add_argument("--compress", default=d.compress, choices=["bfp", "bfp4", "raw", "raw_bf16", "rccl", "local"],
                    help="wire format of the all-reduce: bfp = 8-bit mantissas (17 B per 16 values), bfp4 = 4-bit "
                         "mantissas (9 B per 16 values, --rounding rne only; meant for use with --error-feedback)")
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
    ap.add_argument("--optimizer", default=d.optimizer, choices=["sgd", "adamw", "lion"],
                    help="weight update fused into the all-reduce epilogue; lion: sign of the interpolated momentum "
                         "with decoupled decay, one f32 moment plane (SGD-momentum's bytes and state); not with "
                         "--momentum, --trust-ratio or --moment-codec bfp8")
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
    return {"bfp": f"bfp_{rounding}", "raw": "raw_f32", "raw_bf16": "raw_bf16"}[compress]


def config_from_args(a, positional_sizes=None) -> TrainConfig:
    c = TrainConfig()
    for f in dataclasses.fields(TrainConfig):
        key = f.name
        if hasattr(a, key):
            setattr(c, key, getattr(a, key))
    if positional_sizes:
        c.sizes = list(positional_sizes)
    if c.compress == "bfp4":
        wire_codec(c.compress, c.rounding)  # (--rounding trunc: a ValueError)
    return c
