"""Checkpoint / resume in the reference-compatible weight layout.

The reference never writes weights to disk; its in-memory layout is one contiguous row-major
``C[i] x C[i+1]`` fp32 buffer per layer (sw/mlp_mpi_example_f32.cpp:396-401) plus a ``C[i+1]`` bias. This module
defines the on-disk format as exactly that:

* ``<path>.safetensors`` — tensors ``fc{i}.weight`` [C_i, C_{i+1}] and ``fc{i}.bias`` [C_{i+1}] in f32 (or bf16),
  optional ``fc{i}.momentum`` (flat, f32: SGD's momentum, or Lion's one moment plane when the index says
  ``optimizer`` = "lion"), or for an AdamW model ``fc{i}.exp_avg`` / ``fc{i}.exp_avg_sq`` (its two
  moment planes, flat, f32; the index then carries ``optimizer`` and ``opt_step``, the updates applied so far; a
  stochastically rounded run adds ``sr_step``, the update counter its request seeds are derived from; a model with
  8-bit moment planes stores each plane's bytes whole under the same two names, uint8, and the index carries
  ``moment_codec`` = "bfp8" and the planes' ``moment_n_pad``);
* ``<path>.json`` — index: layer shapes / dtypes / byte offsets into a plain concatenated ``.bin`` image, the
  libxsmm blocking ``bn/bk/bc`` as metadata, iteration counter, world size and engine settings.
* ``<path>.bin`` — the raw concatenation (weight_0, bias_0, weight_1, ...) so a C/C++ consumer (e.g. the
  reference's ``fil_libxsmm[i]`` arrays) can ``fread`` each layer directly.

Only rank 0 writes; loading uses safetensors (no pickle).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from safetensors.torch import load_file, save_file


def save(path: str, model, *, iteration: int = 0, dtype: str = "f32", meta: dict | None = None,
         optimizer: str | None = None, opt_step: int | None = None, sr_step: int | None = None):
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    tensors, index, off = {}, [], 0
    blobs = []
    for i, l in enumerate(model.layers):
        w = l.w_master.detach().to("cpu", tdt).contiguous()
        b = l.b_master.detach().to("cpu", tdt).contiguous()
        tensors[f"fc{i}.weight"] = w
        tensors[f"fc{i}.bias"] = b
        if getattr(l, "var", None) is not None and l.var.dtype == torch.uint8:  # 8-bit planes: their bytes, whole
            tensors[f"fc{i}.exp_avg"] = l.mom.detach().to("cpu").contiguous()
            tensors[f"fc{i}.exp_avg_sq"] = l.var.detach().to("cpu").contiguous()
        elif getattr(l, "var", None) is not None:
            tensors[f"fc{i}.exp_avg"] = l.mom[: l.n].detach().to("cpu").contiguous()
            tensors[f"fc{i}.exp_avg_sq"] = l.var[: l.n].detach().to("cpu").contiguous()
        elif l.mom is not None:
            tensors[f"fc{i}.momentum"] = l.mom[: l.n].detach().to("cpu").contiguous()
        for name, t in ((f"fc{i}.weight", w), (f"fc{i}.bias", b)):
            raw = t.view(torch.uint8).numpy().tobytes() if tdt == torch.bfloat16 else t.numpy().tobytes()
            index.append({"name": name, "shape": list(t.shape), "dtype": dtype, "offset": off, "nbytes": len(raw)})
            blobs.append(raw)
            off += len(raw)
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    save_file(tensors, path + ".safetensors")
    with open(path + ".bin", "wb") as f:
        for raw in blobs:
            f.write(raw)
    info = {"format": "fpga_ai_nic_amd/mlp-v1", "sizes": model.sizes, "iteration": iteration, "dtype": dtype,
            "layout": "row-major C[i] x C[i+1] (reference fil_libxsmm order)", "tensors": index}
    if any(getattr(l, "var", None) is not None and l.var.dtype == torch.uint8 for l in model.layers):
        info["moment_codec"] = "bfp8"
        info["moment_n_pad"] = [int(l.var.numel() // 17 * 16) for l in model.layers]
    if optimizer is not None:
        info["optimizer"] = optimizer
    if opt_step is not None:
        info["opt_step"] = int(opt_step)
    if sr_step is not None:  # the stochastic-rounding trainer's update counter (the step of its request seeds)
        info["sr_step"] = int(sr_step)
    info.update(meta or {})
    with open(path + ".json", "w") as f:
        json.dump(info, f, indent=1)
    return path


def load(path: str, model, optimizer: str | None = None) -> dict:
    """``optimizer``: the resuming run's. Lion's ``fc{i}.momentum`` plane is not SGD's momentum and not AdamW's first
    moment, so a checkpoint whose index names an optimizer loads into a Lion run, and a Lion checkpoint into any run,
    only under that optimizer."""
    with open(path + ".json") as f:
        info = json.load(f)
    saved_opt = info.get("optimizer")
    if optimizer is not None and saved_opt is not None and saved_opt != optimizer and "lion" in (saved_opt, optimizer):
        raise ValueError(f"checkpoint was written under optimizer={saved_opt!r}; this run is optimizer={optimizer!r} "
                         f"(Lion's moment plane belongs to Lion alone: resume under the optimizer the checkpoint was "
                         f"written with)")
    if list(info["sizes"]) != list(model.sizes):
        raise ValueError(f"checkpoint sizes {info['sizes']} != model sizes {model.sizes}")
    sd = load_file(path + ".safetensors")
    saved = info.get("moment_codec", "f32")
    for i, l in enumerate(model.layers):
        if getattr(l, "var", None) is None or f"fc{i}.exp_avg_sq" not in sd:
            continue
        have = "bfp8" if l.var.dtype == torch.uint8 else "f32"
        if have != saved:
            raise ValueError(f"checkpoint moments were saved under moment_codec={saved!r}; the model holds {have!r} "
                             f"planes (resume under the codec the checkpoint was written with)")
        if have == "bfp8" and sd[f"fc{i}.exp_avg"].numel() != l.mom.numel():
            raise ValueError(f"checkpoint fc{i}: 8-bit moment planes of n_pad = {sd[f'fc{i}.exp_avg'].numel() // 17 * 16}"
                             f" elements; the model's bucket is padded to {l.mom.numel() // 17 * 16} (the plane layout "
                             f"depends on n_pad: resume under the same engine layout)")
    for i, l in enumerate(model.layers):
        l.w_master.copy_(sd[f"fc{i}.weight"].to(l.master.device, torch.float32))
        l.b_master.copy_(sd[f"fc{i}.bias"].to(l.master.device, torch.float32))
        if getattr(l, "var", None) is not None and l.var.dtype == torch.uint8 and f"fc{i}.exp_avg_sq" in sd:
            l.mom.copy_(sd[f"fc{i}.exp_avg"].to(l.mom.device))
            l.var.copy_(sd[f"fc{i}.exp_avg_sq"].to(l.var.device))
        elif getattr(l, "var", None) is not None and f"fc{i}.exp_avg_sq" in sd:
            l.mom[: l.n].copy_(sd[f"fc{i}.exp_avg"].to(l.mom.device))
            l.var[: l.n].copy_(sd[f"fc{i}.exp_avg_sq"].to(l.var.device))
        elif l.mom is not None and f"fc{i}.momentum" in sd:
            l.mom[: l.n].copy_(sd[f"fc{i}.momentum"].to(l.mom.device))
    model.sync_lp()
    return info


def read_raw_layer(path: str, name: str) -> np.ndarray:
    """Read one layer from the plain ``.bin`` image via the JSON index (what a C++ consumer does)."""
    with open(path + ".json") as f:
        info = json.load(f)
    ent = next(t for t in info["tensors"] if t["name"] == name)
    with open(path + ".bin", "rb") as f:
        f.seek(ent["offset"])
        raw = f.read(ent["nbytes"])
    if ent["dtype"] == "f32":
        return np.frombuffer(raw, dtype=np.float32).reshape(ent["shape"])
    u = np.frombuffer(raw, dtype=np.uint16).astype(np.uint32) << 16
    return u.view(np.float32).reshape(ent["shape"])
