"""Reading a local checkpoint directory (config.json + *.safetensors shards): shared by the LMM interfaces and the CLIP tower."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Dict

import torch


def read_safetensors_dir(path: Path) -> Dict[str, torch.Tensor]:
    """Every tensor of every *.safetensors shard under `path`.  There is no network: a missing directory or an empty one is an error."""
    from safetensors.torch import load_file
    path = Path(path)
    if not path.is_dir():
        raise FileNotFoundError(f"{path} is not a local checkpoint directory (no network access to fetch one)")
    sd: Dict[str, torch.Tensor] = {}
    for f in sorted(path.glob("*.safetensors")):
        sd.update(load_file(str(f)))
    if not sd:
        raise FileNotFoundError(f"no *.safetensors shards under {path}")
    return sd


def read_config_json(path: Path) -> dict:
    with open(Path(path) / "config.json") as f:
        return json.load(f)
