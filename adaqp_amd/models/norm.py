"""FusedNormReluDropout: LayerNorm -> ReLU -> dropout as one op.

Drop-in for the ``nn.LayerNorm`` entries of a model's ``norms`` list:
parameters are named ``weight``/``bias`` with LayerNorm's init, so
``state_dict`` keys and shapes are the same with and without fusion and
checkpoints load either way with ``strict=True``. The dropout it applies
is the one the unfused stack applies at the top of the NEXT layer.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..ops.norm_act import norm_relu_dropout

_M32 = 0xFFFFFFFF


def resolve_fused_norm(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_FUSED_NORM=1``; an explicit bool wins."""
    if flag is None:
        return os.environ.get('ADAQP_FUSED_NORM') == '1'
    return bool(flag)


def _mix32(h: int) -> int:
    """The triple32 avalanche of ops/quant.py on a Python int."""
    h &= _M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & _M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & _M32
    h ^= h >> 16
    return h


def derive_seed(base_seed: int, layer: int, counter: int, rank: int) -> int:
    """32-bit dropout seed for one call: a hash chain over
    (base_seed, layer, counter, rank), so layers, steps and ranks all draw
    different masks."""
    h = _mix32(base_seed)
    for v in (layer, counter, rank):
        h = _mix32(h ^ ((v * 0x9E3779B9 + 0x7F4A7C15) & _M32))
    return h


class FusedNormReluDropout(nn.Module):
    def __init__(self, hidden: int, p: float, layer: int, eps: float = 1e-5,
                 base_seed: int = 2026):
        super().__init__()
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f'dropout p must be in [0, 1), got {p}')
        self.hidden, self.p, self.layer = hidden, float(p), layer
        self.eps, self.base_seed = eps, base_seed
        self.weight = nn.Parameter(torch.ones(hidden))
        self.bias = nn.Parameter(torch.zeros(hidden))
        # its own stream: the engine's quantization seeds are not consumed
        self.calls = 0
        self.last_seed: Optional[int] = None

    def reset_parameters(self):
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)

    def _next_seed(self) -> int:
        from ..comm.communicator import Communicator
        rank = Communicator.ctx.rank if Communicator.ctx is not None else 0
        seed = derive_seed(self.base_seed, self.layer, self.calls, rank)
        self.calls += 1
        return seed

    def forward(self, x: Tensor) -> Tensor:
        seed = 0
        if self.training and self.p > 0.0:
            seed = self.last_seed = self._next_seed()
        return norm_relu_dropout(x, self.weight, self.bias, self.p, seed,
                                 self.training, self.eps)

    def extra_repr(self) -> str:
        return f'{self.hidden}, p={self.p}, layer={self.layer}, eps={self.eps}'
