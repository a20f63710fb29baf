"""DistGCN: aggregate-then-transform GCN over partitioned graphs.

Reference parity: ``AdaQP/model/distGCN.py`` (DistGCNConv aggregates with
DistAggConv then applies the linear transform; stack uses
dropout -> LayerNorm -> ReLU between layers; Xavier init)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..ops.dist_agg import dist_aggregate
from .norm import FusedNormReluDropout, resolve_fused_norm
from .common import FastLinear


class DistGCNConv(nn.Module):
    def __init__(self, in_dim: int, out_dim: int, layer: int, use_bias: bool = True):
        super().__init__()
        self.layer = layer
        self.linear = FastLinear(in_dim, out_dim, bias=use_bias)

    def reset_parameters(self):
        self.linear.reset_parameters()

    def forward(self, engine, x: Tensor) -> Tensor:
        rst = dist_aggregate(x, engine, self.layer, self.training)
        return self.linear(rst)


class DistGCN(nn.Module):
    def __init__(self, in_dim: int, hidden_dim: int, out_dim: int,
                 num_layers: int = 3, dropout: float = 0.5,
                 use_norm: bool = True,
                 fused_norm: Optional[bool] = None):
        super().__init__()
        dims = [in_dim] + [hidden_dim] * (num_layers - 1) + [out_dim]
        self.convs = nn.ModuleList(
            [DistGCNConv(dims[i], dims[i + 1], layer=i) for i in range(num_layers)])
        # fused_norm: norms[i] does LayerNorm -> ReLU -> the next layer's
        # dropout in one op (None = on iff ADAQP_FUSED_NORM=1). Same function
        # as the unfused stack up to the dropout RNG stream. Without
        # use_norm there is nothing to fuse and the flag has no effect.
        self.fused_norm = use_norm and resolve_fused_norm(fused_norm)
        if self.fused_norm:
            self.norms = nn.ModuleList(
                [FusedNormReluDropout(hidden_dim, dropout, layer=i)
                 for i in range(num_layers - 1)])
        else:
            self.norms = nn.ModuleList(
                [nn.LayerNorm(hidden_dim, elementwise_affine=True)
                 for _ in range(num_layers - 1)]) if use_norm else None
        self.dropout = nn.Dropout(dropout)

    def forward(self, engine, feats: Tensor) -> Tensor:
        h = feats
        for i, conv in enumerate(self.convs):
            h = self.dropout(h) if i > 0 and not self.fused_norm else h
            h = conv(engine, h)
            if i < len(self.convs) - 1:
                if self.fused_norm:
                    h = self.norms[i](h)
                    continue
                if self.norms is not None:
                    h = self.norms[i](h)
                h = torch.relu(h)
        return h
