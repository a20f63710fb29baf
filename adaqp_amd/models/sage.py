"""DistSAGE: GraphSAGE with 'mean' / 'gcn' aggregators.

Reference parity: ``AdaQP/model/distSAGE.py:46-60`` — mean:
``fc_self(local) + fc_neigh(h_neigh)``; gcn: ``fc_neigh(h_neigh)`` where
h_neigh includes the self term (handled inside the aggregation op)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..ops.dist_agg import dist_aggregate
from .norm import FusedNormReluDropout, resolve_fused_norm
import os

from . import common as _common
from .common import (FastLinear, fused_dual_linear, fused_dual_linear_ok,
                     sage_mean_layer)
from ..ops.kernels import packable


class DistSAGEConv(nn.Module):
    def __init__(self, in_dim: int, out_dim: int, layer: int,
                 aggregator_type: str = 'mean', use_bias: bool = True):
        super().__init__()
        assert aggregator_type in ('mean', 'gcn')
        self.layer = layer
        self.aggregator_type = aggregator_type
        self.fc_neigh = FastLinear(in_dim, out_dim, bias=use_bias)
        if aggregator_type == 'mean':
            self.fc_self = FastLinear(in_dim, out_dim, bias=use_bias)

    def reset_parameters(self):
        self.fc_neigh.reset_parameters()
        if self.aggregator_type == 'mean':
            self.fc_self.reset_parameters()

    def forward(self, engine, x: Tensor, pack: bool = False) -> Tensor:
        # ``pack``: x is mostly zeros (DistSAGE.forward's hint), gather it
        # from a packed copy in the forward SpMM.
        # gradients being recorded: the 'mean' layer is one autograd node
        # (same forward calls; fused input-grad add and a shared bias
        # grad in backward). The opt-in ADAQP_FUSED_SAGE path and the
        # eval / no-grad path stay on the formulation below. The node's
        # backward writes the [num_inner, F] aggregation grad as the grad
        # of x, so x must hold exactly the inner rows (it always does when
        # it comes from the layer stack).
        if (self.aggregator_type == 'mean' and torch.is_grad_enabled()
                and self.fc_self.bias is not None
                and x.shape[0] == engine.graph.num_inner
                and os.environ.get('ADAQP_FUSED_SAGE') != '1'):
            return sage_mean_layer(engine, x, self.fc_self, self.fc_neigh,
                                   self.layer, self.training, pack=pack)
        h_neigh = dist_aggregate(x, engine, self.layer, self.training)
        if self.aggregator_type == 'mean':
            x_self = x[:engine.graph.num_inner]
            if (engine.compute_dtype == torch.bfloat16
                    and fused_dual_linear_ok(x_self, h_neigh,
                                             self.fc_neigh.weight.shape[1])):
                return fused_dual_linear(x_self, h_neigh,
                                         self.fc_self, self.fc_neigh)
            return self.fc_self(x_self) + self.fc_neigh(h_neigh)
        return self.fc_neigh(h_neigh)


class DistSAGE(nn.Module):
    def __init__(self, in_dim: int, hidden_dim: int, out_dim: int,
                 num_layers: int = 3, dropout: float = 0.5,
                 use_norm: bool = True, aggregator_type: str = 'mean',
                 fused_norm: Optional[bool] = None):
        super().__init__()
        dims = [in_dim] + [hidden_dim] * (num_layers - 1) + [out_dim]
        self.convs = nn.ModuleList(
            [DistSAGEConv(dims[i], dims[i + 1], layer=i,
                          aggregator_type=aggregator_type)
             for i in range(num_layers)])
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

    def _pack_hint(self, engine, i: int, h: Tensor) -> bool:
        """Whether layer i's forward SpMM should gather from packed rows.
        Decided from what is known on the host, never from a device-side
        count: the input of a layer > 0 in training is
        dropout(relu(norm(.))), and with p >= 0.5 at most half of it is
        non-zero in expectation (about a quarter with the ReLU), for the
        nn.Dropout stack and the fused-norm stack alike. The tensor must
        qualify once cast to the compute dtype (fp32, F % 4 == 0,
        F <= 256). ADAQP_SPMM_PACKED=0/1 switches the whole thing."""
        if os.environ.get('ADAQP_SPMM_PACKED',
                          _common.SPMM_PACKED_DEFAULT) != '1':
            return False
        return (i > 0 and self.training and self.dropout.p >= 0.5
                and engine.compute_dtype == torch.float32
                and h.dtype == torch.float32 and packable(h))

    def forward(self, engine, feats: Tensor) -> Tensor:
        h = feats
        for i, conv in enumerate(self.convs):
            h = self.dropout(h) if i > 0 and not self.fused_norm else h
            if self._pack_hint(engine, i, h):
                h = conv(engine, h, pack=True)
            else:
                h = conv(engine, h)
            if i < len(self.convs) - 1:
                if self.fused_norm:
                    h = self.norms[i](h)
                    continue
                if self.norms is not None:
                    h = self.norms[i](h)
                h = torch.relu(h)
        return h
