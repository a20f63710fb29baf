"""FastLinear: x @ W + b with a GEMM-based bias gradient.

torch's autograd computes grad_bias as ``grad.sum(dim=0)``, which on
ROCm lowers to a strided column reduction running at ~0.2 TB/s for the
[N, 256] grads this model produces (measured: 3.8 ms for 0.73M x 256 —
~10% of an epoch). Computing it as ``ones[1,N] @ grad`` instead routes
it through rocBLAS at memory bandwidth.

``ADAQP_COLSUM=1`` switches the GPU bias gradient to the native one-pass
``colsum`` kernel (csrc/colsum.hip; 0.40 vs 1.52 ms on N x 256 fp32). It
sums in another order than the GEMM, so fp32 bias grads differ in the
last bits and a training run drifts away from the default path's bit
for bit; that is why it is opt-in.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor

from ..ops.kernels import colsum

_ones_cache: dict = {}

# defaults of the two switches (docs/TUNING.md); the environment overrides
SPMM_PACKED_DEFAULT = '1'
AGG0_CACHE_DEFAULT = '1'


def _ones_row(n: int, device, dtype) -> Tensor:
    key = (n, device, dtype)
    t = _ones_cache.get(key)
    if t is None or t.shape[1] < n:
        t = torch.ones(1, n, device=device, dtype=dtype)
        if len(_ones_cache) > 16:
            _ones_cache.clear()
        _ones_cache[key] = t
    return t[:, :n]


def bias_grad(g: Tensor) -> Tensor:
    """Column sum of the contiguous upstream grad ``g`` [N, F], in g's
    dtype: ``ones[1,N] @ g`` on the GPU (``colsum`` with ADAQP_COLSUM=1),
    ``g.sum(0)`` on the CPU."""
    if not g.is_cuda:
        return g.sum(dim=0)
    if os.environ.get('ADAQP_COLSUM') == '1':
        return colsum(g)
    return (_ones_row(g.shape[0], g.device, g.dtype) @ g).reshape(-1)


class _LinearBiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, b: Tensor) -> Tensor:
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w)

    @staticmethod
    def backward(ctx, g: Tensor):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = g @ w.t() if ctx.needs_input_grad[0] else None
        gw = x.t() @ g if ctx.needs_input_grad[1] else None
        gb = None
        if ctx.needs_input_grad[2]:
            gb = bias_grad(g)
        return gx, gw, gb


class FastLinear(nn.Module):
    """Drop-in linear (weight stored [in, out]) with fast bias grad."""

    def __init__(self, in_dim: int, out_dim: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(in_dim, out_dim))
        self.bias = nn.Parameter(torch.zeros(out_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x: Tensor) -> Tensor:
        w, b = self.weight, self.bias
        if torch.is_autocast_enabled('cuda') and x.is_cuda:
            # differentiable casts OUTSIDE the Function: bf16 compute,
            # fp32 master weights get fp32 grads via the cast backward
            dt = torch.get_autocast_dtype('cuda')
            x = x.to(dt)
            w = w.to(dt)
            b = b.to(dt) if b is not None else None
        if b is None:
            return x @ w
        return _LinearBiasFn.apply(x, w, b)


class _FusedDualLinearFn(torch.autograd.Function):
    """out = x @ w1 + h @ w2 + (b1 + b2) via the one-pass MFMA kernel
    (csrc fused_dual_gemm_bf16); backward through plain GEMMs."""

    @staticmethod
    def forward(ctx, x: Tensor, h: Tensor, w1: Tensor, w2: Tensor,
                b1: Tensor, b2: Tensor) -> Tensor:
        from ..ops.kernels import native
        ctx.save_for_backward(x, h, w1, w2)
        M, N = x.shape[0], w1.shape[1]
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
        bias = ((b1 + b2).to(x.dtype) if b1 is not None
                else torch.empty(0, dtype=x.dtype, device=x.device))
        native().fused_dual_gemm_bf16(x.contiguous(), h.contiguous(),
                                      w1.t().contiguous(), w2.t().contiguous(),
                                      bias, out)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, h, w1, w2 = ctx.saved_tensors
        g = g.contiguous()
        gx = g @ w1.t() if ctx.needs_input_grad[0] else None
        gh = g @ w2.t() if ctx.needs_input_grad[1] else None
        gw1 = x.t() @ g if ctx.needs_input_grad[2] else None
        gw2 = h.t() @ g if ctx.needs_input_grad[3] else None
        gb = None
        if ctx.needs_input_grad[4]:
            gb = bias_grad(g)
        return gx, gh, gw1, gw2, gb, gb


def fused_dual_linear_ok(x: Tensor, h: Tensor, n_out: int) -> bool:
    """Opt-in (ADAQP_FUSED_SAGE=1): measured SLOWER than two TUNED
    hipBLASLt GEMMs + add on the products shape (152-177 vs 132 ms/epoch
    — profiles/r01_NOTES.md); hipBLASLt's pipelined schedules win this
    bandwidth-bound tall-skinny shape. Kept as a tested reference
    implementation of a fused MFMA epilogue."""
    import os
    if os.environ.get('ADAQP_FUSED_SAGE') != '1':
        return False
    from ..ops.kernels import has_native
    # fused_dual_linear casts both operands to bf16, so fp32 inputs are
    # acceptable (layer-0 features stay fp32 under a bf16 engine).
    ok_dt = (torch.bfloat16, torch.float32)
    return (x.is_cuda and x.dtype in ok_dt and h.dtype in ok_dt
            and n_out % 16 == 0 and n_out <= 256
            and x.shape[1] % 8 == 0 and h.shape[1] % 8 == 0
            and has_native())


def fused_dual_linear(x, h, lin1: 'FastLinear', lin2: 'FastLinear') -> Tensor:
    """lin1(x) + lin2(h) in one MFMA pass (bf16 CUDA); casts mirror
    FastLinear.forward so fp32 master weights get fp32 grads."""
    dt = torch.bfloat16
    return _FusedDualLinearFn.apply(
        x.to(dt), h.to(dt), lin1.weight.to(dt), lin2.weight.to(dt),
        lin1.bias.to(dt) if lin1.bias is not None else None,
        lin2.bias.to(dt) if lin2.bias is not None else None)


# --------------------------------------------------------------------------
# reuse of a constant forward aggregate (layer 0 of full-graph training)
#
# The layer-0 aggregation reads the input features: no gradient flows into
# them and, without remote rows, nothing stochastic enters the SpMM, so it
# computes the same [num_inner, F0] tensor every epoch. The engine keeps the
# last such result (one tensor, ~1 GB on the flagship) with the key it was
# computed under; an in-place change of the features bumps their version
# and misses. ADAQP_AGG0_CACHE=0 turns the reuse off. With several ranks the
# quantized exchange is stochastic per epoch, so only the central rows of
# the decomposed path would be constant; reusing those is not done.
# --------------------------------------------------------------------------

def _agg_cache_key(ctx, engine, x: Tensor, layer: int, is_train: bool):
    """Cache key, or None when the aggregate may not be reused: the input
    needs a gradient, the engine has remote rows or is tracing, or the
    switch is off."""
    if (ctx.needs_input_grad[0] or engine.graph.num_remote != 0
            or engine.is_tracing
            or os.environ.get('ADAQP_AGG0_CACHE', AGG0_CACHE_DEFAULT) == '0'):
        return None
    return (layer, x.data_ptr(), x._version, tuple(x.shape), x.dtype,
            engine.compute_dtype, bool(is_train))


def _agg_cache_get(engine, key) -> Optional[Tensor]:
    if key is None:
        return None
    kept = getattr(engine, '_agg0_kept', None)
    if kept is not None and kept[0] == key:
        engine.agg0_hits = getattr(engine, 'agg0_hits', 0) + 1
        return kept[2]
    engine.agg0_misses = getattr(engine, 'agg0_misses', 0) + 1
    return None


def _agg_cache_put(engine, key, x: Tensor, h: Tensor) -> None:
    # x is kept alive with the entry, so its data_ptr cannot be handed to
    # another tensor while the key still names it
    if key is not None:
        engine._agg0_kept = (key, x, h)


class _SageMeanFn(torch.autograd.Function):
    """The SAGE 'mean' layer, ``fc_self(x[:I]) + fc_neigh(mean_agg(x))``, as
    ONE autograd node. Forward is the unfused formulation call for call
    (propagate, two addmm, one add). What the single node buys is the
    backward: the input grad ``g @ W_self^T + A^T D^-1 (g @ W_neigh^T)`` is
    written by the backward SpMM's epilogue (``addend``) instead of by a
    zero-fill + slice copy + accumulate pass over [N, F], and the two
    biases, which receive the same upstream grad, share one column sum.

    ``w1/w2/b1/b2`` arrive already cast (bf16 under autocast), as in
    FastLinear.forward, so fp32 master weights get fp32 grads through the
    cast backward. ``x`` is cast inside, as DistAgg does: when its dtype
    differs from the compute dtype (fp32 activations under bf16 autocast)
    the two input-grad terms are added in x's dtype, exactly as autograd
    accumulated them, and the SpMM addend is not used.

    ``pack``: the caller expects ``x`` to be mostly zeros (the output of
    ReLU + dropout); the cast input is then packed once and the forward
    SpMMs gather from the packed copy (same bits, fewer bytes per edge).
    A tensor that does not qualify (``ops.kernels.packable``) is not
    packed. The backward SpMM gathers a dense GEMM output and never is."""

    @staticmethod
    def forward(ctx, x: Tensor, w1: Tensor, w2: Tensor, b1: Tensor,
                b2: Tensor, engine, layer: int, is_train: bool,
                pack: bool = False) -> Tensor:
        from ..ops.dist_agg import propagate
        from ..ops.kernels import pack_rows
        from ..helpers import PropagationMode
        num_inner = engine.graph.num_inner
        key = _agg_cache_key(ctx, engine, x, layer, is_train)
        h = _agg_cache_get(engine, key)
        if h is None:
            xa = x.to(engine.compute_dtype).contiguous()
            packed = pack_rows(xa) if pack else None
            kw = {} if packed is None else {'packed': packed}
            h = propagate(engine, xa, layer, is_train,
                          PropagationMode.Forward, **kw)
            _agg_cache_put(engine, key, x, h)
        xs = x[:num_inner].to(w1.dtype)
        ctx.engine, ctx.layer, ctx.in_dtype = engine, layer, x.dtype
        ctx.in_rows = x.shape[0]
        ctx.save_for_backward(xs, h, w1, w2)
        return torch.addmm(b1, xs, w1) + torch.addmm(b2, h, w2)

    @staticmethod
    def backward(ctx, g: Tensor):
        from ..ops.dist_agg import propagate
        from ..helpers import PropagationMode
        xs, h, w1, w2 = ctx.saved_tensors
        engine = ctx.engine
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            assert ctx.in_rows == engine.graph.num_inner
            gh = (g @ w2.t()).to(engine.compute_dtype).contiguous()
            gx_self = g @ w1.t()
            if gx_self.dtype == gh.dtype == ctx.in_dtype:
                gx = propagate(engine, gh, ctx.layer, True,
                               PropagationMode.Backward, addend=gx_self)
            else:
                gx = propagate(engine, gh, ctx.layer, True,
                               PropagationMode.Backward).to(ctx.in_dtype)
                gx.add_(gx_self)        # promotes gx_self: exact widening
        gw1 = xs.t() @ g if ctx.needs_input_grad[1] else None
        gw2 = h.t() @ g if ctx.needs_input_grad[2] else None
        gb = bias_grad(g) if (ctx.needs_input_grad[3]
                           or ctx.needs_input_grad[4]) else None
        return gx, gw1, gw2, gb, gb, None, None, None, None


def sage_mean_layer(engine, x: Tensor, lin1: 'FastLinear', lin2: 'FastLinear',
                    layer: int, is_train: bool, pack: bool = False) -> Tensor:
    """lin1(x[:num_inner]) + lin2(mean aggregation of x) through
    :class:`_SageMeanFn`; weight/bias casts mirror FastLinear.forward.
    ``pack``: hint that x is mostly zeros (see :class:`_SageMeanFn`)."""
    w1, w2, b1, b2 = lin1.weight, lin2.weight, lin1.bias, lin2.bias
    if torch.is_autocast_enabled('cuda') and x.is_cuda:
        dt = torch.get_autocast_dtype('cuda')
        w1, w2, b1, b2 = w1.to(dt), w2.to(dt), b1.to(dt), b2.to(dt)
    return _SageMeanFn.apply(x, w1, w2, b1, b2, engine, layer, is_train,
                             bool(pack))
