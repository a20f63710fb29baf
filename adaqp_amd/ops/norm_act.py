"""Fused LayerNorm -> ReLU -> dropout (the chain between two conv layers).

One definition, two implementations. For ``x [N,F]``, ``weight``/``bias``
``[F]`` fp32, ``eps``, ``p`` in [0,1), a seed and a ``training`` flag::

    mean_r = mean_f x[r,f]         var_r = mean_f (x[r,f]-mean_r)^2  (biased)
    rstd_r = 1/sqrt(var_r+eps)     z = (x-mean_r)*rstd_r*weight + bias
    keep[r,f] = uniform01(seed, r, f) >= float32(p)
    y = relu(z) * keep * s,        s = float32(1)/(float32(1)-float32(p))

with ``keep`` all true and ``s = 1`` in eval mode or at ``p == 0``.
``uniform01`` is the counter hash of ``ops/quant.py::uniform_noise`` (tag =
row index, feature index, low 32 bits of the seed), so the mask is the
same bits on CPU and GPU and backward recomputes it instead of storing it.

GPU, F <= 1024: the HIP kernels of ``csrc/norm_act.hip`` (2 passes over
``[N,F]`` forward, 3 backward; saves ``x`` plus 8 bytes per row). As in
``ops/kernels.py`` a missing extension is an error, never a fallback.
Everything else (CPU, F > 1024, float64) runs ``norm_relu_dropout_torch``,
which is also the test reference.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import quant as Q
from .kernels import native

MAX_FEATS = 1024          # register-staging limit of the HIP kernels
_M32 = 0xFFFFFFFF


def _check_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f'dropout p must be in [0, 1), got {p}')
    return p


def drop_scale(p: float) -> float:
    """s = float32(1) / (float32(1) - float32(p)), as a Python float."""
    pf = torch.tensor(_check_p(p), dtype=torch.float32)
    return float(torch.tensor(1.0, dtype=torch.float32) / (1.0 - pf))


def keep_mask(seed: int, n_rows: int, num_feats: int, p: float,
              device=None) -> Tensor:
    """bool [N, F]: uniform01(seed, row, feat) >= float32(p)."""
    rows = torch.arange(n_rows, dtype=torch.int64, device=device)
    u = Q.uniform_noise(int(seed) & _M32, rows, num_feats, device=device)
    return u >= torch.tensor(_check_p(p), dtype=torch.float32, device=device)


def bwd_launch_geometry():
    """(max blocks, waves per block) of the backward kernel's row grid: with
    more than their product rows, a wave visits more than one row."""
    C = native()
    return int(C.NORM_ACT_BWD_MAX_BLOCKS), int(C.NORM_ACT_WAVES_PER_BLOCK)


def norm_relu_dropout_torch(x: Tensor, weight: Tensor, bias: Tensor, p: float,
                            seed: int, training: bool,
                            eps: float = 1e-5) -> Tensor:
    """Plain differentiable torch implementation of the definition above
    (fp32 arithmetic; float64 for float64 input). The mask is built with
    ``quant.uniform_noise`` on ``x``'s device."""
    p = _check_p(p)
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(ct)
    mean = xf.mean(dim=1, keepdim=True)
    d = xf - mean
    var = (d * d).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = d * rstd * weight.to(ct) + bias.to(ct)
    y = torch.relu(z)
    if training and p > 0.0:
        keep = keep_mask(seed, x.shape[0], x.shape[1], p, device=x.device)
        y = y * keep.to(ct) * drop_scale(p)
    return y.to(x.dtype)


class _NormActFn(torch.autograd.Function):
    """HIP forward/backward. Saves x, mean, rstd, weight and bias only."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor, p: float,
                seed: int, training: bool, eps: float) -> Tensor:
        N = x.shape[0]
        y = torch.empty_like(x)
        need_stats = training or any(ctx.needs_input_grad[:3])
        n_stats = N if need_stats else 0
        mean = torch.empty(n_stats, dtype=torch.float32, device=x.device)
        rstd = torch.empty(n_stats, dtype=torch.float32, device=x.device)
        native().norm_act_fwd(x, weight, bias, eps, p, seed, training,
                              y, mean, rstd)
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.p, ctx.seed, ctx.training = p, seed, training
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, mean, rstd, weight, bias = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        dx = torch.empty_like(x)
        dwb = native().norm_act_bwd(dy, x, mean, rstd, weight, bias, ctx.p,
                                    ctx.seed, ctx.training, dx)
        return (dx if ctx.needs_input_grad[0] else None,
                dwb[0] if ctx.needs_input_grad[1] else None,
                dwb[1] if ctx.needs_input_grad[2] else None,
                None, None, None, None)


def norm_relu_dropout(x: Tensor, weight: Tensor, bias: Tensor, p: float,
                      seed: int, training: bool, eps: float = 1e-5) -> Tensor:
    """y = dropout(relu(layer_norm(x))) as defined in the module docstring.

    ``x`` [N,F] fp32 or bf16, contiguous; ``weight``/``bias`` fp32 [F];
    output in ``x``'s dtype. Works unchanged under
    ``torch.autocast('cuda', bfloat16)``: a bf16 ``x`` gives a bf16 ``y``
    and the fp32 parameters are read as they are (no cast kernels), so
    their grads are fp32."""
    p = _check_p(p)
    if x.dim() != 2:
        raise ValueError(f'x must be [N, F], got {tuple(x.shape)}')
    seed = int(seed) & _M32
    if (x.is_cuda and x.shape[1] <= MAX_FEATS
            and x.dtype in (torch.float32, torch.bfloat16)):
        return _NormActFn.apply(x, weight, bias, p, seed, bool(training),
                                float(eps))
    return norm_relu_dropout_torch(x, weight, bias, p, seed, training, eps)
