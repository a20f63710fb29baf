"""Float64 oracles and counted-rounding checkers for the fused
LayerNorm -> ReLU -> dropout op (no GPU code; same conventions as
``kernel_oracles.py``).

Every checker takes an implementation's outputs as CPU tensors,
recomputes the op in float64 from the exact inputs and raises
``AssertionError`` naming the first offending index. No tolerance is
sized from an output under test: each bound counts fp32 roundings,
``u = 2^-24`` relative each, to first order, and the final factor 2 covers
second-order terms and the choice of reduction tree.

Forward bound (float64 quantities ``m`` = row mean, ``d = x - m``,
``var``, ``r = 1/sqrt(var+eps)``, ``xhat = d*r``, ``z = xhat*w + b``)::

    Em  = (F+1)*u*mean|x|                  row sum in any order + divide
    rho = (F/2+8)*u + Em^2/(2(var+eps))    var sum, +eps, sqrt, divide
    dxh = r*(Em + u|d|) + |xhat|*(rho+u)   error of the fp32 xhat
    dz  = |w|*dxh + 2u(|xhat*w| + |b|)     error of the fp32 z
    tol = 2*(s*dz + 2u|y_ref|)   [+ bf16_half_ulp(|y_ref|+tol), bf16 out]

``mean`` and ``rstd`` are checked with ``Em`` and ``rho*r``.

Backward bound: see ``check_norm_act_bwd``.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch
from torch import Tensor

from adaqp_amd.ops import quant as Q
from adaqp_amd.ops.norm_act import drop_scale

from kernel_oracles import U32, _first, bf16_half_ulp

FREE_GATE_CAP = 0.01      # at most 1 % of a test input may be free gates


class _Ref:
    """Float64 forward quantities + first-order fp32 error bounds."""

    def __init__(self, x: Tensor, weight: Tensor, bias: Tensor, p: float,
                 seed: int, training: bool, eps: float):
        assert x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16), \
            (x.shape, x.dtype)
        assert weight.dtype == torch.float32 and bias.dtype == torch.float32
        N, F = x.shape
        u = U32
        self.N, self.F = N, F
        x64 = x.double()
        w = weight.double()[None, :]
        b = bias.double()[None, :]
        self.w, self.b = w, b
        self.m = x64.mean(dim=1, keepdim=True) if F else x64.sum(1, keepdim=True)
        self.d = x64 - self.m
        self.var = (self.d * self.d).mean(dim=1, keepdim=True)
        self.r = 1.0 / torch.sqrt(self.var + eps)
        self.xhat = self.d * self.r
        self.z = self.xhat * w + b
        masked = bool(training) and float(p) > 0.0
        if masked:
            pf = torch.tensor(float(p), dtype=torch.float32)
            rows = torch.arange(N, dtype=torch.int64)
            self.keep = Q.uniform_noise(int(seed) & 0xFFFFFFFF, rows, F) >= pf
            self.s = drop_scale(p)          # float32(1)/(1 - float32(p))
        else:
            self.keep = torch.ones(N, F, dtype=torch.bool)
            self.s = 1.0
        self.y = torch.relu(self.z) * self.keep * self.s
        # bounds
        self.Em = (F + 1) * u * x64.abs().mean(dim=1, keepdim=True)
        self.rho = (F / 2 + 8) * u + self.Em ** 2 / (2 * (self.var + eps))
        self.dxh = self.r * (self.Em + u * self.d.abs()) \
            + self.xhat.abs() * (self.rho + u)
        self.dz = w.abs() * self.dxh + 2 * u * ((self.xhat * w).abs() + b.abs())


def check_norm_act_fwd(x: Tensor, weight: Tensor, bias: Tensor, p: float,
                       seed: int, training: bool, y: Tensor,
                       mean: Optional[Tensor] = None,
                       rstd: Optional[Tensor] = None,
                       eps: float = 1e-5) -> None:
    """y [N,F] in x's dtype; mean/rstd fp32 [N] if given. Dropped elements
    must be exactly 0; kept ones within ``tol`` of the float64 oracle."""
    ref = _Ref(x, weight, bias, p, seed, training, eps)
    assert y.shape == x.shape and y.dtype == x.dtype, (y.shape, y.dtype)
    o = y.cpu().double()
    tol = 2 * (ref.s * ref.dz + 2 * U32 * ref.y.abs())
    if y.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(ref.y.abs() + tol)
    dropped = ~ref.keep
    bad = dropped & (o != 0)
    if bad.any():
        i, f = _first(bad)
        raise AssertionError(
            f'y[{i}, {f}] = {float(o[i, f])!r} but the element is dropped '
            f'(p={p}, seed={seed}); {int(bad.sum())} of {int(dropped.sum())} '
            f'dropped elements are non-zero')
    bad = ref.keep & ~((o - ref.y).abs() <= tol)
    if bad.any():
        i, f = _first(bad)
        raise AssertionError(
            f'y[{i}, {f}] = {float(o[i, f])!r}, oracle {float(ref.y[i, f])!r} '
            f'(tol {float(tol[i, f]):.3e}, z {float(ref.z[i, f])!r}, s {ref.s!r}, '
            f'F={ref.F}, p={p}, {y.dtype}); {int(bad.sum())} bad of {o.numel()}')
    for name, got, exp, bound in (
            ('mean', mean, ref.m, ref.Em), ('rstd', rstd, ref.r, ref.rho * ref.r)):
        if got is None:
            continue
        assert got.dtype == torch.float32 and got.shape == (ref.N,), \
            (name, got.dtype, got.shape)
        g = got.cpu().double()[:, None]
        bad = ~((g - exp).abs() <= bound)
        if bad.any():
            i = _first(bad)[0]
            raise AssertionError(
                f'{name}[{i}] = {float(g[i, 0])!r}, oracle {float(exp[i, 0])!r} '
                f'(bound {float(bound[i, 0]):.3e}, F={ref.F})')


def check_norm_act_bwd(x: Tensor, weight: Tensor, bias: Tensor, p: float,
                       seed: int, training: bool, dy: Tensor, dx: Tensor,
                       dweight: Tensor, dbias: Tensor,
                       eps: float = 1e-5) -> None:
    """dy, dx [N,F] in x's dtype; dweight, dbias fp32 [F].

    Oracle (float64): ``g = dy*s*gate`` with ``gate = z > 0 && keep``,
    ``a = g*w``, ``m1 = mean_f a``, ``m2 = mean_f(a*xhat)``,
    ``dx = r*(a - m1 - xhat*m2)``, ``dweight = sum_r g*xhat``,
    ``dbias = sum_r g``.

    Roundings counted (first order, ``u`` each; ``dxh`` and ``rho`` are the
    forward bounds, since backward recomputes ``xhat`` from fp32 ``mean``
    and ``rstd``)::

        g' = fl(dy*s)                    1 rounding            u|g|
        a' = fl(g'*w)                    + 1                   2u|a|
        m1: sum of F a' in any order     (F-1)u mean|a| + the 2u above
            + divide                     dm1 = (F+2)*u*mean|a|
        m2: terms a'*xhat'               |a|*dxh + 3u|a*xhat| each,
            sum in any order + divide    dm2 = mean(|a|*dxh) + (F+3)*u*mean|a*xhat|
        t = a - m1 - xhat*m2             dt = 2u|a| + dm1 + |xhat|*dm2 + |m2|*dxh
                                              + 3u(|a| + |m1| + |xhat*m2|)
                                         (product, two subtractions)
        dx = r*t                         r*dt + |dx_ref|*(rho + u)
        tol_dx = 2*(r*dt + |dx_ref|*(rho+u))    [+ bf16 half ulp, bf16 out]

        dweight_f: N terms g'*xhat', each |g|*dxh + 2u|g*xhat| off, summed
            in any order over N rows: N*u*sum_r|g*xhat|
        tol_dw = 2*(sum_r(|g|*dxh + 2u|g*xhat|) + N*u*sum_r|g*xhat|)
        tol_db = 2*(N+1)*u*sum_r|g|

    Free gates. ReLU's gate is discontinuous: where the fp32 ``z`` may land
    on either side of 0, i.e. ``-dz < z_ref <= dz`` (a tie at ``dz == 0``
    is computed exactly and is NOT free), an implementation may gate the
    element either way. Each such kept element (r, j) widens the
    tolerances by its largest possible influence, with
    ``delta = |dy*s*w|_j``: on ``dx[r,i]`` by
    ``r*delta*([i=j] + (1 + |xhat_i*xhat_j|)/F)``, on ``dweight_j`` by
    ``|dy*s*xhat|`` and on ``dbias_j`` by ``|dy*s|``. Free gates may be at
    most 1 % of the elements (``FREE_GATE_CAP``); the checker raises beyond
    that, so a test input cannot hide errors behind them.
    """
    ref = _Ref(x, weight, bias, p, seed, training, eps)
    N, F, u = ref.N, ref.F, U32
    assert dy.shape == x.shape and dy.dtype == x.dtype, (dy.shape, dy.dtype)
    assert dx.shape == x.shape and dx.dtype == x.dtype, (dx.shape, dx.dtype)
    for t in (dweight, dbias):
        assert t.shape == (F,) and t.dtype == torch.float32, (t.shape, t.dtype)
    w, r, xhat, s = ref.w, ref.r, ref.xhat, ref.s
    g_full = dy.cpu().double() * s                # dy*s before gating
    gate = (ref.z > 0) & ref.keep
    g = g_full * gate
    a = g * w
    m1 = a.mean(dim=1, keepdim=True)
    m2 = (a * xhat).mean(dim=1, keepdim=True)
    t_ref = a - m1 - xhat * m2
    dx_ref = r * t_ref
    dw_ref = (g * xhat).sum(dim=0)
    db_ref = g.sum(dim=0)

    dm1 = (F + 2) * u * a.abs().mean(dim=1, keepdim=True)
    dm2 = (a.abs() * ref.dxh).mean(dim=1, keepdim=True) \
        + (F + 3) * u * (a * xhat).abs().mean(dim=1, keepdim=True)
    dt = 2 * u * a.abs() + dm1 + xhat.abs() * dm2 + m2.abs() * ref.dxh \
        + 3 * u * (a.abs() + m1.abs() + (xhat * m2).abs())
    tol_dx = 2 * (r * dt + dx_ref.abs() * (ref.rho + u))
    tol_dw = 2 * ((g.abs() * ref.dxh + 2 * u * (g * xhat).abs()).sum(dim=0)
                  + N * u * (g * xhat).abs().sum(dim=0))
    tol_db = 2 * (N + 1) * u * g.abs().sum(dim=0)

    free = ref.keep & (ref.z > -ref.dz) & (ref.z <= ref.dz)
    n_free = int(free.sum())
    if n_free > FREE_GATE_CAP * max(N * F, 1):
        i, f = _first(free)
        raise AssertionError(
            f'{n_free} of {N * F} elements are free ReLU gates (|z| within '
            f'the fp32 error of z), more than {FREE_GATE_CAP:.0%}: first at '
            f'[{i}, {f}], z = {float(ref.z[i, f])!r}, dz = '
            f'{float(ref.dz[i, f]):.3e}')
    if n_free:
        delta = (g_full * w).abs() * free
        tol_dx = tol_dx + r * (
            delta + (delta.sum(dim=1, keepdim=True) + xhat.abs()
                     * (delta * xhat.abs()).sum(dim=1, keepdim=True)) / F)
        tol_dw = tol_dw + ((g_full * xhat).abs() * free).sum(dim=0)
        tol_db = tol_db + (g_full.abs() * free).sum(dim=0)
    if dx.dtype == torch.bfloat16:
        tol_dx = tol_dx + bf16_half_ulp(dx_ref.abs() + tol_dx)

    o = dx.cpu().double()
    bad = ~((o - dx_ref).abs() <= tol_dx)
    if bad.any():
        i, f = _first(bad)
        raise AssertionError(
            f'dx[{i}, {f}] = {float(o[i, f])!r}, oracle {float(dx_ref[i, f])!r} '
            f'(tol {float(tol_dx[i, f]):.3e}, N={N}, F={F}, p={p}, {dx.dtype}, '
            f'{n_free} free gates); {int(bad.sum())} bad of {o.numel()}')
    for name, got, exp, tol in (('dweight', dweight, dw_ref, tol_dw),
                                ('dbias', dbias, db_ref, tol_db)):
        gt = got.cpu().double()
        bad = ~((gt - exp).abs() <= tol)
        if bad.any():
            f = _first(bad)[0]
            raise AssertionError(
                f'{name}[{f}] = {float(gt[f])!r}, oracle {float(exp[f])!r} '
                f'(tol {float(tol[f]):.3e}, N={N}, F={F}, p={p}, '
                f'{n_free} free gates); {int(bad.sum())} bad of {F}')


# --------------------------------------------------------------------------
# shared inputs (CPU tensors, fixed generators)
# --------------------------------------------------------------------------

NORM_FS = (1, 2, 17, 100, 256, 602, 1024)     # every VE, idle lanes, the limit
NORM_F_TORCH = 1030                           # past the kernels' limit
NORM_PS = (0.0, 0.5, 0.9)
NORM_N = 37                                   # last block partial
NORM_SEED = 2 ** 32 + 977                     # exercises the low-32-bit rule
CONST_ROW, SMALL_ROW, OFFSET_ROW = 1, 2, 3
CONST_VALUE = 0.75


@functools.lru_cache(maxsize=None)
def norm_case(N: int, F: int, dtype=torch.float32):
    """(x [N,F] dtype, weight [F], bias [F], dy [N,F] dtype) — do not modify.

    Rows have scale 10^U(-1,1) and offset 2*scale*N(0,1). Row 1 is constant
    (var = 0, output relu(bias)*keep*s), row 2 is scaled by 1e-3 (eps
    matters) and row 3 has offset 1e3 with unit spread (breaks a one-pass
    variance); row 3 is only placed when N >= 16, because up to ~5 % of
    its gates are free and a smaller input would exceed the 1 % cap.
    weight has both signs with |w| in [0.5, 1.5); |bias| in [0.25, 0.75)
    with both signs, so the constant row has no free gates."""
    gen = torch.Generator().manual_seed(4000 + 7 * N + F)
    scale = 10.0 ** (torch.rand(N, 1, generator=gen) * 2 - 1)
    offset = 2 * scale * torch.randn(N, 1, generator=gen)
    x = torch.randn(N, F, generator=gen) * scale + offset
    if N > CONST_ROW:
        x[CONST_ROW] = CONST_VALUE
    if N > SMALL_ROW:
        x[SMALL_ROW] = torch.randn(F, generator=gen) * 1e-3
    if N >= 16:
        x[OFFSET_ROW] = torch.randn(F, generator=gen) + 1e3

    def signed(lo, width):
        sign = torch.where(torch.rand(F, generator=gen) < 0.5, -1.0, 1.0)
        return sign * (lo + width * torch.rand(F, generator=gen))
    weight = signed(0.5, 1.0)
    bias = signed(0.25, 0.5)
    dy = torch.randn(N, F, generator=gen)
    return x.to(dtype), weight, bias, dy.to(dtype)
