"""Float64 oracle, input generator and bound checkers for the masked loss
(``adaqp_amd.ops.loss``). No GPU code.

The oracle computes the loss and its gradient in float64 from the input
widened exactly, with boolean indexing (the definition's own words). A
checker takes an implementation's output as a CPU tensor and raises
``AssertionError`` with the worst error as a share of its bound. No bound
is sized from an output under test. With ``u = 2^-24`` (fp32 unit
roundoff), n masked rows and upstream gradient g::

    CE  gradient  |dz^ - dz| <= (C + 8) u |g|            per element
    CE  loss      |L^ - L|   <= (n + C + 16) u sum_masked(|lse_r| + |z[r,y_r]|)
    BCE gradient  |dz^ - dz| <= 8 u |g| / C              per element
    BCE loss      |L^ - L|   <= (n C + 8) u (1/C) sum_masked sum_c
                                (|z| + log1p(exp(-|z|)))
    bf16 gradient the fp32 bound + half a bf16 ulp of dz

Half a bf16 ulp is 2^(e-8) for 2^e <= |dz| < 2^(e+1), between 2^-9 |dz| and
2^-8 |dz|: the one rounding ``f32_to_bf16`` applies to an fp32 value inside
the fp32 bound. A flat 2^-9 |dz| would refuse correctly rounded results in
the lower half of every binade (``kernel_oracles.bf16_half_ulp``).

They hold for any summation order: gamma_C covers the softmax denominator
and the remaining 8 the subtraction, ``exp``, the divide, the one-hot and
the product (accurate ``expf``/``logf``/``log1pf`` assumed); gamma_n and
gamma_{nC} cover the sum over rows. An infinite logit in a masked row adds
nothing to the BCE loss scale (its own term is exactly 0 or infinite).
Unmasked rows of a gradient must be +0.0 bit for bit, and every checked
value must be finite.
"""
from __future__ import annotations

import functools
from typing import Tuple

import torch
from torch import Tensor

from kernel_oracles import U32, bf16_half_ulp

LOSS_SEED = 20261
# every C at which the kernels take another path: one class, below / at /
# above one wavefront, the datasets' odd widths, two and three trips of
# the class loop, the widest row the kernels take
LOSS_CS = (1, 2, 47, 64, 65, 107, 128, 129, 1024)
LOSS_C_TORCH = 1025       # above the kernels' limit: the torch definition
LOSS_NS = (1, 63, 64, 65, 257)
LOSS_G = -1.75            # upstream gradient of the tests, not 1


@functools.lru_cache(maxsize=None)
def loss_case(N: int, C: int, multilabel: bool, dtype: torch.dtype,
              density: float = 0.66, scale: float = 8.0,
              extremes: bool = True,
              seed: int = LOSS_SEED) -> Tuple[Tensor, Tensor, Tensor]:
    """(logits [N,C] in ``dtype``, labels, mask) on the CPU, cached and
    never modified by a test. ``density`` 0 / 1 give the all-false /
    all-true mask. ``extremes`` plants, in masked rows, a logit of 1e4 in
    a non-label class, one of -1e4 in the label class and a -inf in a
    non-label class; in unmasked rows NaN, +inf and -inf logits and, for
    the single-label loss, labels far outside [0, C)."""
    g = torch.Generator().manual_seed(seed + 7919 * N + 31 * C + int(multilabel))
    z = torch.randn(N, C, generator=g) * scale
    if density <= 0:
        mask = torch.zeros(N, dtype=torch.bool)
    elif density >= 1:
        mask = torch.ones(N, dtype=torch.bool)
    else:
        mask = torch.rand(N, generator=g) < density
    if multilabel:
        labels = (torch.rand(N, C, generator=g) < 0.3).float()
        soft = torch.rand(N, C, generator=g)
        labels = torch.where(torch.rand(N, C, generator=g) < 0.05, soft, labels)
    else:
        labels = torch.randint(0, C, (N,), generator=g)
    if extremes:
        on = torch.nonzero(mask).flatten().tolist()
        off = torch.nonzero(~mask).flatten().tolist()
        plant = [(1e4, False), (-1e4, True), (float('-inf'), False)]
        for r, (val, at_label) in zip(on, plant):
            if multilabel:
                c = (r + 1) % C
                labels[r, c] = 1.0 if at_label else 0.0
            else:
                y = int(labels[r])
                if not at_label and C == 1:
                    if val == float('-inf'):
                        continue            # no non-label class to hold it
                    c = 0
                else:
                    c = y if at_label else (y + 1) % C
            z[r, c] = val
        for r, val in zip(off, (float('nan'), float('inf'), float('-inf'))):
            z[r, r % C] = val
        if not multilabel:
            for r, val in zip(off, (10 ** 12, -5, C)):
                labels[r] = val
    return z.to(dtype), labels, mask


def oracle(logits: Tensor, labels: Tensor, mask: Tensor, multilabel: bool,
           g: float = 1.0):
    """-> (loss, dz [N,C], loss_scale, n) in float64 from the exact inputs.
    ``loss_scale`` is the sum the loss bound multiplies."""
    assert logits.dtype in (torch.float32, torch.bfloat16), logits.dtype
    N, C = logits.shape
    z = logits.double()[mask]
    n = int(mask.sum())
    dz = torch.zeros(N, C, dtype=torch.float64)
    if multilabel:
        y = labels.double()[mask]
        zy = torch.where(y == 0, torch.zeros_like(z), z * y)
        soft = torch.log1p(torch.exp(-z.abs()))
        loss = (z.clamp_min(0) - zy + soft).sum() / C
        dz[mask] = (g / C) * (torch.sigmoid(z) - y)
        mag = torch.where(torch.isinf(z), torch.zeros_like(z), z.abs() + soft)
        scale = mag.sum() / C
    else:
        y = labels[mask]
        assert n == 0 or (int(y.min()) >= 0 and int(y.max()) < C), \
            'the oracle takes valid labels in masked rows'
        lse = torch.logsumexp(z, dim=1)
        zy = z.gather(1, y[:, None]).squeeze(1)
        loss = (lse - zy).sum()
        p = torch.exp(z - lse[:, None])
        p[torch.arange(n), y] -= 1.0
        dz[mask] = g * p
        scale = (lse.abs() + zy.abs()).sum()
    return loss, dz, scale, n


def loss_bound(logits: Tensor, labels: Tensor, mask: Tensor,
               multilabel: bool) -> float:
    _, _, scale, n = oracle(logits, labels, mask, multilabel)
    C = logits.shape[1]
    k = (n * C + 8) if multilabel else (n + C + 16)
    return k * U32 * float(scale)


def check_loss(logits: Tensor, labels: Tensor, mask: Tensor, multilabel: bool,
               loss_hat: Tensor, extra: float = 0.0) -> float:
    """``loss_hat``: the raw sum an implementation returned. ``extra`` is
    added to the bound for roundings the caller applied on top (stated
    where used). Returns the error as a share of the bound."""
    ref, _, _, n = oracle(logits, labels, mask, multilabel)
    got = float(loss_hat.detach().double().cpu())
    assert got == got and abs(got) != float('inf'), f'loss is {got}'
    bound = loss_bound(logits, labels, mask, multilabel) + extra
    err = abs(got - float(ref))
    if n == 0:
        assert got == 0.0 and str(got) == '0.0', f'empty mask: loss {got!r}'
    assert err <= bound, (f'loss {got!r} vs oracle {float(ref)!r}: error '
                          f'{err:.3e} > bound {bound:.3e}')
    return err / bound if bound else 0.0


def check_grad(logits: Tensor, labels: Tensor, mask: Tensor, multilabel: bool,
               g: float, dz_hat: Tensor) -> float:
    """``dz_hat``: d(loss * g)/d logits as the implementation returned it,
    in logits' dtype. Returns the worst error as a share of its bound."""
    assert dz_hat.shape == logits.shape and dz_hat.dtype == logits.dtype, \
        (dz_hat.shape, dz_hat.dtype)
    _, ref, _, _ = oracle(logits, labels, mask, multilabel, g)
    C = logits.shape[1]
    got = dz_hat.detach().cpu()
    off = got[~mask]
    bits = off.view(torch.int32 if got.dtype == torch.float32 else torch.int16)
    assert not bits.any(), 'an unmasked row of dz is not +0.0 bit for bit'
    d = got.double()[mask]
    r = ref[mask]
    assert torch.isfinite(d).all(), 'non-finite dz in a masked row'
    tol = torch.full_like(r, (8.0 / C if multilabel else C + 8.0) * U32 * abs(g))
    if got.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(r.abs() + tol)
    err = (d - r).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        raise AssertionError(
            f'dz[masked {i}] = {float(d[tuple(i)])!r} vs oracle '
            f'{float(r[tuple(i)])!r}: error {float(err[tuple(i)]):.3e} > '
            f'bound {float(tol[tuple(i)]):.3e}')
    return float((err / tol).max()) if err.numel() else 0.0
