"""Masked training loss: softmax cross-entropy (single-label) or
BCE-with-logits (multilabel) summed over the rows a bool mask selects.

One definition, two implementations. For ``logits`` z ``[N, C]`` (fp32 or
bf16), ``mask`` bool ``[N]`` and an upstream scalar gradient ``g``::

    single-label, labels int64 [N]:
        m_r = max_c z[r,c]        lse_r = m_r + log sum_c exp(z[r,c] - m_r)
        loss = sum_{r: mask[r]} (lse_r - z[r, labels[r]])
        dz[r,c] = g * (softmax(z_r)_c - [c == labels[r]])
    multilabel, labels fp32 [N, C] with targets in [0, 1]:
        loss = (1/C) sum_{r: mask[r]} sum_c (max(z,0) - z*y + log1p(exp(-|z|)))
        dz[r,c] = (g/C) * (sigmoid(z) - y)
    rows with mask[r] == False: never used (NaN or inf there reaches
    nothing); their dz is exactly +0.0.

The result is the raw sum as a 0-dim fp32 tensor (``compute_loss`` divides
by the global train count). All arithmetic is fp32; ``dz`` has the dtype of
``logits``, a bf16 ``dz`` being the fp32 value rounded once. A class with
``y == 0`` contributes no ``z*y`` term, so ``z = -inf`` there gives its
limit 0. A single-label row whose label is outside ``[0, C)`` contributes
NaN to the loss and is never used as an index.

GPU, C <= 1024: the HIP kernels of ``csrc/masked_loss.hip``. Forward reads
only the masked rows and saves 8 bytes per row (single-label) or nothing
(multilabel); backward is one pass that writes every element of ``dz``
and reads ``g`` on the device, so the op never syncs the host. The loss is
summed in a fixed order without atomics: the same input gives the same
bits. As in ``ops/kernels.py`` a missing extension is an error, never a
fallback. Everything else (CPU, C > 1024, float64) runs
``masked_loss_torch``, which is also the test reference.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .kernels import native

MAX_CLASSES = 1024        # widest row the HIP kernels take
calls = 0                 # times masked_loss was entered (tests read this)


def resolve_fused_loss(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_FUSED_LOSS=1``; an explicit bool wins."""
    if flag is None:
        return os.environ.get('ADAQP_FUSED_LOSS') == '1'
    return bool(flag)


def launch_geometry(num_classes: int) -> Tuple[int, int]:
    """(max blocks, rows a block handles per trip of its row loop) of the
    HIP kernels for ``num_classes``: with more than their product rows, a
    block makes a second trip."""
    C = native()
    return (int(C.MASKED_LOSS_MAX_BLOCKS),
            int(C.masked_loss_rows_per_block(int(num_classes))))


def _check(logits: Tensor, labels: Tensor, mask: Tensor, multilabel: bool):
    if logits.dim() != 2:
        raise ValueError(f'logits must be [N, C], got {tuple(logits.shape)}')
    N, C = logits.shape
    if mask.dtype != torch.bool or tuple(mask.shape) != (N,):
        raise ValueError(f'mask must be bool [{N}], got {mask.dtype} '
                         f'{tuple(mask.shape)}')
    want = (N, C) if multilabel else (N,)
    if tuple(labels.shape) != want:
        raise ValueError(f'labels must be {list(want)}, got '
                         f'{tuple(labels.shape)}')


def masked_loss_torch(logits: Tensor, labels: Tensor, mask: Tensor,
                      multilabel: bool) -> Tensor:
    """Plain differentiable torch implementation of the definition above
    (fp32 arithmetic; float64 for float64 input), with a ``where`` on the
    mask instead of boolean indexing."""
    _check(logits, labels, mask, multilabel)
    ct = torch.float64 if logits.dtype == torch.float64 else torch.float32
    C = logits.shape[1]
    zero = torch.zeros((), dtype=ct, device=logits.device)
    # unmasked rows become zeros before any arithmetic sees them
    z = torch.where(mask[:, None], logits.to(ct), zero)
    if multilabel:
        y = labels.to(ct)
        zy = torch.where(y == 0, zero, z * y)
        term = z.clamp_min(0) - zy + torch.log1p(torch.exp(-z.abs()))
        return torch.where(mask[:, None], term, zero).sum() / C
    # as the kernels: the row max, then exp(z - m) / s in backward. A
    # gradient through lse alone would round the exponent to |lse| * 2^-24
    m = z.detach().max(dim=1, keepdim=True).values
    lse = m.squeeze(1) + torch.log(torch.exp(z - m).sum(dim=1))
    valid = (labels >= 0) & (labels < C)
    picked = z.gather(1, labels.clamp(0, max(C - 1, 0))[:, None]).squeeze(1)
    nan = torch.full((), float('nan'), dtype=ct, device=logits.device)
    zy = torch.where(valid, picked, nan)
    return torch.where(mask, lse - zy, zero).sum()


class _MaskedLossFn(torch.autograd.Function):
    """HIP forward/backward. Saves logits, labels, mask and the per-row
    (max, exp sum) pairs of the single-label forward."""

    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor, mask: Tensor,
                multilabel: bool) -> Tensor:
        loss, stats = native().masked_loss_fwd(logits, labels, mask, multilabel)
        ctx.save_for_backward(logits, labels, mask, stats)
        ctx.multilabel = multilabel
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        logits, labels, mask, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        # g stays on the device: the kernel reads it
        g = g.to(torch.float32).contiguous()
        dz = native().masked_loss_bwd(logits, labels, mask, stats, g,
                                      ctx.multilabel)
        return dz, None, None, None


def masked_loss(logits: Tensor, labels: Tensor, mask: Tensor,
                multilabel: bool) -> Tensor:
    """The masked loss sum defined in the module docstring.

    ``logits`` [N, C] fp32 or bf16 (made contiguous if it is not);
    ``labels`` int64 [N] or, multilabel, fp32 [N, C] targets;
    ``mask`` bool [N]. Returns a 0-dim fp32 tensor.

    Labels of the stated dtype are read in place. Any other dtype is
    converted on every call, for multilabel targets a full [N, C] copy:
    store them as fp32 (the graph loaders do)."""
    global calls
    calls += 1
    multilabel = bool(multilabel)
    _check(logits, labels, mask, multilabel)
    if (logits.is_cuda and 1 <= logits.shape[1] <= MAX_CLASSES
            and logits.dtype in (torch.float32, torch.bfloat16)):
        labels = (labels.to(torch.float32) if multilabel
                  else labels.to(torch.int64))
        return _MaskedLossFn.apply(logits.contiguous(), labels.contiguous(),
                                   mask.contiguous(), multilabel)
    return masked_loss_torch(logits, labels, mask, multilabel)
