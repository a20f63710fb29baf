#!/usr/bin/env python3
"""Microbench of the training loss: the fused masked-loss HIP pair
(``ops.loss.masked_loss``) against the torch chain ``compute_loss`` runs by
default (boolean-index gather, F.cross_entropy / BCE-with-logits with
reduction='sum', and their backward with its index_put).

Both paths run forward plus backward in one process, alternated call by
call, timed with device events after a warmup. The torch path's timed
region holds its host syncs (the ``nonzero`` behind each boolean index), as
an epoch does. Prints per path the median (min..max) time and, for the
fused path, the achieved bytes/s from the algorithmic byte count:

  forward   masked rows of z (+ y, multilabel) read once, 8 B per masked
            row written (single-label)
  backward  masked rows of z (+ y) read once, all of dz written once

Shapes: the flagship's 2.45 M x 47 single-label in fp32 and bf16, and the
yelp shape 717 k x 100 multilabel; mask density 0.66.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch
import torch.nn.functional as F

SHAPES = (          # name, rows, classes, multilabel, dtype
    ('products fp32', 2_449_029, 47, False, torch.float32),
    ('products bf16', 2_449_029, 47, False, torch.bfloat16),
    ('yelp fp32', 716_847, 100, True, torch.float32),
)


def fused_bytes(N, C, n_masked, es, multilabel):
    rows = n_masked * C * es + (n_masked * C * 4 if multilabel else 0)
    fwd = rows + N + (0 if multilabel else n_masked * (8 + 8))
    bwd = rows + N + N * C * es + (0 if multilabel else n_masked * (8 + 8))
    return fwd + bwd


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--density', type=float, default=0.66)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench needs a GPU: timings on a CPU say '
                         'nothing about the kernels')
    from adaqp_amd.ops.kernels import native
    from adaqp_amd.ops.loss import masked_loss
    native()
    dev = torch.device('cuda')
    print(f'{torch.cuda.get_device_name(0)}  density={args.density} '
          f'iters={args.iters} warmup={args.warmup}')

    for name, N, C, multilabel, dtype in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        z = (torch.randn(N, C, device=dev, generator=gen) * 4).to(dtype)
        z.requires_grad_(True)
        mask = torch.rand(N, device=dev, generator=gen) < args.density
        if multilabel:
            labels = (torch.rand(N, C, device=dev, generator=gen) < 0.1).float()
        else:
            labels = torch.randint(0, C, (N,), device=dev, generator=gen)
        count = mask.sum().float().reshape(1)
        n_masked = int(count)

        def fused():
            return masked_loss(z, labels, mask, multilabel) / count

        def chain():
            # what train_epoch + compute_loss run with the switch off
            zf = z.float()
            if multilabel:
                raw = F.binary_cross_entropy_with_logits(
                    zf[mask], labels[mask].float(), reduction='sum') / C
            else:
                raw = F.cross_entropy(zf[mask], labels[mask], reduction='sum')
            return raw / count

        def step(path):
            z.grad = None
            loss = path()
            loss.backward()
            return loss

        paths = (('fused', fused), ('torch', chain))
        got = {}
        for _ in range(args.warmup):
            for n, path in paths:
                got[n] = (float(step(path).detach()), z.grad.float().clone())
        torch.cuda.synchronize()
        dl = abs(got['fused'][0] - got['torch'][0])
        dg = float((got['fused'][1] - got['torch'][1]).abs().max())
        times = {n: [] for n, _ in paths}
        for _ in range(args.iters):
            for n, path in paths:                 # alternate the two paths
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                step(path)
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e-3)
        nbytes = fused_bytes(N, C, n_masked, z.element_size(), multilabel)
        print(f'{name}: N={N} C={C} masked={n_masked}  '
              f'|loss diff| {dl:.3e}  max |grad diff| {dg:.3e}')
        for n, _ in paths:
            t = times[n]
            med = statistics.median(t)
            rate = (f'  {nbytes/med/1e12:5.2f} TB/s of {nbytes/1e9:.2f} GB'
                    if n == 'fused' else '')
            print(f'  fwd+bwd {n:5s}: {med*1e3:8.3f} ms '
                  f'({min(t)*1e3:.3f}..{max(t)*1e3:.3f}){rate}')
        sp = statistics.median(times['torch']) / statistics.median(times['fused'])
        print(f'  torch/fused = {sp:.2f}x')
        sys.stdout.flush()
        del z, labels, mask, got
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
