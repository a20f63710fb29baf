#!/usr/bin/env python3
"""Microbench of the inter-layer chain: the fused LayerNorm+ReLU+dropout
HIP pair against the torch chain the models run by default
(nn.LayerNorm -> relu -> nn.Dropout, under bf16 autocast for bf16).

Both paths run in one process, alternated call by call, timed with device
events after a warmup. Prints per path the median (min..max) time and the
achieved bytes/s from algorithmic byte counts:

  fused    forward  2 passes over [N,F] (read x, write y)
           backward 3 passes (read dy, read x, write dx)
  torch    forward  LN r+w, ReLU r+w, dropout r+w, + a byte mask
           backward dropout (g, mask -> g), ReLU (g, out -> g),
                    LN input grad (g, x -> dx), gamma/beta (g, x)

'eff' divides the FUSED byte count by the path's time, so the two paths
compare on the same numerator; 'own' uses the path's own count.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch

FLAGSHIP_ROWS = 2_449_029          # ogbn-products nodes (bench.py --gpus 1)


def byte_counts(N, F, es, mid):
    """Algorithmic bytes. es = element size of x/y; mid = element size of
    the torch chain's intermediates (4 under bf16 autocast: LayerNorm
    returns fp32 there)."""
    E = N * F
    fused_f = 2 * E * es
    fused_b = 3 * E * es
    torch_f = E * (es + mid) + 2 * E * mid + 2 * E * mid + E
    torch_b = (2 * E * mid + E) + 3 * E * mid + (E * mid + 2 * E * es) \
        + (E * mid + E * es)
    return fused_f, fused_b, torch_f, torch_b


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=FLAGSHIP_ROWS)
    p.add_argument('--F', type=int, default=256)
    p.add_argument('--p', type=float, default=0.5)
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', type=str, default='fp32,bf16')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('norm_bench needs a GPU: timings on a CPU say '
                         'nothing about the kernels')
    from adaqp_amd.ops.kernels import native
    from adaqp_amd.ops.norm_act import norm_relu_dropout
    native()
    dev = torch.device('cuda')
    N, F = args.rows, args.F
    print(f'{torch.cuda.get_device_name(0)}  N={N} F={F} p={args.p} '
          f'iters={args.iters} warmup={args.warmup}')

    for name in args.dtypes.split(','):
        dtype = {'fp32': torch.float32, 'bf16': torch.bfloat16}[name]
        bf16 = dtype == torch.bfloat16
        es, mid = (2, 4) if bf16 else (4, 4)
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(N, F, device=dev, generator=gen).to(dtype).requires_grad_(True)
        dy_f = torch.randn(N, F, device=dev, generator=gen).to(dtype)
        dy_by = {dtype: dy_f}
        if bf16:                     # the autocast chain returns fp32
            dy_by[torch.float32] = dy_f.float()
        ln = torch.nn.LayerNorm(F).to(dev)
        drop = torch.nn.Dropout(args.p)
        calls = [0]

        def fused():
            calls[0] += 1
            return norm_relu_dropout(x, ln.weight, ln.bias, args.p, calls[0], True)

        def chain():
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
                return drop(torch.relu(ln(x)))

        def fwd(path):
            with torch.no_grad():
                path()

        def fwd_bwd(path):
            x.grad = ln.weight.grad = ln.bias.grad = None
            y = path()
            y.backward(dy_by[y.dtype])

        fb = byte_counts(N, F, es, mid)
        for label, step, own in (('fwd', fwd, (fb[0], fb[2])),
                                 ('fwd+bwd', fwd_bwd,
                                  (fb[0] + fb[1], fb[2] + fb[3]))):
            paths = (('fused', fused, own[0]), ('torch', chain, own[1]))
            for _ in range(args.warmup):
                for _, path, _ in paths:
                    step(path)
            torch.cuda.synchronize()
            times = {n: [] for n, _, _ in paths}
            for _ in range(args.iters):
                for n, path, _ in paths:          # alternate the two paths
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(path)
                    e1.record()
                    e1.synchronize()
                    times[n].append(e0.elapsed_time(e1) * 1e-3)
            for n, _, own_bytes in paths:
                t = times[n]
                med = statistics.median(t)
                print(f'{name:4s} {label:8s} {n:5s}: {med*1e3:8.3f} ms '
                      f'({min(t)*1e3:.3f}..{max(t)*1e3:.3f})  '
                      f'eff {own[0]/med/1e12:5.2f} TB/s  '
                      f'own {own_bytes/med/1e12:5.2f} TB/s')
            sp = statistics.median(times['torch']) / statistics.median(times['fused'])
            print(f'{name:4s} {label:8s} torch/fused = {sp:.2f}x')
            sys.stdout.flush()
        del x, dy_f, dy_by
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
