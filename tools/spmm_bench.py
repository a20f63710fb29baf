#!/usr/bin/env python3
"""Self-contained SpMM microbench (no partition machinery, safe under
rocprofv3). Builds a products-like CSR directly on the GPU and times the
spmm_csr kernel; prints effective gather TB/s.

``--wave-index`` picks the SW == 64 kernel (0 = per-lane index kernel,
1 = wave-uniform index kernel; default: the library's). Both
(``--wave-index 0,1``) are alternated call by call and each is reported
as median (min..max) of per-call device-event times, after checking that
they produce the same bits."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch


def build_csr(rows, deg_mean, n_cols, device, seed=0, hub_frac=0.001):
    g = torch.Generator(device='cpu').manual_seed(seed)
    deg = torch.full((rows,), deg_mean, dtype=torch.int64)
    nhub = max(int(rows * hub_frac), 1)
    deg[torch.randperm(rows, generator=g)[:nhub]] = deg_mean * 100
    indptr = torch.zeros(rows + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    E = int(indptr[-1])
    # clustered columns: around the row's own neighborhood
    r = torch.repeat_interleave(torch.arange(rows), deg)
    off = (torch.randn(E, generator=g) * (n_cols * 0.01)).long()
    idx = (r * (n_cols // max(rows, 1)) + off).clamp_(0, n_cols - 1)
    return indptr.to(device), idx.to(device), E


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=700_000)
    p.add_argument('--cols', type=int, default=750_000)
    p.add_argument('--deg', type=int, default=50)
    p.add_argument('--F', type=int, default=256)
    p.add_argument('--iters', type=int, default=10)
    p.add_argument('--col-block', type=int, default=0)
    p.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    p.add_argument('--no-scale', action='store_true',
                   help='no src/dst scale vectors (SAGE forward has no src scale)')
    p.add_argument('--wave-index', type=str, default=None,
                   help='SW == 64 kernel: 0 or 1; "0,1" alternates them call '
                        'by call')
    args = p.parse_args()
    assert torch.cuda.is_available()
    from adaqp_amd.ops.kernels import SpmmView, spmm, native
    native()
    dev = torch.device('cuda')
    indptr, indices, E = build_csr(args.rows, args.deg, args.cols, dev)
    view = SpmmView(indptr, indices, 0, args.rows,
                    col_block=args.col_block).to(dev)
    dtype = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    x = torch.randn(args.cols, args.F, device=dev).to(dtype)
    src = None if args.no_scale else torch.rand(args.cols, device=dev) + 0.5
    dst = None if args.no_scale else torch.rand(args.rows, device=dev) + 0.5
    gather_bytes = E * (args.F * x.element_size() + 12)
    head = (f'rows={args.rows} E={E} F={args.F} {args.dtype} '
            f'cb={args.col_block}')

    if args.wave_index is None or ',' not in args.wave_index:
        wi = None if args.wave_index is None else bool(int(args.wave_index))
        for _ in range(3):
            y = spmm(view, x, None, src, dst, wave_index=wi)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            y = spmm(view, x, None, src, dst, wave_index=wi)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        print(f'{head}: {dt*1e3:.3f} ms/call, '
              f'apparent gather {gather_bytes/dt/1e12:.2f} TB/s')
        sys.stdout.flush()
        return

    modes = [int(m) for m in args.wave_index.split(',')]
    outs = {}
    for _ in range(3):
        for m in modes:
            outs[m] = spmm(view, x, None, src, dst, wave_index=bool(m))
    torch.cuda.synchronize()
    same = all(torch.equal(outs[modes[0]], outs[m]) for m in modes[1:])
    print(f'{head}: outputs of wave-index {modes} bit-identical: {same}')
    times = {m: [] for m in modes}
    for _ in range(args.iters):
        for m in modes:
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            spmm(view, x, None, src, dst, wave_index=bool(m))
            b.record()
            b.synchronize()
            times[m].append(a.elapsed_time(b))
    for m in modes:
        t = times[m]
        med = statistics.median(t)
        print(f'  wave-index {m}: {med:.3f} ms ({min(t):.3f}..{max(t):.3f}), '
              f'apparent gather {gather_bytes/(med*1e-3)/1e12:.2f} TB/s')
    sys.stdout.flush()


if __name__ == '__main__':
    main()
