#!/usr/bin/env python3
"""Self-contained SpMM microbench (no partition machinery, safe under
rocprofv3). Builds a products-like CSR directly on the GPU and times the
spmm_csr kernel; prints effective gather TB/s.

``--wave-index`` picks the SW == 64 kernel (0 = per-lane index kernel,
1 = wave-uniform index kernel; default: the library's). Both
(``--wave-index 0,1``) are alternated call by call and each is reported
as median (min..max) of per-call device-event times, after checking that
they produce the same bits.

``--packed 0,1`` does the same for the packed-gather kernel against the
dense one (fp32, F % 4 == 0, F <= 256), once per ``--density``: the input
is synthetic, zeros placed i.i.d. per element, and the pack kernel is timed
on its own. ``--packed-depth 4,8`` adds one packed variant per number of
row fetches in flight."""
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
    p.add_argument('--packed', type=str, default=None,
                   help='"0,1": dense and packed-gather kernel alternated '
                        'call by call, per --density')
    p.add_argument('--density', type=str, default='0.25,0.5,1.0',
                   help='fractions of non-zero elements for --packed')
    p.add_argument('--packed-depth', type=str, default='4',
                   help='row fetches in flight in the packed kernel (4, 8 '
                        'or "4,8")')
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

    if args.packed is not None:
        packed_bench(args, view, x, src, dst, E, head)
        return

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


def _timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _fmt(t):
    return f'{statistics.median(t):.3f} ms ({min(t):.3f}..{max(t):.3f})'


def packed_bench(args, view, x, src, dst, E, head):
    from adaqp_amd.ops.kernels import pack_rows, spmm
    assert x.dtype == torch.float32, '--packed is fp32 only'
    want = [int(m) for m in args.packed.split(',')]
    depths = [int(d) for d in args.packed_depth.split(',')]
    # variants: None = dense kernel, d = packed kernel with d fetches in flight
    variants = ([None] if 0 in want else []) + (depths if 1 in want else [])
    gen = torch.Generator(device=x.device).manual_seed(7)
    for dens in [float(d) for d in args.density.split(',')]:
        keep = torch.rand(x.shape, device=x.device, generator=gen) < dens
        xd = (x * keep).contiguous()
        del keep
        nnz = (xd != 0).sum(1)
        ovf = float((nnz > args.F // 2).float().mean())
        tp = []
        for i in range(3 + args.iters):
            t, pk = _timed(lambda: pack_rows(xd))
            if i >= 3:
                tp.append(t)
        assert pk is not None
        outs = {}
        for _ in range(3):
            for v in variants:
                outs[v] = spmm(view, xd, None, src, dst,
                               packed=None if v is None else pk,
                               packed_depth=v)
        torch.cuda.synchronize()
        same = all(torch.equal(outs[variants[0]], outs[v])
                   for v in variants[1:])
        print(f'{head} density={dens} (overflow rows {ovf:.3f}): outputs of '
              f'{["dense" if v is None else f"packed/{v}" for v in variants]}'
              f' bit-identical: {same}')
        print(f'  pack kernel: {_fmt(tp)}, '
              f'{(xd.numel() * 4 + pk.buf.numel()) / (statistics.median(tp) * 1e-3) / 1e12:.2f}'
              f' TB/s read + written (upper bound on bytes)')
        times = {v: [] for v in variants}
        for _ in range(args.iters):
            for v in variants:
                t, _ = _timed(lambda: spmm(view, xd, None, src, dst,
                                           packed=None if v is None else pk,
                                           packed_depth=v))
                times[v].append(t)
        for v in variants:
            name = 'dense' if v is None else f'packed, {v} in flight'
            print(f'  {name}: {_fmt(times[v])}')
        sys.stdout.flush()
        del xd, pk, outs


if __name__ == '__main__':
    main()
