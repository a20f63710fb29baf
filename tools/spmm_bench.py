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
dense one (fp32 with F % 4 == 0 or ``--dtype bf16`` with F % 8 == 0,
F <= 256), once per ``--density``: the input
is synthetic, zeros placed i.i.d. per element, and the pack kernel is timed
on its own. ``--packed-depth 4,8`` adds one packed variant per number of
row fetches in flight.

``--gather-bf16`` times the fp32 dense kernel against the bf16-gather path
of the fp32 backward (``round_rows_bf16`` plus the mixed SpMM, with an fp32
addend), alternated call by call on the same view.

``--zero-rows 0,0.34,0.92`` times the dense kernel against ``row_live`` plus
the row-skipping kernel (the output layer's backward), once per fraction of
all-zero rows, alternated call by call with an addend, after asserting that
all give the same bits. ``--compact 0,1`` picks the row-skipping kernels: 0 the
edge-walking one (fp32 only), 1 the edge-compacting one (fp32 and
``--dtype bf16``, which has no other); with ``--order 0,1`` every kernel,
the dense one included, runs once per segment order.

``--order 0,1`` alternates the static segment order and the ordered sweep call
by call, the sweep once per ``--chunk`` size (``--chunk 1,4,16,64``), after
asserting that all give the same bits. Alone it times the dense kernel; with
``--packed 1`` the packed-gather kernel at each ``--density``, with
``--zero-rows`` the row-skipping kernel at each fraction (with ``--compact``
as well: see above)."""
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
    p.add_argument('--gather-bf16', action='store_true',
                   help='fp32 dense kernel against the stochastic-rounding '
                        'cast plus the bf16-gather kernel, alternated call '
                        'by call (fp32 only)')
    p.add_argument('--zero-rows', type=str, default=None,
                   help='fractions of all-zero rows, e.g. "0,0.34,0.92": fp32 '
                        'dense kernel against row_live plus the row-skipping '
                        'kernel, alternated call by call')
    p.add_argument('--compact', type=str, default=None,
                   help='with --zero-rows: "0,1" the edge-walking (fp32) '
                        'and the edge-compacting row-skipping kernel, '
                        'alternated call by call with the dense one')
    p.add_argument('--order', type=str, default=None,
                   help='"0,1": static segment order and ordered sweep '
                        'alternated call by call; combines with --packed 1 '
                        'and --zero-rows')
    p.add_argument('--chunk', type=str, default='4',
                   help='segments per ticket of the ordered sweep, e.g. '
                        '"1,4,16,64"')
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

    if args.zero_rows is not None and (args.compact is not None
                                       or x.dtype == torch.bfloat16):
        zero_rows_bench(args, view, x, src, dst, head)
        return

    if args.order is not None:
        order_bench(args, view, x, src, dst, head)
        return

    if args.packed is not None:
        packed_bench(args, view, x, src, dst, E, head)
        return

    if args.gather_bf16:
        gather_bf16_bench(args, view, x, src, dst, head)
        return

    if args.zero_rows is not None:
        zero_rows_bench(args, view, x, src, dst, head)
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


def order_bench(args, view, x, src, dst, head):
    """Static order against the ordered sweep at each chunk size, on the
    dense, the packed-gather (--packed 1) or the row-skipping (--zero-rows)
    kernel."""
    from adaqp_amd.ops.kernels import pack_rows, row_live, spmm
    orders = [int(o) for o in args.order.split(',')]
    variants = ([(0, 4)] if 0 in orders else []) + (
        [(1, int(c)) for c in args.chunk.split(',')] if 1 in orders else [])
    E = int(view.indices.numel())
    gen = torch.Generator(device=x.device).manual_seed(7)
    if args.packed is not None:
        assert x.dtype == torch.float32 and '1' in args.packed.split(',')
        cases = [('density', float(d)) for d in args.density.split(',')]
    elif args.zero_rows is not None:
        assert x.dtype == torch.float32
        cases = [('zero rows', float(f)) for f in args.zero_rows.split(',')]
    else:
        cases = [('dense', None)]
    for kind, val in cases:
        kw, xc = {}, x
        if kind == 'density':
            xc = (x * (torch.rand(x.shape, device=x.device, generator=gen)
                       < val)).contiguous()
            kw = {'packed': pack_rows(xc)}
            assert kw['packed'] is not None
        elif kind == 'zero rows':
            keep = torch.rand(x.shape[0], device=x.device, generator=gen) >= val
            xc = (x * keep[:, None]).contiguous()
            kw = {'live': row_live(xc),
                  'addend': torch.randn(args.rows, args.F, device=x.device)}
        outs = {}
        for _ in range(3):
            for v in variants:
                outs[v] = spmm(view, xc, None, src, dst, order=v[0],
                               chunk=v[1], **kw)
        torch.cuda.synchronize()
        for v in variants[1:]:
            assert torch.equal(outs[variants[0]], outs[v]), \
                f'order/chunk {v} differs from {variants[0]}'
        print(f'{head} {kind}{"" if val is None else " " + str(val)}: outputs '
              f'of {len(variants)} traversals bit-identical: True')
        del outs
        times = {v: [] for v in variants}
        for _ in range(args.iters):
            for v in variants:
                t, _ = _timed(lambda: spmm(view, xc, None, src, dst,
                                           order=v[0], chunk=v[1], **kw))
                times[v].append(t)
        for v in variants:
            name = 'static order' if v[0] == 0 else f'ordered, chunk {v[1]}'
            med = statistics.median(times[v])
            print(f'  {name}: {_fmt(times[v])}, {E / (med * 1e-3) / 1e9:.2f} '
                  f'G edges/s')
        sys.stdout.flush()
        del xc, kw


def packed_bench(args, view, x, src, dst, E, head):
    from adaqp_amd.ops.kernels import pack_rows, pack_rows_bf16, spmm
    if x.dtype == torch.bfloat16:
        pack_rows = pack_rows_bf16
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
              f'{(xd.numel() * xd.element_size() + pk.buf.numel()) / (statistics.median(tp) * 1e-3) / 1e12:.2f}'
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


def gather_bf16_bench(args, view, x, src, dst, head):
    """fp32 dense SpMM against round_rows_bf16 + the mixed SpMM on the same
    view, with an fp32 addend as the SAGE backward has one."""
    from adaqp_amd.ops.kernels import round_rows_bf16, spmm
    assert x.dtype == torch.float32 and args.F % 2 == 0
    addend = torch.randn(args.rows, args.F, device=x.device)

    def dense():
        return spmm(view, x, None, src, dst, addend=addend)

    def cast():
        return round_rows_bf16(x, 1234)

    def mixed(xb):
        return spmm(view, xb, None, src, dst, addend=addend,
                    out_dtype=torch.float32)

    for _ in range(3):
        yd, xb = dense(), cast()
        ym = mixed(xb)
    torch.cuda.synchronize()
    same = torch.equal(ym, spmm(view, xb.float(), None, src, dst, addend=addend))
    err = float((ym - yd).abs().max() / yd.abs().max())
    print(f'{head}: bf16-gather output equals the fp32 kernel on the widened '
          f'rows: {same}; max |mixed - fp32| / max |fp32| = {err:.3e}')
    td, tc, tm = [], [], []
    for _ in range(args.iters):
        td.append(_timed(dense)[0])
        t, xb = _timed(cast)
        tc.append(t)
        tm.append(_timed(lambda: mixed(xb))[0])
    E = int(view.indices.numel())
    print(f'  fp32 dense:       {_fmt(td)}, apparent gather '
          f'{E * (args.F * 4 + 12) / (statistics.median(td) * 1e-3) / 1e12:.2f} TB/s')
    print(f'  cast (SR, bf16):  {_fmt(tc)}, '
          f'{x.numel() * 6 / (statistics.median(tc) * 1e-3) / 1e12:.2f} TB/s '
          f'read + written')
    print(f'  bf16 gather:      {_fmt(tm)}, apparent gather '
          f'{E * (args.F * 2 + 12) / (statistics.median(tm) * 1e-3) / 1e12:.2f} TB/s')
    print(f'  cast + bf16 gather, sum of medians: '
          f'{statistics.median(tc) + statistics.median(tm):.3f} ms')
    sys.stdout.flush()


def zero_rows_bench(args, view, x, src, dst, head):
    """Dense SpMM against row_live + the row-skipping SpMMs (--compact: 0 the
    edge-walking kernel, 1 the edge-compacting one) on the same view, with an
    addend as the SAGE backward has one; rows are zeroed i.i.d. with each
    given probability. With --order every kernel runs once per order."""
    from adaqp_amd.ops.kernels import row_live, spmm
    bf16 = x.dtype == torch.bfloat16
    compacts = ([1] if bf16 else
                [int(c) for c in (args.compact or '0').split(',')])
    assert not bf16 or args.F % 2 == 0
    orders = ([None] if args.order is None
              else [int(o) for o in args.order.split(',')])
    chunk = int(args.chunk.split(',')[0])
    # (name, order, compact); compact None = the dense kernel
    variants = [(f'{k}{"" if o is None else f", order {o}"}', o, c)
                for k, c in [('dense', None)]
                + [(('compacting' if c else 'edge-walking'), c)
                   for c in compacts]
                for o in orders]
    addend = torch.randn(args.rows, args.F, device=x.device).to(x.dtype)
    gen = torch.Generator(device=x.device).manual_seed(11)
    E = int(view.indices.numel())
    bits = torch.int16 if bf16 else torch.int32
    for frac in [float(f) for f in args.zero_rows.split(',')]:
        keep = torch.rand(x.shape[0], device=x.device, generator=gen) >= frac
        xz = (x * keep[:, None]).contiguous()

        def mark():
            return row_live(xz)

        def run(v, live):
            kw = {} if v[1] is None else {'order': v[1], 'chunk': chunk}
            if v[2] is not None:
                kw.update(live=live, compact=bool(v[2]))
            return spmm(view, xz, None, src, dst, addend=addend, **kw)

        outs = {}
        for _ in range(3):
            live = mark()
            for v in variants:
                outs[v] = run(v, live)
        torch.cuda.synchronize()
        for v in variants[1:]:
            assert torch.equal(outs[variants[0]].view(bits),
                               outs[v].view(bits)), \
                f'{v[0]} differs from {variants[0][0]}'
        dead = 1.0 - float(live.float().mean())
        print(f'{head} zero rows {frac} (marked dead {dead:.3f}): outputs of '
              f'{len(variants)} variants bit-identical: True')
        del outs
        tl, times = [], {v: [] for v in variants}
        for _ in range(args.iters):
            t, live = _timed(mark)
            tl.append(t)
            for v in variants:
                times[v].append(_timed(lambda: run(v, live))[0])
        print(f'  row_live: {_fmt(tl)}, '
              f'{xz.numel() * xz.element_size() / (statistics.median(tl) * 1e-3) / 1e12:.2f}'
              f' TB/s read')
        for v in variants:
            med = statistics.median(times[v])
            print(f'  {v[0]}: {_fmt(times[v])}, '
                  f'{E / (med * 1e-3) / 1e9:.2f} G edges/s'
                  + ('' if v[2] is None else
                     f'; with row_live {med + statistics.median(tl):.3f} ms'))
        sys.stdout.flush()
        del xz, keep, live


if __name__ == '__main__':
    main()
