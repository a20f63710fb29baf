#!/usr/bin/env python3
"""Microbench of the quantized-gather SpMM against the path it replaces.

A marginal-like view is built on the GPU: ``--rows`` destination rows of
mean degree ``--deg`` over ``--local`` local and ``--remote`` remote columns,
each edge remote with probability ``--remote-frac``. The remote block is
quantized at a uniform bit width (``--bits mixed``: 2, 4 or 8 bits per row at
random). Per width, two pipelines are alternated call by call on the same wire
bytes and timed with device events:

  unfused: quant_unpack (mixed_dequantize into a fresh [R, F] block) + the
           dense SpMM
  fused:   the row-descriptor kernel + the quantized-gather SpMM

after checking that both give the same bits. Reported as median (min..max).

``--dtype bf16`` gathers bf16 rows: the unfused pipeline unpacks into a bf16
block and runs the dense bf16 SpMM, or with ``--out-dtype fp32`` the mixed
SpMM (bf16 rows, fp32 result); the fused one is the bf16 quantized-gather
kernel (``spmm(..., quant_bf16=True)``) with the same output type."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=200_000)
    p.add_argument('--local', type=int, default=600_000)
    p.add_argument('--remote', type=int, default=150_000)
    p.add_argument('--deg', type=int, default=50)
    p.add_argument('--remote-frac', type=float, default=0.3)
    p.add_argument('--F', type=int, default=256)
    p.add_argument('--bits', type=str, default='2,4,8')
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--density', type=float, default=1.0,
                   help='< 1: zero local elements i.i.d. and also time the '
                        'unfused pipeline with the packed local gather')
    p.add_argument('--dtype', choices=['fp32', 'bf16'], default='fp32',
                   help='dtype of the gathered rows')
    p.add_argument('--out-dtype', choices=['same', 'fp32'], default='same',
                   help='fp32 with --dtype bf16: the mixed SpMM')
    args = p.parse_args()
    bf16 = args.dtype == 'bf16'
    assert bf16 or args.out_dtype == 'same', '--out-dtype fp32 needs --dtype bf16'
    assert not bf16 or args.density == 1.0, '--density is for fp32'
    dt = torch.bfloat16 if bf16 else torch.float32
    # keywords of the SpMM under test and of its unfused counterpart
    okw = {'out_dtype': torch.float32} if args.out_dtype == 'fp32' else {}
    qkw = dict(okw, quant_bf16=True) if bf16 else {}
    assert torch.cuda.is_available()
    from adaqp_amd.comm.buffers import _layout
    from adaqp_amd.ops.kernels import (QuantRemote, SpmmView, mixed_dequantize,
                                       mixed_quantize, native, pack_rows, spmm)
    native()
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    R, NL, F = args.remote, args.local, args.F
    E = args.rows * args.deg
    indptr = torch.arange(args.rows + 1, dtype=torch.int64) * args.deg
    # clustered columns of either kind around the row's own neighbourhood
    r = torch.arange(E) // args.deg
    rem = torch.rand(E, generator=gen) < args.remote_frac
    jit = torch.randn(E, generator=gen)
    loc_c = (r * (NL // args.rows) + (jit * NL * 0.01).long()).clamp_(0, NL - 1)
    rem_c = (r * R // args.rows + (jit * R * 0.01).long()).clamp_(0, R - 1) + NL
    indices = torch.where(rem, rem_c, loc_c)
    view = SpmmView(indptr.to(dev), indices.to(dev), 0, args.rows).to(dev)
    xl = torch.randn(NL, F, device=dev).to(dt)
    pk = None
    if args.density < 1.0:      # what the fused path gives up: packed local rows
        xl *= torch.rand(NL, F, device=dev) < args.density
        pk = pack_rows(xl)
    xsrc = torch.randn(R, F, device=dev)
    dst = torch.rand(args.rows, device=dev) + 0.5
    rows = torch.arange(R)
    print(f'rows={args.rows} E={E} local={NL} remote={R} F={F} remote edges '
          f'{float(rem.float().mean()):.3f}; [R, F] {args.dtype} block not '
          f'allocated by the fused path: '
          f'{R * F * xl.element_size() / 2**20:.1f} MiB')
    for bits in args.bits.split(','):
        row_bits = (torch.tensor([2, 4, 8])[torch.randint(0, 3, (R,), generator=gen)]
                    if bits == 'mixed' else torch.full((R,), int(bits)))
        plan = _layout([row_bits], [rows], F).to(dev)
        payload, params = mixed_quantize(xsrc, plan, 11)
        buf = QuantRemote.wire_buffer(plan.total_bytes, dev).copy_(payload)

        def unfused():
            xr = mixed_dequantize(buf, params, plan,
                                  torch.empty(R, F, dtype=dt, device=dev))
            return spmm(view, xl, xr, None, dst, **okw)

        def fused():
            return spmm(view, xl, QuantRemote(buf, params, plan, F), None, dst,
                        **qkw)

        def dequant_only():
            return mixed_dequantize(buf, params, plan,
                                    torch.empty(R, F, dtype=dt, device=dev))

        def desc_only():
            return QuantRemote(buf, params, plan, F).descriptors()

        def unfused_packed():
            xr = mixed_dequantize(buf, params, plan,
                                  torch.empty(R, F, device=dev))
            return spmm(view, xl, xr, None, dst, packed=pk)

        fns = {'unfused (unpack + dense SpMM)': unfused,
               'fused (descriptors + quantized-gather SpMM)': fused,
               'unpack alone': dequant_only, 'descriptors alone': desc_only}
        if pk is not None:
            fns['unfused, local rows packed (unpack + packed SpMM)'] = unfused_packed
        for _ in range(3):
            outs = {k: f() for k, f in fns.items()}
        torch.cuda.synchronize()
        a, b = list(outs.values())[:2]
        print(f'bits={bits} wire {plan.total_bytes / 2**20:.1f} MiB: outputs '
              f'bit-identical: {a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))}')
        del outs, a, b
        times = {k: [] for k in fns}
        for _ in range(args.iters):
            for k, f in fns.items():
                times[k].append(_timed(f)[0])
        for k in fns:
            print(f'  {k}: {_fmt(times[k])}')
        sys.stdout.flush()


if __name__ == '__main__':
    main()
