"""``row_live`` on bf16 and the ``compact=`` keyword of ``spmm`` on the CPU:
the first is the bit-pattern definition of the native kernel, the second is
ignored as ``live`` is."""
import torch


def test_row_live_bf16_is_the_bit_pattern_test():
    from adaqp_amd.ops.kernels import row_live
    x = torch.randn(41, 12, generator=torch.Generator().manual_seed(5))
    x[::3] = 0.0
    x[4] = -0.0
    x[7] = 0.0
    x[7, 2] = 1e-40                    # a bf16 denormal
    x[10] = 0.0
    x[10, 11] = float('nan')
    x = x.bfloat16()
    live = row_live(x)
    assert live.dtype == torch.uint8 and live.shape == (41,)
    assert torch.equal(live.bool(), (x.view(torch.int16) & 0x7FFF).ne(0).any(1))
    assert not live[0] and not live[4] and live[7] and live[10] and live[1]


def test_compact_is_ignored_on_the_cpu():
    from adaqp_amd.ops.kernels import SpmmView, row_live, spmm
    gen = torch.Generator().manual_seed(19)
    R, NL, NR, F = 30, 40, 10, 12
    deg = torch.randint(0, 6, (R,), generator=gen)
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.randint(0, NL + NR, (int(indptr[-1]),), generator=gen)
    view = SpmmView(indptr, indices, 0, R)
    xl = torch.randn(NL, F, generator=gen)
    xl[::3] = 0.0
    xr = torch.randn(NR, F, generator=gen)
    src = torch.rand(NL + NR, generator=gen) + 0.5
    dst = torch.rand(R, generator=gen) + 0.5
    for dtype in (torch.float32, torch.bfloat16):
        a, b = xl.to(dtype), xr.to(dtype)
        y0 = spmm(view, a, b, src, dst)
        y1 = spmm(view, a, b, src, dst, live=row_live(a), compact=True)
        assert y1.dtype == y0.dtype and torch.equal(y0, y1)
        assert torch.isfinite(y0).all()      # so equal values are equal bits
