"""The native column sum (bias gradient) against the float64 sum.

Bound: the one ``test_linear_grads_gpu`` uses for ``ones @ g`` — fp32
accumulation, at most one rounding per term plus two, each at most U32
relative to S = sum |g|: ``(N + 2) * U32 * S``, plus half a bf16 ulp
where the result is stored as bf16. The kernel's fixed-order tree has
fewer roundings on every path than N, so the bound holds for any N."""
import pytest
import torch

from kernel_oracles import U32, _first, bf16_half_ulp

pytestmark = pytest.mark.gpu

# (0,16) no rows; (1,1) one element; 47 / 300: odd and non-multiple-of-8
# widths (narrow loads); 4099 rows: more than one row block, ragged tail
SHAPES = [(0, 16), (1, 1), (77, 16), (130, 48), (4099, 47), (3000, 256),
          (5, 300)]


def check_colsum(got, g):
    gd = g.detach().cpu().double()
    N = gd.shape[0]
    ref, S = gd.sum(0), gd.abs().sum(0)
    tol = (N + 2) * U32 * S
    if got.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(ref.abs() + tol)
    o = got.detach().cpu().double()
    assert o.shape == ref.shape, (o.shape, ref.shape)
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        (i,) = _first(bad)
        raise AssertionError(
            f'colsum[{i}] = {float(o[i])!r}, oracle {float(ref[i])!r} '
            f'(tol {float(tol[i]):.3e}, N {N}, {got.dtype}); '
            f'{int(bad.sum())} bad of {o.numel()}')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('N,F', SHAPES)
def test_colsum(N, F, dtype):
    from adaqp_amd.ops.kernels import colsum, native
    native()
    gen = torch.Generator().manual_seed(1000 * N + F)
    g = torch.randn(N, F, generator=gen).to(dtype)
    gg = g.cuda()
    out = colsum(gg)
    assert out.dtype == dtype and out.shape == (F,)
    check_colsum(out, g)
    assert torch.equal(out, colsum(gg))         # fixed order: same bits
    if N == 0:
        assert (out.float() == 0).all()
