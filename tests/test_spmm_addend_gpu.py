"""The SpMM epilogue addend: ``spmm(..., addend=a)`` must equal
``spmm(...) + a`` bit for bit — the SpMM value is rounded to y's dtype
first and the add rounds on its own (never an FMA with the dst scale).
Covered: the direct store of every sub-wavefront width, both SW == 64
kernels, split rows and empty rows (the partial-combine pass), views
without rows or without edges, and an ``out=`` row slice."""
import pytest
import torch

import kernel_oracles as O
from test_spmm_scalar_gpu import NL, R, _graph, _x

pytestmark = pytest.mark.gpu

# fp32 104 runs SW == 32, bf16 256 runs SW == 32; the rest SW == 64
CASES = [(torch.float32, 256), (torch.float32, 132), (torch.float32, 104),
         (torch.bfloat16, 256), (torch.bfloat16, 520)]


def _addend(nrows, F, dtype, seed=3):
    gen = torch.Generator().manual_seed(seed + F)
    return torch.randn(nrows, F, generator=gen).to(dtype).cuda()


def _view(indptr, indices, col_block):
    from adaqp_amd.ops.kernels import SpmmView, native
    native()
    return SpmmView(indptr.cuda(), indices.cuda(), 0, indptr.numel() - 1,
                    col_block=col_block).to('cuda')


@pytest.mark.parametrize('wave_index', [True, False])
@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype,F', CASES)
def test_addend_equals_separate_add(dtype, F, col_block, wave_index):
    from adaqp_amd.ops.kernels import spmm
    indptr, indices, src, dst = _graph()
    view = _view(indptr, indices, col_block)
    assert view.n_part > 0 and view.zero_rows.numel() > 0
    xg = _x(F, dtype).cuda()
    xl, xr = xg[:NL].contiguous(), xg[NL:].contiguous()
    a = _addend(R, F, dtype)
    for s, d in ((src.cuda(), dst.cuda()), (None, None)):
        plain = spmm(view, xl, xr, s, d, wave_index=wave_index)
        fused = spmm(view, xl, xr, s, d, addend=a, wave_index=wave_index)
        assert fused.dtype == dtype
        assert torch.equal(fused, plain + a)
    # row 0 is empty: its result is the addend itself
    assert torch.equal(fused[0], a[0])


@pytest.mark.parametrize('wave_index', [True, False])
@pytest.mark.parametrize('dtype,F', [(torch.float32, 256),
                                     (torch.bfloat16, 520)])
def test_addend_out_slice(dtype, F, wave_index):
    """``out=`` and ``addend=`` both row slices at an odd row offset, as the
    central/marginal calls pass them; rows outside keep their fill."""
    from adaqp_amd.ops.kernels import spmm
    indptr, indices, src, dst = _graph()
    view = _view(indptr, indices, 0)
    xg = _x(F, dtype).cuda()
    xl, xr = xg[:NL].contiguous(), xg[NL:].contiguous()
    a_big = _addend(R + 7, F, dtype)
    big = torch.full((R + 7, F), -3.0, dtype=dtype, device='cuda')
    plain = spmm(view, xl, xr, src.cuda(), dst.cuda(), wave_index=wave_index)
    y = spmm(view, xl, xr, src.cuda(), dst.cuda(), out=big[5:5 + R],
             addend=a_big[5:5 + R], wave_index=wave_index)
    assert y.data_ptr() == big[5:5 + R].data_ptr()
    assert torch.equal(big[5:5 + R], plain + a_big[5:5 + R])
    assert (big[:5].float() == -3.0).all() and (big[5 + R:].float() == -3.0).all()


@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_addend_degenerate_views(dtype, col_block):
    """No rows: an empty result. Rows without any edge (with col_block the
    kernel's n_seg == 0 early-out): the addend itself."""
    from adaqp_amd.ops.kernels import spmm
    F = 256
    x = _x(F, dtype).cuda()
    none = torch.empty(0, dtype=torch.int64)
    view = _view(torch.zeros(1, dtype=torch.int64), none, col_block)
    y = spmm(view, x, None, None, None, addend=_addend(0, F, dtype))
    torch.cuda.synchronize()
    assert y.shape == (0, F) and y.dtype == dtype
    view = _view(torch.zeros(5, dtype=torch.int64), none, col_block)
    a = _addend(4, F, dtype)
    y = spmm(view, x, None, None, torch.ones(4, device='cuda'), addend=a)
    assert torch.equal(y, a)
