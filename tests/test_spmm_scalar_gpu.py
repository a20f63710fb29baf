"""The wave-uniform-index SpMM kernel against the per-lane SW == 64 kernel
(bit for bit) and against the float64 oracle.

Both kernels add edge j of a segment into accumulator j & 1 in increasing
j with one fmaf each and finish with (acc0 + acc1) * ds, so their results
must be ``torch.equal``; the row lengths below walk every loop of the new
kernel (quad, pair, single, one to three index chunks, split rows)."""
import functools

import pytest
import torch

import kernel_oracles as O

pytestmark = pytest.mark.gpu

# every (dtype, F) here runs one whole wavefront per segment (SW == 64):
# fp32 F > 128 and bf16 F > 256; 132 leaves lanes idle, 520 takes two
# feature chunks per segment
CASES = [(torch.float32, 132), (torch.float32, 256), (torch.bfloat16, 520)]
ROW_LENS = [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700]
R, NL, NR = 80, 180, 120


@functools.lru_cache(maxsize=None)
def _graph():
    gen = torch.Generator().manual_seed(97)
    degs = ROW_LENS + torch.randint(0, 9, (R - len(ROW_LENS),),
                                    generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.randint(0, NL + NR, (int(indptr[-1]),), generator=gen)
    assert (indices >= NL).any() and (indices < NL).any()
    src = torch.rand(NL + NR, generator=gen) + 0.5
    dst = torch.rand(R, generator=gen) + 0.5
    return indptr, indices, src, dst


@functools.lru_cache(maxsize=None)
def _x(F, dtype):
    gen = torch.Generator().manual_seed(5 + F)
    return torch.randn(NL + NR, F, generator=gen).to(dtype)


def _both(indptr, indices, x, nl, src, dst, col_block):
    """(y_wave, y_lane, view): the two SW == 64 kernels on one view, each
    into a NaN-filled output so an unwritten element shows."""
    from adaqp_amd.ops.kernels import SpmmView, native, spmm
    native()
    nrows = indptr.numel() - 1
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, nrows,
                    col_block=col_block).to('cuda')
    xg = x.cuda()
    xl, xr = xg[:nl].contiguous(), xg[nl:].contiguous()
    s = None if src is None else src.cuda()
    d = None if dst is None else dst.cuda()
    ys = []
    for wave in (True, False):
        out = torch.full((nrows, x.shape[1]), float('nan'), dtype=x.dtype,
                         device='cuda')
        ys.append(spmm(view, xl, xr, s, d, out=out, wave_index=wave))
    return ys[0], ys[1], view


@pytest.mark.parametrize('scaled', [True, False])
@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype,F', CASES)
def test_wave_index_equals_lane_index(dtype, F, col_block, scaled):
    indptr, indices, src, dst = _graph()
    if not scaled:
        src = dst = None
    x = _x(F, dtype)
    y_wave, y_lane, view = _both(indptr, indices, x, NL, src, dst, col_block)
    assert view.n_part > 0                      # rows 256+ are split
    assert not torch.isnan(y_lane.float()).any()
    assert torch.equal(y_wave, y_lane)
    O.check_spmm(indptr, indices, x, src, dst, y_wave.cpu(),
                 O.segs_per_row(view))


@pytest.mark.parametrize('dtype,F', [(torch.float32, 132),
                                     (torch.bfloat16, 520)])
def test_wave_index_grid_stride(dtype, F):
    """More segments than one pass of 16384 blocks x 4 wavefronts covers."""
    indptr, indices, src, dst = O.grid_stride_graph()
    x = O.grid_stride_x(F, dtype)
    y_wave, y_lane, view = _both(indptr, indices, x, O.GS_NL, src, dst, 0)
    assert view.seg_row.numel() > 65536
    assert torch.equal(y_wave, y_lane)
    O.check_spmm(indptr, indices, x, src, dst, y_wave.cpu(),
                 O.segs_per_row(view))
