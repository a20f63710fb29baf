"""``row_live`` and the row-skipping fp32 SpMM (csrc/spmm_rowskip.hip).

The kernel does ``spmm_csr_kernel``'s arithmetic in the same order and only
leaves out the fetch of local rows that ``row_live`` marks as all zero, so
``spmm(..., live=row_live(x))`` must equal ``spmm(...)`` on exact bits: every
comparison here is ``torch.equal`` on the int32 view, NaN positions included.
The float64 oracle of ``agg_oracles`` bounds the result as well, with that
module's counted tolerance (no engine scale vector enters: the scales here
are plain fp32 inputs the oracle reads exactly, so ``n_scales = 0``).

The graph has in-degrees 0, 1, 2, 3, 4, 5, 7 and 64 (every batch shape of the
edge loop), one row of 600 edges (split into segments at the default 256, so
the partial slots and ``combine_parts`` run) and 50 remote rows, which are
always fetched. 301 local rows: not a multiple of the four rows a
sub-wavefront of ``row_live`` owns, and several blocks at every width."""
import functools
import itertools

import pytest
import torch

from agg_oracles import _counted_tolerance, _raise_first, spmm_reference
from kernel_oracles import segs_per_row

pytestmark = pytest.mark.gpu

# F -> (sub-wavefront width, elements per lane) the kernel picks
SHAPES = {256: (64, 4), 104: (32, 4), 48: (16, 4), 6: (16, 2), 47: (64, 1)}
R, NL, NR = 200, 301, 50
HUB = 600
DEGS = [0, 1, 2, 3, 4, 5, 7, 64, HUB]
NEGZERO_ROW, DENORM_ROW, NAN_ROW, INF_ROW = 7, 10, 13, 16   # all 1 mod 3


def _i32(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _graph():
    gen = torch.Generator().manual_seed(41)
    degs = DEGS + torch.randint(0, 12, (R - len(DEGS),), generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.randint(0, NL + NR, (int(indptr[-1]),), generator=gen)
    assert (indices >= NL).any() and (indices < NL).any()
    # column DENORM_ROW (one denormal, else zeros) is gathered only by the
    # two long rows, next to dozens of ordinary values: a sum made of that
    # denormal alone would be rounded to a denormal, an absolute error the
    # oracle's relative bound has no term for
    lo, hi = int(indptr[DEGS.index(64)]), int(indptr[len(DEGS)])
    short = torch.ones_like(indices, dtype=torch.bool)
    short[lo:hi] = False
    indices[short & (indices == DENORM_ROW)] = DENORM_ROW + 2
    indices[lo], indices[hi - 1] = DENORM_ROW, DENORM_ROW
    src = torch.rand(NL + NR, generator=gen) + 0.25
    dst = torch.rand(R, generator=gen) + 0.5
    return indptr, indices, src, dst


@functools.lru_cache(maxsize=None)
def _view():
    from adaqp_amd.ops.kernels import SEG_EDGES, SpmmView, native
    native()
    indptr, indices, _, _ = _graph()
    assert HUB > 2 * SEG_EDGES
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, R).to('cuda')
    assert view.n_part >= 3 and view.zero_rows.numel() > 0
    return view


@functools.lru_cache(maxsize=None)
def _operands(F):
    """{name: (x_local, finite)} on the CPU, the remote block and the addend.
    'none' has no zero row, 'third' about a third, 'all' only zero rows;
    'special' is 'third' with a NaN row and an Inf row. 'third' also holds a
    row of -0.0 only (zero) and a row whose one non-zero is a denormal
    (live)."""
    gen = torch.Generator().manual_seed(900 + F)
    base = torch.randn(NL, F, generator=gen)
    third = base.clone()
    third[torch.arange(NL) % 3 == 1] = 0.0
    third[NEGZERO_ROW] = -0.0
    third[DENORM_ROW, F // 2] = 1e-40
    assert third[DENORM_ROW, F // 2] != 0
    assert third[DENORM_ROW].abs().max() < 1.2e-38
    special = third.clone()
    special[NAN_ROW, 0] = float('nan')
    special[INF_ROW, F - 1] = float('-inf')
    xs = {'none': (base, True), 'third': (third, True),
          'all': (torch.zeros(NL, F), True), 'special': (special, False)}
    xr = torch.randn(NR, F, generator=gen)
    xr[::5] = 0.0                       # zero remote rows are fetched anyway
    addend = torch.randn(R, F, generator=gen)
    return xs, xr, addend


def _live_ref(x):
    return (_i32(x) & 0x7FFFFFFF).ne(0).any(1)


@pytest.mark.parametrize('F', list(SHAPES))
def test_row_live_is_the_bit_pattern_test(F):
    from adaqp_amd.ops.kernels import native, row_live
    C = native()
    xs, xr, _ = _operands(F)
    for name, (x, _) in xs.items():
        live = row_live(x.cuda())
        assert live.dtype == torch.uint8 and live.shape == (NL,)
        want = _live_ref(x)
        assert torch.equal(live.cpu().bool(), want), name
        assert set(live.cpu().tolist()) <= {0, 1}
    third = xs['third'][0]
    want = _live_ref(third)
    assert not want[NEGZERO_ROW] and want[DENORM_ROW]
    assert not want[1] and want[0]
    frac = 1.0 - float(want.float().mean())
    assert 0.30 < frac < 0.37
    sp = _live_ref(xs['special'][0])
    assert sp[NAN_ROW] and sp[INF_ROW]
    for n in (1, 2, 3, 5, NR):           # fewer rows than one group owns
        x = xr[:n].clone()
        assert torch.equal(row_live(x.cuda()).cpu().bool(), _live_ref(x))
    assert C.row_live(torch.zeros(0, F, device='cuda')).shape == (0,)


@pytest.mark.parametrize('F', list(SHAPES))
def test_rowskip_spmm_equals_dense(F):
    from adaqp_amd.ops.kernels import row_live, spmm
    indptr, indices, src, dst = _graph()
    view = _view()
    segs = segs_per_row(view)
    xs, xr, addend = _operands(F)
    xr_d, addend_d = xr.cuda(), addend.cuda()
    src_d, dst_d = src.cuda(), dst.cuda()
    ve = 4 if F % 4 == 0 else 2 if F % 2 == 0 else 1
    sw = 16
    while sw < 64 and sw * ve < F:
        sw *= 2
    assert (sw, ve) == SHAPES[F]
    for name, (x, finite) in xs.items():
        xl = x.cuda()
        live = row_live(xl)
        ones = torch.ones_like(live)
        for ss, ds, ad, use_out in itertools.product([False, True], repeat=4):
            kw = dict(x_remote=xr_d, src_scale=src_d if ss else None,
                      dst_scale=dst_d if ds else None,
                      addend=addend_d if ad else None)
            dense = spmm(view, xl, **kw)
            out = (torch.full((R, F), float('nan'), device='cuda')
                   if use_out else None)
            got = spmm(view, xl, out=out, live=live, **kw)
            assert out is None or got is out
            assert torch.equal(_i32(got), _i32(dense)), (name, ss, ds, ad)
            # nothing marked dead: every row is fetched, zero rows included
            full = spmm(view, xl, live=ones, **kw)
            assert torch.equal(_i32(full), _i32(dense)), (name, ss, ds, ad)
            if finite and not ad:
                ref, S, deg = spmm_reference(
                    indptr, indices, torch.cat([x, xr]),
                    src if ss else None, dst if ds else None)
                ref, tol = _counted_tolerance(
                    ref, None, S, torch.zeros_like(S), deg, segs, 0,
                    torch.float32)
                _raise_first(f'F={F} {name} ss={ss} ds={ds}', got, ref, tol,
                             deg, segs)
        if not finite:
            assert torch.isnan(dense).any() and torch.isinf(dense).any()


def test_rowskip_spmm_without_a_remote_block():
    """Local columns only (the central view of the decomposed path)."""
    from adaqp_amd.ops.kernels import SpmmView, row_live, spmm
    indptr, indices, src, _ = _graph()
    view = SpmmView(indptr.cuda(), (indices % NL).cuda(), 0, R).to('cuda')
    xs, _, addend = _operands(48)
    xl = xs['third'][0].cuda()
    dense = spmm(view, xl, None, src.cuda(), None, addend=addend.cuda())
    got = spmm(view, xl, None, src.cuda(), None, addend=addend.cuda(),
               live=row_live(xl))
    assert torch.equal(_i32(got), _i32(dense))


def test_live_is_not_combined_with_other_gathers():
    from adaqp_amd.ops.kernels import pack_rows, row_live, spmm
    view = _view()
    xs, xr, _ = _operands(48)
    xl = xs['third'][0].cuda()
    live = row_live(xl)
    with pytest.raises(AssertionError):
        spmm(view, xl, xr.cuda(), None, None, packed=pack_rows(xl), live=live)
    with pytest.raises(AssertionError):
        spmm(view, xl.bfloat16(), xr.cuda().bfloat16(), None, None,
             out_dtype=torch.float32, live=live)
