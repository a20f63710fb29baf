"""The edge-compacting row-skipping SpMM (csrc/spmm_compact.hip), fp32 and
bf16, and ``row_live`` on bf16.

The kernel gives each accumulator exactly the live edges the dense kernel
gives it, in the same order, so ``spmm(..., live=row_live(x))`` must equal
``spmm(...)`` of the same dtype on exact bits: every comparison is
``torch.equal`` on the integer view, NaN positions included. For finite inputs
the float64 oracle of ``agg_oracles`` bounds the result as well, with that
module's counted tolerance (the scales are plain fp32 inputs the oracle reads
exactly, so ``n_scales = 0``).

In-degrees 0..5, 7 and 15/16/17, 31/33, 63/64/65, 129 hit every batch size and
the chunk boundary of every sub-wavefront width; a row of 600 edges is split
into segments (partial slots, combine pass). Inputs are ``randn`` with scales
in [0.25, 1.5]: no product underflows, so the documented ``-0.f`` exception of
the row-skipping kernels cannot occur."""
import functools
import os

import pytest
import torch

from agg_oracles import _counted_tolerance, _raise_first, spmm_reference
from kernel_oracles import segs_per_row

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
# 260 (fp32) and 520 (bf16) are the smallest F with a second feature pass
SHAPES = ([(F32, F) for F in (256, 104, 48, 6, 47, 260)]
          + [(BF, F) for F in (256, 104, 48, 6, 520)])
PATTERNS = ['none', 'third', '92', 'all', 'special']
R, NL, NR = 200, 301, 50
HUB = 600
DEGS = [0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 33, 63, 64, 65, 129, HUB]
NEGZERO_ROW, DENORM_ROW, NAN_ROW, INF_ROW = 7, 10, 13, 16   # all 1 mod 3
# (src scale, dst scale, addend, out= a row slice) of the calls of one case
COMBOS = [(False, False, False, False), (True, True, False, False),
          (True, False, True, True), (False, True, True, False)]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


@functools.lru_cache(maxsize=None)
def _graph():
    gen = torch.Generator().manual_seed(43)
    degs = DEGS + torch.randint(0, 12, (R - len(DEGS),), generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.randint(0, NL + NR, (int(indptr[-1]),), generator=gen)
    # the denormal row is gathered only by the two longest rows, next to
    # dozens of ordinary values: a sum made of it alone would be a denormal,
    # an absolute error the oracle's relative bound has no term for
    lo, hi = int(indptr[DEGS.index(129)]), int(indptr[len(DEGS)])
    short = torch.ones_like(indices, dtype=torch.bool)
    short[lo:hi] = False
    indices[short & (indices == DENORM_ROW)] = DENORM_ROW + 2
    indices[lo], indices[hi - 1] = DENORM_ROW, DENORM_ROW
    src = torch.rand(NL + NR, generator=gen) * 1.25 + 0.25
    dst = torch.rand(R, generator=gen) * 1.25 + 0.25
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
def _operands(dtype, F):
    """({pattern: x_local}, remote block, addend over R + 8 rows), on the CPU.
    'third' also holds a row of -0.0 only (dead) and a row whose one non-zero
    is a denormal (live); 'special' is 'third' with a NaN and an Inf row."""
    gen = torch.Generator().manual_seed(700 + F)
    base = torch.randn(NL, F, generator=gen)
    rows = torch.arange(NL)
    third = base.clone()
    third[rows % 3 == 1] = 0.0
    third[NEGZERO_ROW] = -0.0
    third[DENORM_ROW, F // 2] = 1e-40
    sparse = base.clone()
    sparse[rows % 13 != 0] = 0.0                      # 92 % dead
    special = third.clone()
    special[NAN_ROW, 0] = float('nan')
    special[INF_ROW, F - 1] = float('-inf')
    xs = {'none': base, 'third': third, '92': sparse,
          'all': torch.zeros(NL, F), 'special': special}
    xs = {k: v.to(dtype) for k, v in xs.items()}
    assert xs['third'][DENORM_ROW, F // 2] != 0
    assert xs['third'][DENORM_ROW].float().abs().max() < 1.2e-38
    xr = torch.randn(NR, F, generator=gen)
    xr[::5] = 0.0                       # zero remote rows are fetched anyway
    addend = torch.randn(R + 8, F, generator=gen)
    return xs, xr.to(dtype), addend.to(dtype)


@functools.lru_cache(maxsize=None)
def _oracle(dtype, F, pattern, ss, ds):
    indptr, indices, src, dst = _graph()
    xs, xr, _ = _operands(dtype, F)
    ref, S, deg = spmm_reference(indptr, indices, torch.cat([xs[pattern], xr]),
                                 src if ss else None, dst if ds else None)
    segs = segs_per_row(_view())
    ref, tol = _counted_tolerance(ref, None, S, torch.zeros_like(S), deg,
                                  segs, 0, dtype)
    return ref, tol, deg, segs


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dtype,F', SHAPES,
                         ids=[f'{"bf16" if d == BF else "fp32"}-{F}'
                              for d, F in SHAPES])
def test_compact_spmm_equals_dense(dtype, F, pattern, order):
    from adaqp_amd.ops.kernels import row_live, spmm
    _, _, src, dst = _graph()
    view = _view()
    xs, xr, addend = _operands(dtype, F)
    xl, xr_d, addend_d = xs[pattern].cuda(), xr.cuda(), addend.cuda()
    src_d, dst_d = src.cuda(), dst.cuda()
    live = row_live(xl)
    want = (_bits(xs[pattern]) & 0x7FFF != 0).any(1) if dtype == BF else \
        (_bits(xs[pattern]) & 0x7FFFFFFF != 0).any(1)
    assert live.dtype == torch.uint8
    assert torch.equal(live.cpu().bool(), want)
    if pattern == 'third':
        assert not want[NEGZERO_ROW] and want[DENORM_ROW]
    if pattern == '92':
        assert 0.91 < 1.0 - float(want.float().mean()) < 0.93
    finite = pattern != 'special'
    for ss, ds, ad, use_out in COMBOS:
        kw = dict(x_remote=xr_d, src_scale=src_d if ss else None,
                  dst_scale=dst_d if ds else None,
                  addend=addend_d[4:4 + R] if ad else None, order=order)
        dense = spmm(view, xl, **kw)
        out = (torch.full((R + 8, F), float('nan'), device='cuda',
                          dtype=dtype)[4:4 + R] if use_out else None)
        got = spmm(view, xl, out=out, live=live, compact=True, **kw)
        assert out is None or got is out
        assert got.dtype == dtype
        assert torch.equal(_bits(got), _bits(dense)), (ss, ds, ad)
        if dtype == F32:      # the edge-walking kernel agrees as well
            walk = spmm(view, xl, live=live, compact=False, **kw)
            assert torch.equal(_bits(got), _bits(walk)), (ss, ds, ad)
        if finite and not ad:
            ref, tol, deg, segs = _oracle(dtype, F, pattern, ss, ds)
            _raise_first(f'{dtype} F={F} {pattern} ss={ss} ds={ds}', got, ref,
                         tol, deg, segs)
    if not finite:
        assert torch.isnan(dense).any() and torch.isinf(dense).any()


@pytest.mark.parametrize('F', [256, 104, 48, 6, 520])
def test_row_live_bf16_on_few_rows(F):
    """Fewer rows than one sub-wavefront owns, and none."""
    from adaqp_amd.ops.kernels import row_live
    _, xr, _ = _operands(BF, F)
    for n in (1, 2, 3, 5, NR):
        x = xr[:n].clone()
        assert torch.equal(row_live(x.cuda()).cpu().bool(),
                           (_bits(x) & 0x7FFF != 0).any(1))
    assert row_live(torch.zeros(0, F, device='cuda', dtype=BF)).shape == (0,)


@pytest.fixture(scope='module')
def world1():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29811')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    comm = Communicator()
    try:
        g = random_partitioned_graph(3000, 30000, 64, 10, 1, seed=9)
        yield comm, partition_all(g, 1)[0]
    finally:
        Communicator.shutdown()


def _step(world1, skip, monkeypatch):
    """(loss, grads) of one training step of a two-layer DistSAGE on a bf16
    engine, the loss masked to every third node, and the skip-path hits."""
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import global_train_count, train_epoch
    monkeypatch.delenv('ADAQP_BWD_SKIP_ZERO_BF16', raising=False)
    comm, lg = world1
    engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                         msg_dims=[64, 32], device=comm.device)
    engine.set_uniform_assignment(8)
    engine.compute_dtype = BF
    engine.bwd_skip_zero_bf16 = skip
    n = engine.graph.train_mask.shape[0]
    engine.graph.train_mask = torch.arange(n, device=comm.device) % 3 == 0
    torch.manual_seed(1234)
    model = DistSAGE(64, 32, 10, 2).to(comm.device)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loss = train_epoch(engine, model, opt, global_train_count(engine),
                       multilabel=False)
    torch.cuda.synchronize()
    return (loss, [p.grad.clone() for p in model.parameters()],
            engine.bwd_skip_hits)


def test_bf16_training_step_is_the_same_bits_with_and_without_the_skip(
        world1, monkeypatch):
    loss_on, grads_on, hits_on = _step(world1, True, monkeypatch)
    loss_off, grads_off, hits_off = _step(world1, False, monkeypatch)
    assert hits_on == 1 and hits_off == 0
    assert torch.isfinite(loss_on) and torch.equal(_bits(loss_on), _bits(loss_off))
    assert any(bool(g.ne(0).any()) for g in grads_on)
    for k, (a, b) in enumerate(zip(grads_on, grads_off)):
        assert torch.equal(_bits(a), _bits(b)), f'grad {k} differs'
