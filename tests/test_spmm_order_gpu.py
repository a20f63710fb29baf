"""The ordered sweep over the SpMM segments (``order=1``) against the static
order (``order=0``).

The traversal decides only which wavefront computes a segment and when: every
segment is computed by the same code and split rows are combined in slot
order, so every comparison here is ``torch.equal``. The graph is the one of
test_spmm_scalar_gpu.py: an empty row 0, rows that walk every edge loop, split
hub rows and a remote block; its 83 segments are no multiple of a chunk or of
the segments of a block."""
import copy
import os

import pytest
import torch

from test_spmm_scalar_gpu import NL, R, _graph, _x

pytestmark = pytest.mark.gpu

# chunk sizes: one segment, an odd count, the widest of the sweep, more than
# the view has segments
CHUNKS = [1, 3, 64, 1000]
# fp32: F = 256 -> SW 64, 104 -> SW 32, 36 -> SW 16; bf16 256 -> SW 32, VE 8
DENSE = [(torch.float32, 256), (torch.float32, 104), (torch.float32, 36),
         (torch.bfloat16, 256)]


def _view(indptr, indices):
    from adaqp_amd.ops.kernels import SpmmView, native
    native()
    nrows = indptr.numel() - 1
    return SpmmView(indptr.cuda(), indices.cuda(), 0, nrows).to('cuda')


def _main_view():
    indptr, indices, _, _ = _graph()
    view = _view(indptr, indices)
    n_seg = view.seg_row.numel()
    assert view.n_part > 0 and n_seg % 4 and n_seg % 3 and n_seg < 1000
    return view


def _operands(F, dtype, scaled):
    _, _, src, dst = _graph()
    xg = _x(F, dtype).cuda()
    s, d = (src.cuda(), dst.cuda()) if scaled else (None, None)
    return xg[:NL].contiguous(), xg[NL:].contiguous(), s, d


def _nan_out(rows, F, dtype):
    return torch.full((rows, F), float('nan'), dtype=dtype, device='cuda')


def _same(a, b):
    assert not torch.isnan(a.float()).any()
    assert torch.equal(a, b)


@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('scaled', [True, False])
@pytest.mark.parametrize('dtype,F', DENSE)
def test_dense_order_equal(dtype, F, scaled, chunk):
    from adaqp_amd.ops.kernels import spmm
    view = _main_view()
    xl, xr, s, d = _operands(F, dtype, scaled)
    gen = torch.Generator().manual_seed(11 + F)
    addend = torch.randn(R, F, generator=gen).to(dtype).cuda()

    def run(order, **kw):
        return spmm(view, xl, xr, s, d, order=order, chunk=chunk, **kw)

    _same(run(1, out=_nan_out(R, F, dtype)), run(0, out=_nan_out(R, F, dtype)))
    _same(run(1, addend=addend), run(0, addend=addend))
    # out= as a row slice of a larger tensor, at an odd row offset
    big = [_nan_out(R + 8, F, dtype) for _ in range(2)]
    for order, b in zip((0, 1), big):
        run(order, out=b[3:3 + R])
    assert torch.equal(big[1][3:3 + R], big[0][3:3 + R])
    for b in big:
        assert torch.isnan(b[:3].float()).all()
        assert torch.isnan(b[3 + R:].float()).all()
        assert not torch.isnan(b[3:3 + R].float()).any()


@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('density', [0.25, 1.0])
@pytest.mark.parametrize('F', [256, 104])
def test_packed_order_equal(F, density, chunk):
    from adaqp_amd.ops.kernels import pack_rows, spmm
    view = _main_view()
    xl, xr, s, d = _operands(F, torch.float32, True)
    gen = torch.Generator().manual_seed(3 + F)
    xl = (xl * (torch.rand(NL, F, generator=gen) < density).cuda()).contiguous()
    pk = pack_rows(xl)
    assert pk is not None
    dense = spmm(view, xl, xr, s, d, order=0)
    for src in (s, None):          # the forward has no src scale
        y0 = spmm(view, xl, xr, src, d, packed=pk, order=0,
                  out=_nan_out(R, F, torch.float32))
        y1 = spmm(view, xl, xr, src, d, packed=pk, order=1, chunk=chunk,
                  out=_nan_out(R, F, torch.float32))
        _same(y1, y0)
        if src is not None:
            assert torch.equal(y0, dense)


@pytest.mark.parametrize('chunk', CHUNKS)
@pytest.mark.parametrize('zero_frac', [0.0, 0.5, 1.0])
def test_rowskip_order_equal(zero_frac, chunk):
    from adaqp_amd.ops.kernels import row_live, spmm
    F = 256
    view = _main_view()
    xl, xr, s, d = _operands(F, torch.float32, True)
    gen = torch.Generator().manual_seed(29)
    keep = (torch.rand(NL, generator=gen) >= zero_frac).cuda()
    xl = (xl * keep[:, None]).contiguous()
    live = row_live(xl)
    assert int(live.sum()) == int(keep.sum())
    addend = torch.randn(R, F, generator=gen).cuda()
    y0 = spmm(view, xl, xr, s, d, addend=addend, live=live, order=0)
    y1 = spmm(view, xl, xr, s, d, addend=addend, live=live, order=1,
              chunk=chunk, out=_nan_out(R, F, torch.float32))
    _same(y1, y0)
    assert torch.equal(y0, spmm(view, xl, xr, s, d, addend=addend, order=0))


@pytest.mark.parametrize('kernel', ['dense', 'packed', 'rowskip'])
def test_edge_views(kernel):
    """No rows; rows without an edge (zeros, or the addend); one segment."""
    from adaqp_amd.ops.kernels import pack_rows, row_live, spmm
    F = 256
    xl, _, _, _ = _operands(F, torch.float32, False)
    kw = {'packed': pack_rows(xl)} if kernel == 'packed' else (
        {'live': row_live(xl)} if kernel == 'rowskip' else {})
    none = torch.zeros(0, dtype=torch.int64)

    empty = _view(torch.zeros(1, dtype=torch.int64), none)
    for chunk in (1, 16):
        y = spmm(empty, xl, None, None, None, order=1, chunk=chunk, **kw)
        assert y.shape == (0, F)

    bare = _view(torch.zeros(8, dtype=torch.int64), none)
    addend = torch.randn(7, F, generator=torch.Generator().manual_seed(1)).cuda()
    for chunk in (1, 3, 16):
        y = spmm(bare, xl, None, None, None, order=1, chunk=chunk,
                 out=_nan_out(7, F, torch.float32), **kw)
        assert torch.equal(y, torch.zeros_like(y))
        y = spmm(bare, xl, None, None, None, order=1, chunk=chunk,
                 addend=addend, out=_nan_out(7, F, torch.float32), **kw)
        assert torch.equal(y, addend)

    one = _view(torch.tensor([0, 5]), torch.tensor([7, 0, NL - 1, 7, 33]))
    assert one.seg_row.numel() == 1
    y0 = spmm(one, xl, None, None, None, order=0, **kw)
    for chunk in (1, 16):
        y1 = spmm(one, xl, None, None, None, order=1, chunk=chunk,
                  out=_nan_out(1, F, torch.float32), **kw)
        _same(y1, y0)


def test_repeat_and_streams():
    """A fresh counter per call: three calls in a row agree. No counter
    shared between streams: two calls running on two streams agree too."""
    from adaqp_amd.ops.kernels import spmm
    F = 256
    view = _main_view()
    xl, xr, s, d = _operands(F, torch.float32, True)
    ref = spmm(view, xl, xr, s, d, order=0)
    for _ in range(3):
        _same(spmm(view, xl, xr, s, d, order=1, chunk=3,
                   out=_nan_out(R, F, torch.float32)), ref)
    outs = [_nan_out(R, F, torch.float32) for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        spmm(view, xl, xr, s, d, order=1, chunk=1, out=outs[0])
    spmm(view, xl, xr, s, d, order=1, chunk=1, out=outs[1])
    torch.cuda.synchronize()
    _same(outs[0], ref)
    _same(outs[1], ref)


@pytest.fixture(scope='module')
def comm():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29811')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.ops.kernels import native
    native()
    c = Communicator()
    try:
        yield c
    finally:
        Communicator.shutdown()


def test_module_default_switch(comm, monkeypatch):
    """``sage_mean_layer`` forward + backward with the module default at 0 and
    at 1: same outputs and gradients, and the default reaches the native
    calls."""
    import adaqp_amd.ops.kernels as K
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models.common import FastLinear, sage_mean_layer
    from adaqp_amd.runtime import GraphEngine
    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    f_in, f_out = 256, 48
    g = random_partitioned_graph(2000, 20000, 64, 10, 1, seed=3)
    engine = GraphEngine(partition_all(g, 1)[0], RunMode('AdaQP'),
                         DistGNNType.DistSAGE, msg_dims=[64, f_in, f_in],
                         device=comm.device)
    engine.set_uniform_assignment(8)
    dev, n = comm.device, engine.graph.num_inner
    gen = torch.Generator().manual_seed(7)
    x0 = torch.relu(torch.randn(n, f_in, generator=gen)).to(dev)
    gout = torch.randn(n, f_out, generator=gen).to(dev)
    torch.manual_seed(5)
    lins = [FastLinear(f_in, f_out).to(dev) for _ in range(2)]

    seen = []
    C = K.native()
    for name in ('spmm_csr', 'spmm_csr_rowskip'):
        real = getattr(C, name)
        monkeypatch.setattr(
            C, name,
            lambda *a, _real=real: (seen.append(a[-2]), _real(*a))[1])
    res = []
    for order in (0, 1):
        monkeypatch.setattr(K, 'SPMM_ORDER', order)
        del seen[:]
        l1, l2 = copy.deepcopy(lins)
        x = x0.clone().requires_grad_(True)
        out = sage_mean_layer(engine, x, l1, l2, 1, True)
        out.backward(gout)
        assert seen and all(o == order for o in seen)
        res.append((out.detach(), x.grad, l1.weight.grad, l1.bias.grad,
                    l2.weight.grad, l2.bias.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
