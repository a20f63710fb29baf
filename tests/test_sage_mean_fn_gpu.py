"""The one-node SAGE 'mean' layer (``sage_mean_layer``) against the
formulation it replaces, written out here: ``dist_aggregate``, two
``FastLinear`` and an add, on a tiny world-1 engine.

The forward runs the same calls, and the backward the same GEMMs; the
input grad is the same two terms added with one rounding (in the SpMM
epilogue, or in x's dtype when that differs from the compute dtype), so
output, input grad and weight grads must be ``torch.equal``. The two
bias grads are one column sum: equal to each other and within its bound;
on the default path (``ones @ g``, as the parent) also ``torch.equal``
to the parent's, with ``ADAQP_COLSUM=1`` from the native kernel."""
import copy
import os

import pytest
import torch

from test_colsum_gpu import check_colsum

pytestmark = pytest.mark.gpu

F_IN, F_OUT, LAYER = 256, 48, 1


@pytest.fixture(scope='module')
def world1():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29793')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.ops.kernels import native
    native()
    comm = Communicator()
    try:
        g = random_partitioned_graph(2000, 20000, 64, 10, 1, seed=3)
        yield comm, partition_all(g, 1)[0]
    finally:
        Communicator.shutdown()


def _engine(world1, cdt):
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.runtime import GraphEngine
    comm, lg = world1
    engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                         msg_dims=[64, F_IN, F_IN], device=comm.device)
    engine.compute_dtype = cdt
    engine.set_uniform_assignment(8)
    return engine


def _parent(engine, x, lin1, lin2):
    from adaqp_amd.ops.dist_agg import dist_aggregate
    h = dist_aggregate(x, engine, LAYER, True)
    return lin1(x[:engine.graph.num_inner]) + lin2(h)


def _node(engine, x, lin1, lin2):
    from adaqp_amd.models.common import sage_mean_layer
    return sage_mean_layer(engine, x, lin1, lin2, LAYER, True)


# (compute dtype, x dtype): fp32; bf16 autocast over fp32 activations, as
# the layer stack runs it; bf16 activations (the addend epilogue in bf16)
@pytest.mark.parametrize('native_colsum', [False, True])
@pytest.mark.parametrize('x_grad', [True, False])
@pytest.mark.parametrize('cdt,xdt', [(torch.float32, torch.float32),
                                     (torch.bfloat16, torch.float32),
                                     (torch.bfloat16, torch.bfloat16)])
def test_sage_mean_node_matches_parent(world1, cdt, xdt, x_grad,
                                       native_colsum, monkeypatch):
    from adaqp_amd.models.common import FastLinear
    monkeypatch.delenv('ADAQP_COLSUM', raising=False)
    engine = _engine(world1, cdt)
    dev = world1[0].device
    n = engine.graph.num_inner
    gen = torch.Generator().manual_seed(77)
    x0 = torch.randn(n, F_IN, generator=gen).to(xdt).to(dev)
    g = torch.randn(n, F_OUT, generator=gen).to(cdt).to(dev)
    torch.manual_seed(5)
    lins = [FastLinear(F_IN, F_OUT).to(dev) for _ in range(2)]
    with torch.no_grad():
        for lin in lins:
            lin.bias.copy_(torch.randn(F_OUT, generator=gen))
    bf16 = cdt == torch.bfloat16
    res = []
    for fn in (_parent, _node):
        if fn is _node and native_colsum:
            monkeypatch.setenv('ADAQP_COLSUM', '1')
        l1, l2 = copy.deepcopy(lins)
        x = x0.clone().requires_grad_(x_grad)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
            out = fn(engine, x, l1, l2)
        assert out.dtype == cdt
        out.backward(g)
        res.append((out.detach(), x.grad, l1, l2))
    (o_p, gx_p, p1, p2), (o_n, gx_n, n1, n2) = res
    assert torch.equal(o_n, o_p)
    if x_grad:
        assert gx_n.dtype == xdt and torch.equal(gx_n, gx_p)
    else:
        assert gx_n is None and gx_p is None
    for a, b in ((n1, p1), (n2, p2)):
        assert a.weight.grad.dtype == torch.float32
        assert torch.equal(a.weight.grad, b.weight.grad)
    assert torch.equal(n1.bias.grad, n2.bias.grad)
    assert n1.bias.grad.dtype == torch.float32
    if not native_colsum:
        assert torch.equal(n1.bias.grad, p1.bias.grad)
        assert torch.equal(n2.bias.grad, p2.bias.grad)
    # fp32 master bias grad holds a value that was stored as bf16 under bf16
    check_colsum(n1.bias.grad.to(cdt), g)
