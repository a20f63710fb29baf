"""``ADAQP_BWD_GATHER_BF16`` through one SAGE-mean and one GCN layer on a tiny
world-1 fp32 engine (the construction of test_sage_mean_fn_gpu.py).

With the switch on, the input gradient is the backward composed by hand from
``round_rows_bf16`` (with the seed the layer used) and the fp32 ``spmm`` on
the widened rows, bit for bit; with it off it is the plain fp32 backward.
Weight and bias gradients do not depend on the gather."""
import copy

import pytest
import torch

from test_sage_mean_fn_gpu import world1  # noqa: F401  (the tiny world-1 graph)

pytestmark = pytest.mark.gpu

F_IN, F_OUT, LAYER = 40, 24, 1


def _layer_backward(engine, model, lins, x0, g):
    """(input grad, [(weight grad, bias grad), ...]) of one layer."""
    from adaqp_amd.models.common import sage_mean_layer
    from adaqp_amd.ops.dist_agg import dist_aggregate
    lins = copy.deepcopy(lins)
    x = x0.clone().requires_grad_(True)
    if model == 'sage':
        out = sage_mean_layer(engine, x, lins[0], lins[1], LAYER, True)
    else:
        out = lins[1](dist_aggregate(x, engine, LAYER, True))
    out.backward(g)
    return x.grad, [(l.weight.grad, l.bias.grad) for l in lins
                    if l.weight.grad is not None]


@pytest.mark.parametrize('model', ['sage', 'gcn'])
def test_input_grad_is_the_hand_composed_backward(world1, model, monkeypatch):
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models.common import FastLinear
    from adaqp_amd.ops.dist_agg import bwd_gather_seed
    from adaqp_amd.ops.kernels import round_rows_bf16, spmm
    from adaqp_amd.runtime import GraphEngine
    monkeypatch.delenv('ADAQP_BWD_GATHER_BF16', raising=False)
    comm, lg = world1
    dev = comm.device
    sage = model == 'sage'
    engine = GraphEngine(lg, RunMode('AdaQP'),
                         DistGNNType.DistSAGE if sage else DistGNNType.DistGCN,
                         msg_dims=[64, F_IN, F_IN], device=dev)
    engine.set_uniform_assignment(8)
    assert engine.compute_dtype == torch.float32
    n = engine.graph.num_inner
    gen = torch.Generator().manual_seed(79)
    x0 = torch.randn(n, F_IN, generator=gen).to(dev)
    g = torch.randn(n, F_OUT, generator=gen).to(dev)
    torch.manual_seed(5)
    lins = [FastLinear(F_IN, F_OUT).to(dev) for _ in range(2)]
    with torch.no_grad():
        for lin in lins:
            lin.bias.copy_(torch.randn(F_OUT, generator=gen))

    # the operand of the backward SpMM, its scales and its addend
    gh = g @ lins[1].weight.t()
    if sage:
        src, dst, addend = engine.sage_src_b, None, g @ lins[0].weight.t()
    else:
        src, dst, addend = engine.gcn_src_b, engine.gcn_dst_b, None

    gx_off, wb_off = _layer_backward(engine, model, lins, x0, g)
    assert engine.bwd_gather_calls == 0
    assert torch.equal(gx_off, spmm(engine.full_view, gh, None, src, dst,
                                    addend=addend))

    monkeypatch.setenv('ADAQP_BWD_GATHER_BF16', '1')
    gx_on, wb_on = _layer_backward(engine, model, lins, x0, g)
    assert engine.bwd_gather_calls == 1
    rows = round_rows_bf16(gh, bwd_gather_seed(engine, LAYER, 0))
    assert rows.dtype == torch.bfloat16
    want = spmm(engine.full_view, rows.float(), None, src, dst, addend=addend)
    assert gx_on.dtype == torch.float32
    assert torch.equal(gx_on.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(gx_on, gx_off)
    assert len(wb_on) == len(wb_off) == (2 if sage else 1)
    for (w1, b1), (w0, b0) in zip(wb_on, wb_off):
        assert torch.equal(w1, w0) and torch.equal(b1, b0)
