"""The packed-gather hint through ``sage_mean_layer`` and ``DistSAGE``, and
the reuse of the layer-0 forward aggregate, on tiny world-1 engines.

The packed SpMM gives the dense SpMM's bits and the kept aggregate is the
tensor a recomputation would give, so everything compared here (outputs,
losses, logits, every gradient) must be ``torch.equal``."""
import copy
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def comm():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29797')
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


def _engine(comm, msg_dims):
    """A fresh graph per engine: LocalGraph.to moves in place and one test
    below changes the features."""
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.runtime import GraphEngine
    g = random_partitioned_graph(2000, 20000, 64, 10, 1, seed=3)
    engine = GraphEngine(partition_all(g, 1)[0], RunMode('AdaQP'),
                         DistGNNType.DistSAGE, msg_dims=msg_dims,
                         device=comm.device)
    engine.set_uniform_assignment(8)
    assert engine.graph.num_remote == 0
    return engine


def _count_packs(monkeypatch):
    import adaqp_amd.ops.kernels as K
    calls = []
    real = K.pack_rows

    def counting(x):
        p = real(x)
        calls.append(p is not None)
        return p
    monkeypatch.setattr(K, 'pack_rows', counting)
    return calls


@pytest.mark.parametrize('x_grad', [True, False])
@pytest.mark.parametrize('f_in,f_out', [(256, 48), (104, 256)])
def test_sage_mean_layer_hint_on_off(comm, f_in, f_out, x_grad, monkeypatch):
    from adaqp_amd.models.common import FastLinear, sage_mean_layer
    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    calls = _count_packs(monkeypatch)
    engine = _engine(comm, [64, f_in, f_in])
    dev, n = comm.device, engine.graph.num_inner
    gen = torch.Generator().manual_seed(7 + f_in)
    # relu + dropout(0.5): about a quarter of the elements survive
    x0 = torch.relu(torch.randn(n, f_in, generator=gen))
    x0 = (x0 * (torch.rand(n, f_in, generator=gen) < 0.5) * 2.0).to(dev)
    g = torch.randn(n, f_out, generator=gen).to(dev)
    torch.manual_seed(5)
    lins = [FastLinear(f_in, f_out).to(dev) for _ in range(2)]
    with torch.no_grad():
        for lin in lins:
            lin.bias.copy_(torch.randn(f_out, generator=gen))
    res = []
    for pack in (False, True):
        l1, l2 = copy.deepcopy(lins)
        x = x0.clone().requires_grad_(x_grad)
        out = sage_mean_layer(engine, x, l1, l2, 1, True, pack=pack)
        out.backward(g)
        res.append((out.detach(), x.grad, l1, l2))
    assert calls == [True]                   # packed once, in the hinted call
    (o_d, gx_d, d1, d2), (o_p, gx_p, p1, p2) = res
    assert torch.equal(o_p, o_d)
    if x_grad:
        assert torch.equal(gx_p, gx_d)
    else:
        assert gx_p is None and gx_d is None
    for a, b in ((p1, d1), (p2, d2)):
        assert torch.equal(a.weight.grad, b.weight.grad)
        assert torch.equal(a.bias.grad, b.bias.grad)


def test_distsage_packed_env_switch(comm, monkeypatch):
    """3-layer DistSAGE, same seed before each run so the dropout masks
    agree: ADAQP_SPMM_PACKED=1 against =0."""
    from adaqp_amd.models import DistSAGE
    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    monkeypatch.delenv('ADAQP_FUSED_NORM', raising=False)
    calls = _count_packs(monkeypatch)
    engine = _engine(comm, [64, 256, 256])
    torch.manual_seed(2)
    model0 = DistSAGE(64, 256, 10, 3).to(comm.device)
    res = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('ADAQP_SPMM_PACKED', flag)
        model = copy.deepcopy(model0).train()
        torch.manual_seed(123)
        logits = model(engine, engine.graph.feats)
        logits.square().sum().backward()
        res[flag] = (logits.detach(), [p.grad for p in model.parameters()])
        assert calls == ([] if flag == '0' else [True, True])
    assert torch.equal(res['0'][0], res['1'][0])
    assert len(res['0'][1]) == len(res['1'][1]) > 0
    for a, b in zip(res['0'][1], res['1'][1]):
        assert a is not None and torch.equal(a, b)


# ---------------------------------------------------------------------------
# layer-0 aggregate reuse
# ---------------------------------------------------------------------------

class _Run:
    """One engine + model + optimizer; ``epoch`` returns (loss, logits,
    grads) of one train_epoch with a fixed dropout seed."""

    def __init__(self, comm, model0, state=None):
        from adaqp_amd.runtime.utils import global_train_count
        self.engine = _engine(comm, [64, 32, 32])
        if state is None:
            self.model = copy.deepcopy(model0)
            self.opt = torch.optim.Adam(self.model.parameters(), lr=0.01)
        else:
            self.model, self.opt = copy.deepcopy(state)
            self.model._forward_hooks.clear()      # the source run's hook
        self.gc = global_train_count(self.engine)
        self.logits = None
        self.model.register_forward_hook(
            lambda m, a, out: setattr(self, 'logits', out.detach().clone()))

    def epoch(self, seed):
        from adaqp_amd.runtime.utils import train_epoch
        torch.manual_seed(seed)
        loss = train_epoch(self.engine, self.model, self.opt, self.gc,
                           multilabel=False)
        return (loss.clone(), self.logits,
                [p.grad.clone() for p in self.model.parameters()])

    def counters(self):
        return self.engine.agg0_misses, self.engine.agg0_hits


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == len(b[2]) > 0
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def test_layer0_aggregate_reuse(comm, monkeypatch):
    from adaqp_amd.models import DistSAGE
    torch.manual_seed(4)
    model0 = DistSAGE(64, 32, 10, 3).to(comm.device)

    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    off = _Run(comm, model0)
    ref = [off.epoch(100), off.epoch(101)]
    assert off.counters() == (0, 0)
    off.engine.graph.feats.mul_(2)
    ref.append(off.epoch(102))

    monkeypatch.delenv('ADAQP_AGG0_CACHE')
    on = _Run(comm, model0)
    _same(on.epoch(100), ref[0])
    assert on.counters() == (1, 0)
    _same(on.epoch(101), ref[1])
    assert on.counters() == (1, 1)
    # a fresh engine from the same model/optimizer state, features doubled
    fresh = _Run(comm, None, state=(on.model, on.opt))
    fresh.engine.graph.feats.mul_(2)
    # an in-place change of the features must miss and recompute
    on.engine.graph.feats.mul_(2)
    third = on.epoch(102)
    assert on.counters() == (2, 1)
    _same(third, ref[2])
    _same(fresh.epoch(102), third)
    assert fresh.counters() == (1, 0)
    assert not torch.equal(ref[2][1], ref[1][1])


def test_layer0_reuse_never_while_tracing(comm, monkeypatch):
    from adaqp_amd.models import DistSAGE
    monkeypatch.delenv('ADAQP_AGG0_CACHE', raising=False)
    torch.manual_seed(4)
    run = _Run(comm, DistSAGE(64, 32, 10, 3).to(comm.device))
    run.engine.is_tracing = True
    run.epoch(1)
    run.epoch(2)
    assert run.counters() == (0, 0)
    run.engine.is_tracing = False
    run.epoch(3)
    run.epoch(4)
    assert run.counters() == (1, 1)
