"""``ADAQP_BWD_SKIP_ZERO`` through three training steps of a 3-layer DistSAGE.

The output layer's backward SpMM skips the gradient rows of the nodes outside
the train mask (about a third of this graph). That changes which rows are
fetched and nothing else, so with the switch on and off, from the same seed,
the loss, every gradient and every parameter must be the same bits after each
step. ``engine.bwd_skip_hits`` shows that the output layer took the
row-skipping path once per step and no other layer did; both propagation
paths (full and decomposed) are run."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, HIDDEN, LAYERS = 3, 32, 3


@pytest.fixture(scope='module')
def world1():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29797')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.ops.kernels import native
    native()
    comm = Communicator()
    try:
        g = random_partitioned_graph(3000, 30000, 64, 10, 1, seed=9)
        lg = partition_all(g, 1)[0]
        out = 1.0 - float(lg.train_mask.float().mean())
        assert 0.25 < out < 0.45, out
        yield comm, lg
    finally:
        Communicator.shutdown()


def _i32(t):
    return t.detach().contiguous().view(torch.int32)


def _train(world1, parallel, skip, monkeypatch):
    """[(loss, grads, params) after each step], skip-path hits, and the
    layers whose backward SpMM was given a liveness array."""
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import global_train_count, train_epoch
    monkeypatch.setenv('ADAQP_BWD_SKIP_ZERO', '1' if skip else '0')
    monkeypatch.delenv('ADAQP_BWD_GATHER_BF16', raising=False)
    comm, lg = world1
    engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                         msg_dims=[64, HIDDEN, HIDDEN], device=comm.device)
    engine.set_uniform_assignment(8)
    engine.use_parallel = parallel
    assert engine.compute_dtype == torch.float32
    torch.manual_seed(1234)
    model = DistSAGE(64, HIDDEN, 10, LAYERS).to(comm.device)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    gc = global_train_count(engine)

    layers = []
    import adaqp_amd.ops.dist_agg as da
    orig = da.propagate

    def spy(engine_, x, layer, is_train, mode, **kw):
        if kw.get('live') is not None:
            layers.append(layer)
        return orig(engine_, x, layer, is_train, mode, **kw)
    monkeypatch.setattr(da, 'propagate', spy)

    steps = []
    for _ in range(STEPS):
        loss = train_epoch(engine, model, opt, gc, multilabel=False)
        steps.append((_i32(loss).clone(),
                      [_i32(p.grad).clone() for p in model.parameters()],
                      [_i32(p).clone() for p in model.parameters()]))
    torch.cuda.synchronize()
    monkeypatch.setattr(da, 'propagate', orig)
    return steps, engine.bwd_skip_hits, layers


@pytest.mark.parametrize('parallel', [False, True],
                         ids=['full', 'decomposed'])
def test_training_is_the_same_bits_with_and_without_the_skip(
        world1, parallel, monkeypatch):
    on, hits_on, layers_on = _train(world1, parallel, True, monkeypatch)
    off, hits_off, layers_off = _train(world1, parallel, False, monkeypatch)
    assert hits_on == STEPS and layers_on == [LAYERS - 1] * STEPS
    assert hits_off == 0 and layers_off == []
    for step, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a[0], b[0]), f'loss differs at step {step}'
        assert torch.isfinite(a[0].view(torch.float32)).all()
        for k, (x, y) in enumerate(zip(a[1], b[1])):
            assert torch.equal(x, y), f'grad {k} differs at step {step}'
        for k, (x, y) in enumerate(zip(a[2], b[2])):
            assert torch.equal(x, y), f'param {k} differs at step {step}'
    # the steps did something: parameters moved between step 0 and step 2
    assert any(not torch.equal(x, y) for x, y in zip(on[0][2], on[-1][2]))
