"""CPU tests of the masked loss: ``masked_loss_torch`` and both
``compute_loss`` paths against the float64 oracle of loss_oracles.py within
its bounds, the checkers' rejection of planted faults, and the wiring of
the ``fused_loss`` switch through compute_loss, train_epoch, the Trainer
and the CLI."""
import importlib.util
import os
import subprocess
import sys
import types

import pytest
import torch

import loss_oracles as O
from adaqp_amd.ops import loss as L
from adaqp_amd.ops import masked_loss, masked_loss_torch
from adaqp_amd.runtime.utils import compute_loss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['fp32', 'bf16']
KINDS = [False, True]
KIND_IDS = ['ce', 'bce']
CS = O.LOSS_CS + (O.LOSS_C_TORCH,)


def _run(fn, z, labels, mask, multilabel, g=O.LOSS_G):
    zg = z.clone().requires_grad_(True)
    loss = fn(zg, labels, mask, multilabel)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * g).backward()
    return loss.detach(), zg.grad


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('C', CS)
def test_torch_definition_within_bounds(C, multilabel, dtype):
    for N, scale in ((65, 1.0), (257, 8.0), (63, 30.0)):
        z, labels, mask = O.loss_case(N, C, multilabel, dtype, scale=scale)
        loss, dz = _run(masked_loss_torch, z, labels, mask, multilabel)
        O.check_loss(z, labels, mask, multilabel, loss)
        O.check_grad(z, labels, mask, multilabel, O.LOSS_G, dz)


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('density', [0.0, 1.0])
def test_torch_definition_uniform_masks(density, multilabel):
    z, labels, mask = O.loss_case(65, 47, multilabel, torch.float32,
                                  density=density)
    loss, dz = _run(masked_loss_torch, z, labels, mask, multilabel)
    O.check_loss(z, labels, mask, multilabel, loss)
    O.check_grad(z, labels, mask, multilabel, O.LOSS_G, dz)
    if density == 0.0:
        assert float(loss) == 0.0 and not dz.view(torch.int32).any()


def test_out_of_range_label_in_a_masked_row_is_nan():
    z, labels, mask = O.loss_case(65, 47, False, torch.float32, extremes=False)
    labels = labels.clone()
    labels[int(torch.nonzero(mask)[0])] = 47
    loss, dz = _run(masked_loss_torch, z, labels, mask, False)
    assert torch.isnan(loss)
    assert not dz[~mask].view(torch.int32).any()


def test_dispatch_on_cpu_is_the_torch_definition():
    for multilabel in KINDS:
        z, labels, mask = O.loss_case(65, 47, multilabel, torch.float32)
        before = L.calls
        a, da = _run(masked_loss, z, labels, mask, multilabel)
        assert L.calls == before + 1
        b, db = _run(masked_loss_torch, z, labels, mask, multilabel)
        assert torch.equal(a, b) and torch.equal(da, db)
    with pytest.raises(ValueError):
        masked_loss(z, labels, mask[:-1], True)
    with pytest.raises(ValueError):
        masked_loss(z, labels[:, :-1], mask, True)
    with pytest.raises(ValueError):
        masked_loss(z[0], labels, mask, True)


def test_float64_runs_in_float64():
    z, labels, mask = O.loss_case(65, 47, False, torch.float32)
    loss = masked_loss(z.double(), labels, mask, False)
    assert loss.dtype == torch.float64
    ref, _, _, _ = O.oracle(z, labels, mask, False)
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref))


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_compute_loss_fused_and_unfused_within_bound(multilabel):
    """global_count is a power of two, so the division is exact and the
    raw sum is recovered exactly. The -inf logit is left out: torch's own
    BCE gives NaN for it."""
    gc = torch.tensor([64.0])
    for C in (47, 107):
        z, labels, mask = O.loss_case(257, C, multilabel, torch.float32,
                                      extremes=False)
        for fused in (True, False):
            loss = compute_loss(z, labels, mask, multilabel, gc, fused=fused)
            O.check_loss(z, labels, mask, multilabel, loss.reshape(()) * 64.0)


# ---------------------------------------------------------------------------
# the checkers bite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_checkers_reject_planted_faults(multilabel):
    z, labels, mask = O.loss_case(257, 47, multilabel, torch.float32,
                                  extremes=False)
    loss, dz = _run(masked_loss_torch, z, labels, mask, multilabel)
    O.check_loss(z, labels, mask, multilabel, loss)
    O.check_grad(z, labels, mask, multilabel, O.LOSS_G, dz)
    # an oracle fed the wrong mask: one masked row dropped
    wrong = mask.clone()
    wrong[int(torch.nonzero(mask)[-1])] = False
    with pytest.raises(AssertionError):
        O.check_loss(z, labels, wrong, multilabel, loss)
    with pytest.raises(AssertionError):
        O.check_grad(z, labels, wrong, multilabel, O.LOSS_G, dz)
    # the label shifted by one in the masked rows
    if multilabel:
        shifted = labels.roll(1, dims=1)
    else:
        shifted = torch.where(mask, (labels + 1) % 47, labels)
    with pytest.raises(AssertionError):
        O.check_loss(z, shifted, mask, multilabel, loss)
    with pytest.raises(AssertionError):
        O.check_grad(z, shifted, mask, multilabel, O.LOSS_G, dz)
    # the wrong upstream gradient, a gradient off by 2^-16, a stray value
    # in an unmasked row, a -0.0 there, a non-finite loss
    with pytest.raises(AssertionError):
        O.check_grad(z, labels, mask, multilabel, 1.0, dz)
    r = int(torch.nonzero(mask)[-1])
    bad = dz.clone()
    bad[r, 3] += 2.0 ** -16
    with pytest.raises(AssertionError):
        O.check_grad(z, labels, mask, multilabel, O.LOSS_G, bad)
    for stray in (1e-30, -0.0, float('nan')):
        bad = dz.clone()
        bad[int(torch.nonzero(~mask)[-1]), 5] = stray
        with pytest.raises(AssertionError):
            O.check_grad(z, labels, mask, multilabel, O.LOSS_G, bad)
    with pytest.raises(AssertionError):
        O.check_loss(z, labels, mask, multilabel, loss * float('nan'))
    with pytest.raises(AssertionError):
        O.check_loss(z, labels, mask, multilabel, loss * (1 + 2.0 ** -10))
    with pytest.raises(AssertionError):
        O.check_grad(z, labels, mask, multilabel, O.LOSS_G, dz.bfloat16())


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------
def test_switch_precedence(monkeypatch):
    z, labels, mask = O.loss_case(65, 47, False, torch.float32, extremes=False)
    gc = torch.tensor([64.0])

    def entered(**kw):
        before = L.calls
        compute_loss(z, labels, mask, False, gc, **kw)
        return L.calls - before

    monkeypatch.delenv('ADAQP_FUSED_LOSS', raising=False)
    assert not L.resolve_fused_loss(None)
    assert entered() == 0 and entered(fused=None) == 0
    assert entered(fused=True) == 1
    monkeypatch.setenv('ADAQP_FUSED_LOSS', '1')
    assert L.resolve_fused_loss(None)
    assert entered() == 1
    assert entered(fused=False) == 0         # an explicit bool wins
    assert not L.resolve_fused_loss(False) and L.resolve_fused_loss(True)
    monkeypatch.setenv('ADAQP_FUSED_LOSS', '0')
    assert entered() == 0 and entered(fused=True) == 1


@pytest.fixture
def world1(monkeypatch):
    from adaqp_amd.comm import Communicator
    monkeypatch.delenv('ADAQP_FUSED_LOSS', raising=False)
    monkeypatch.setenv('MASTER_ADDR', '127.0.0.1')
    monkeypatch.setenv('MASTER_PORT', '29467')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '1')
    comm = Communicator(backend='gloo')
    try:
        yield comm
    finally:
        Communicator.shutdown()


def test_train_epoch_switch(world1, monkeypatch):
    """train_epoch enters the op once per epoch when told to, by argument
    or by the env var, and never otherwise; both paths see the same
    first-epoch logits and give losses within the oracle's bound."""
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import global_train_count, train_epoch
    g = random_partitioned_graph(300, 3000, 16, 7, 1, seed=5)
    lg = partition_all(g, 1)[0]

    def run(epochs, **kw):
        engine = GraphEngine(lg, RunMode('Vanilla'), DistGNNType.DistSAGE,
                             msg_dims=[16, 16, 16],
                             device=torch.device('cpu'))
        torch.manual_seed(0)
        model = DistSAGE(16, 16, 7, 3, dropout=0.0)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        cap = []
        model.register_forward_hook(
            lambda m, inp, out: cap.append(out.detach().clone()))
        gc = global_train_count(engine)
        before = L.calls
        losses = [train_epoch(engine, model, opt, gc, False, **kw)
                  for _ in range(epochs)]
        return cap[0], losses, L.calls - before, engine, float(gc)

    z_on, l_on, n_on, engine, gc = run(3, fused_loss=True)
    z_off, l_off, n_off, _, _ = run(3, fused_loss=False)
    assert n_on == 3 and n_off == 0
    assert torch.equal(z_on, z_off)
    labels, mask = engine.graph.labels, engine.graph.train_mask
    # the division by the train count is one more rounding: u * |L|
    for loss in (l_on[0], l_off[0]):
        raw = loss.double().reshape(()) * gc
        O.check_loss(z_on, labels, mask, False, raw,
                     extra=O.U32 * abs(float(raw)))
    assert run(1)[2] == 0
    monkeypatch.setenv('ADAQP_FUSED_LOSS', '1')
    assert run(1)[2] == 1
    assert run(1, fused_loss=False)[2] == 0


def test_trainer_passes_fused_loss_from_config(monkeypatch):
    import adaqp_amd.runtime.trainer as T
    monkeypatch.delenv('ADAQP_FUSED_LOSS', raising=False)
    seen = []

    def fake_train_epoch(engine, model, optimizer, gc, multilabel,
                         fused_loss=None):
        seen.append(fused_loss)
        return torch.zeros(())

    monkeypatch.setattr(T, 'train_epoch', fake_train_epoch)
    monkeypatch.setattr(T, 'global_train_count', lambda engine: None)
    monkeypatch.setattr(T, 'evaluate', lambda engine, model, multilabel: {})
    assert 'fused_loss' not in T.load_config('reddit')['runtime']
    for flag in (True, False, None):
        t = T.Trainer.__new__(T.Trainer)
        t.cfg = {'runtime': {'num_epochs': 1, 'log_steps': 1000,
                             'eval_every': 1000}}
        if flag is not None:
            t.cfg['runtime']['fused_loss'] = flag
        t.args = types.SimpleNamespace()
        t.mode = types.SimpleNamespace(
            bit_type=types.SimpleNamespace(name='FULL'))
        t.engine = types.SimpleNamespace(
            device=torch.device('cpu'),
            timer=types.SimpleNamespace(enabled=False))
        t.model = t.optimizer = None
        t.multilabel = False
        t.comm = types.SimpleNamespace(rank=1)
        t.epoch_times = []
        t.recorder = types.SimpleNamespace(add=lambda metrics, epoch: None,
                                           best=lambda: {})
        t.train(start_epoch=0)
    assert seen == [True, False, None]


def test_main_parses_fused_loss():
    spec = importlib.util.spec_from_file_location(
        'adaqp_main_loss', os.path.join(REPO, 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    assert parser.parse_args(['--fused_loss']).fused_loss is True
    assert parser.parse_args([]).fused_loss is False


def test_main_cli_runs_with_fused_loss(tmp_path):
    env = dict(os.environ, MASTER_PORT='29534')
    env.pop('ADAQP_FUSED_LOSS', None)
    subprocess.run(
        [sys.executable, 'graph_partition.py', '--dataset', 'reddit',
         '--partition_size', '1', '--scale', '0.002',
         '--partition_dir', str(tmp_path / 'parts')],
        cwd=REPO, check=True, capture_output=True, timeout=300)
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, 'main.py'), '--dataset', 'reddit',
         '--model_name', 'sage', '--mode', 'Vanilla', '--fused_loss',
         '--num_epochs', '3', '--log_steps', '1',
         '--partition_dir', str(tmp_path / 'parts')],
        cwd=str(tmp_path), env=env, capture_output=True, text=True,
        timeout=600)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-1500:])
    assert 'best:' in out.stdout
