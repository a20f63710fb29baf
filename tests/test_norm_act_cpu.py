"""CPU tests of the fused LayerNorm -> ReLU -> dropout op: the float64
checkers of norm_oracles.py accept correct fp32 implementations and reject
each mutation below; mask properties; module, model, trainer and CLI
wiring of ``fused_norm``."""
import importlib.util
import math
import os
import types

import pytest
import torch
import torch.nn.functional as Fn

import norm_oracles as O
from adaqp_amd.ops import quant as Q
from adaqp_amd.ops import norm_relu_dropout, norm_relu_dropout_torch
from adaqp_amd.ops.norm_act import drop_scale, keep_mask

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = O.NORM_SEED
SHAPES = [(O.NORM_N, F) for F in O.NORM_FS + (O.NORM_F_TORCH,)] \
    + [(1, 17), (5, 256)]


def _grads(fn, x, w, b, dy):
    """fp32 forward + autograd backward of fn(x, w, b) -> (y, dx, dw, db)."""
    xf = x.float().clone().requires_grad_(True)
    w1 = w.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    y = fn(xf, w1, b1)
    y.backward(dy.float())
    return y.detach(), xf.grad, w1.grad, b1.grad


def _unfused(p, seed):
    def fn(x, w, b):
        y = torch.relu(Fn.layer_norm(x, (x.shape[1],), w, b))
        if p > 0:
            y = y * keep_mask(seed, x.shape[0], x.shape[1], p) * drop_scale(p)
        return y
    return fn


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
@pytest.mark.parametrize('p', O.NORM_PS)
@pytest.mark.parametrize('N,F', SHAPES)
def test_checkers_accept_fp32_implementations(N, F, p, dtype):
    """norm_relu_dropout_torch and torch's own layer_norm -> relu -> mask*s,
    both in fp32 with autograd backward, pass both checkers (bf16: the
    inputs are bf16-valued and the outputs rounded once)."""
    x, w, b, dy = O.norm_case(N, F, dtype)
    for fn in (lambda x_, w_, b_: norm_relu_dropout_torch(x_, w_, b_, p, SEED, True),
               _unfused(p, SEED)):
        y, dx, dw, db = _grads(fn, x, w, b, dy)
        O.check_norm_act_fwd(x, w, b, p, SEED, True, y.to(dtype))
        O.check_norm_act_bwd(x, w, b, p, SEED, True, dy, dx.to(dtype), dw, db)


def test_dispatch_on_cpu_is_the_torch_implementation():
    x, w, b, _ = O.norm_case(O.NORM_N, 100)
    y = norm_relu_dropout(x, w, b, 0.5, SEED, True)
    assert torch.equal(y, norm_relu_dropout_torch(x, w, b, 0.5, SEED, True))
    # eval ignores p: no zeros from dropout, no scaling
    ye = norm_relu_dropout(x, w, b, 0.9, SEED, False)
    assert torch.equal(ye, norm_relu_dropout(x, w, b, 0.0, SEED, True))
    O.check_norm_act_fwd(x, w, b, 0.9, SEED, False, ye)


# --------------------------------------------------------------------------
# mutations: one fp32 implementation with a switch per bug
# --------------------------------------------------------------------------

def _impl(x, w, b, dy, p, seed, eps=1e-5, *, no_eps=False, unbiased=False,
          strict_mask=False, no_scale=False, gate_ge=False, dw_no_s=False,
          dx_no_m2=False):
    """Manual fp32 forward + backward of the definition; returns
    (y, dx, dweight, dbias)."""
    N, F = x.shape
    x = x.float()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / ((F - 1) if unbiased else F)
    rstd = 1.0 / torch.sqrt(var + (0.0 if no_eps else eps))
    xhat = d * rstd
    z = xhat * w + b
    if p > 0:
        u = Q.uniform_noise(seed & 0xFFFFFFFF, torch.arange(N), F)
        pf = torch.tensor(p, dtype=torch.float32)
        keep = (u > pf) if strict_mask else (u >= pf)
        s = drop_scale(p)
    else:
        keep, s = torch.ones(N, F, dtype=torch.bool), 1.0
    s_out = 1.0 if no_scale else s
    y = torch.relu(z) * keep * s_out
    gate = ((z >= 0) if gate_ge else (z > 0)) & keep
    g = dy.float() * s * gate
    a = g * w
    m1 = a.mean(1, keepdim=True)
    m2 = (a * xhat).mean(1, keepdim=True)
    dx = rstd * (a - m1 - (0.0 if dx_no_m2 else xhat * m2))
    dw = (g * xhat).sum(0) / (s if dw_no_s else 1.0)
    db = g.sum(0)
    return y, dx, dw, db


def _check(x, w, b, dy, p, seed, out):
    y, dx, dw, db = out
    O.check_norm_act_fwd(x, w, b, p, seed, True, y)
    O.check_norm_act_bwd(x, w, b, p, seed, True, dy, dx, dw, db)


def _zero_const_case():
    """The F=100 case with the constant row at 0 and bias 0 on it: there
    z is exactly 0 in every arithmetic (dz = 0), so the gate is not free."""
    x, w, b, dy = (t.clone() for t in O.norm_case(O.NORM_N, 100))
    x[O.CONST_ROW] = 0.0
    return x, w, torch.zeros_like(b), dy


def _tie_p(x, w, b):
    """p equal to one element's uniform01 value, at an element whose
    output is clearly positive: `>` drops it, `>=` keeps it."""
    N, F = x.shape
    u = Q.uniform_noise(SEED & 0xFFFFFFFF, torch.arange(N), F)
    y0 = norm_relu_dropout_torch(x, w, b, 0.0, SEED, True)
    cand = (u > 0.3) & (u < 0.7) & (y0 > 0.1)
    i, f = torch.nonzero(cand)[0].tolist()
    return float(u[i, f]), (i, f)


def test_unmutated_implementation_passes():
    x, w, b, dy = O.norm_case(O.NORM_N, 100)
    _check(x, w, b, dy, 0.5, SEED, _impl(x, w, b, dy, 0.5, SEED))
    p, _ = _tie_p(x, w, b)
    _check(x, w, b, dy, p, SEED, _impl(x, w, b, dy, p, SEED))
    x, w, b, dy = _zero_const_case()
    _check(x, w, b, dy, 0.5, SEED, _impl(x, w, b, dy, 0.5, SEED))


@pytest.mark.parametrize('mutation', ['no_eps', 'unbiased', 'no_scale',
                                      'dw_no_s', 'dx_no_m2'])
def test_mutation_rejected(mutation):
    x, w, b, dy = O.norm_case(O.NORM_N, 100)
    out = _impl(x, w, b, dy, 0.5, SEED, **{mutation: True})
    with pytest.raises(AssertionError):
        _check(x, w, b, dy, 0.5, SEED, out)


def test_mutation_strict_mask_rejected():
    x, w, b, dy = O.norm_case(O.NORM_N, 100)
    p, (i, f) = _tie_p(x, w, b)
    u = Q.uniform_noise(SEED & 0xFFFFFFFF, torch.arange(O.NORM_N), 100)
    assert float(u[i, f]) == p                 # some u == p on this input
    out = _impl(x, w, b, dy, p, SEED, strict_mask=True)
    with pytest.raises(AssertionError, match=rf'y\[{i}, {f}\]'):
        O.check_norm_act_fwd(x, w, b, p, SEED, True, out[0])


def test_mutation_gate_ge_rejected():
    x, w, b, dy = _zero_const_case()
    y, dx, dw, db = _impl(x, w, b, dy, 0.5, SEED, gate_ge=True)
    O.check_norm_act_fwd(x, w, b, 0.5, SEED, True, y)    # forward is the same
    with pytest.raises(AssertionError, match=rf'dx\[{O.CONST_ROW}, '):
        O.check_norm_act_bwd(x, w, b, 0.5, SEED, True, dy, dx, dw, db)


def test_free_gate_cap_raises():
    """A constant non-zero row with bias 0 makes the whole row free gates
    (1/37 of the input): the checker refuses the input itself."""
    x, w, b, dy = (t.clone() for t in O.norm_case(O.NORM_N, 100))
    b = torch.zeros_like(b)
    out = _impl(x, w, b, dy, 0.0, SEED)
    with pytest.raises(AssertionError, match='free ReLU gates'):
        O.check_norm_act_bwd(x, w, b, 0.0, SEED, True, dy, *out[1:])


def test_gradcheck_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(5, 7, generator=gen, dtype=torch.float64, requires_grad=True)
    w = (torch.rand(7, generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
    b = torch.randn(7, generator=gen, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda x_, w_, b_: norm_relu_dropout_torch(x_, w_, b_, 0.5, 12345, True),
        (x, w, b))


# --------------------------------------------------------------------------
# mask
# --------------------------------------------------------------------------

def test_mask_is_the_quant_hash():
    N, F, p = 64, 256, 0.5
    x = torch.ones(N, F)
    w, b = torch.zeros(F), torch.ones(F)          # y = keep * s
    y = norm_relu_dropout_torch(x, w, b, p, SEED, True)
    keep = Q.uniform_noise(SEED & 0xFFFFFFFF, torch.arange(N), F) \
        >= torch.tensor(p, dtype=torch.float32)
    assert torch.equal(y != 0, keep)
    assert torch.equal(y[keep], torch.full_like(y[keep], drop_scale(p)))
    # only the low 32 bits of the seed count
    y2 = norm_relu_dropout_torch(x, w, b, p, SEED + 2 ** 32, True)
    assert torch.equal(y, y2)
    y3 = norm_relu_dropout_torch(x, w, b, p, SEED + 1, True)
    assert not torch.equal(y != 0, y3 != 0)
    # keep fraction: n Bernoulli(1-p) draws, sigma = sqrt(p(1-p)/n)
    n = N * F
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(float(keep.float().mean()) - (1 - p)) <= 4 * sigma


@pytest.mark.parametrize('p', [1.0, -0.1])
def test_bad_p_raises(p):
    x, w, b, _ = O.norm_case(5, 256)
    with pytest.raises(ValueError):
        norm_relu_dropout(x, w, b, p, 1, True)
    with pytest.raises(ValueError):
        norm_relu_dropout_torch(x, w, b, p, 1, True)


# --------------------------------------------------------------------------
# module and model wiring
# --------------------------------------------------------------------------

@pytest.fixture
def world1(monkeypatch):
    """In-process gloo world of one rank + a tiny graph engine factory."""
    from adaqp_amd.comm import Communicator
    monkeypatch.delenv('ADAQP_FUSED_NORM', raising=False)
    monkeypatch.setenv('MASTER_ADDR', '127.0.0.1')
    monkeypatch.setenv('MASTER_PORT', '29466')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('WORLD_SIZE', '1')
    comm = Communicator(backend='gloo')
    try:
        yield comm
    finally:
        Communicator.shutdown()


def _engine(kind):
    from adaqp_amd.graph import partition_all, tiny_ring_graph
    from adaqp_amd.helpers import RunMode
    from adaqp_amd.runtime import GraphEngine
    torch.manual_seed(7)
    g = tiny_ring_graph(40, feat_dim=6, num_classes=3, extra_edges=60)
    lg = partition_all(g, 1)[0]
    engine = GraphEngine(lg, RunMode('Vanilla'), kind, msg_dims=[6, 8, 8],
                         device=torch.device('cpu'))
    return engine, lg


def _models():
    from adaqp_amd.helpers import DistGNNType
    from adaqp_amd.models import DistGCN, DistSAGE
    return ((DistGCN, DistGNNType.DistGCN), (DistSAGE, DistGNNType.DistSAGE))


def test_state_dict_loads_both_ways():
    for cls, _ in _models():
        torch.manual_seed(1)
        plain = cls(6, 8, 3, 3, fused_norm=False)
        fused = cls(6, 8, 3, 3, fused_norm=True)
        assert list(plain.state_dict()) == list(fused.state_dict())
        for k, v in plain.state_dict().items():
            assert fused.state_dict()[k].shape == v.shape, k
        with torch.no_grad():
            for n in plain.norms:
                n.weight.uniform_(0.5, 1.5)
                n.bias.uniform_(-1, 1)
        fused.load_state_dict(plain.state_dict(), strict=True)
        assert torch.equal(fused.norms[1].weight, plain.norms[1].weight)
        back = cls(6, 8, 3, 3, fused_norm=False)
        back.load_state_dict(fused.state_dict(), strict=True)
        assert torch.equal(back.norms[0].bias, plain.norms[0].bias)


def test_fused_model_equals_unfused_in_float64(world1):
    """dropout = 0: the two stacks are the same function, so in float64
    logits and parameter grads agree to rounding (1e-10 relative)."""
    for cls, kind in _models():
        engine, lg = _engine(kind)
        engine.compute_dtype = torch.float64
        torch.manual_seed(3)
        plain = cls(6, 8, 3, 3, dropout=0.0, fused_norm=False).double()
        with torch.no_grad():
            for n in plain.norms:
                n.weight.uniform_(0.5, 1.5)
                n.bias.uniform_(-0.5, 0.5)
        fused = cls(6, 8, 3, 3, dropout=0.0, fused_norm=True).double()
        fused.load_state_dict(plain.state_dict(), strict=True)
        feats = lg.feats.double()
        outs = []
        for model in (plain, fused):
            model.train()
            logits = model(engine, feats)
            Fn.cross_entropy(logits, lg.labels).backward()
            outs.append((logits.detach(),
                         {k: p.grad for k, p in model.named_parameters()}))
        (l0, g0), (l1, g1) = outs

        def close(a, b):
            return float((a - b).abs().max()) <= 1e-10 * float(a.abs().max())
        assert l0.dtype == torch.float64 and close(l0, l1)
        for k in g0:
            assert g1[k] is not None and close(g0[k], g1[k]), k


def test_fused_model_masks_and_eval(world1):
    from adaqp_amd.helpers import DistGNNType
    from adaqp_amd.models import DistSAGE, FusedNormReluDropout
    engine, lg = _engine(DistGNNType.DistSAGE)
    torch.manual_seed(4)
    model = DistSAGE(6, 8, 3, 3, dropout=0.5, fused_norm=True)
    assert all(isinstance(n, FusedNormReluDropout) for n in model.norms)
    seen = []
    hook = model.norms[0].register_forward_hook(
        lambda m, inp, out: seen.append((m.last_seed, out.detach() == 0)))
    model.train()
    model(engine, lg.feats)
    model(engine, lg.feats)
    hook.remove()
    (s0, z0), (s1, z1) = seen
    assert s0 != s1 and not torch.equal(z0, z1)      # a fresh mask per call
    assert model.norms[0].last_seed != model.norms[1].last_seed
    # eval: plain relu(layer_norm(x)), no dropout zeros, no scaling
    model.eval()
    cap = []
    model.norms[0].register_forward_hook(
        lambda m, inp, out: cap.append((inp[0].detach(), out.detach())))
    model(engine, lg.feats)
    x, y = cap[0]
    n0 = model.norms[0]
    ref = torch.relu(Fn.layer_norm(x, (8,), n0.weight, n0.bias))
    assert torch.allclose(y, ref, rtol=1e-5, atol=1e-6)
    O.check_norm_act_fwd(x, n0.weight.detach(), n0.bias.detach(), 0.5, 0,
                         False, y)


def test_fused_norm_flag_resolution(monkeypatch):
    from adaqp_amd.models import DistGCN, DistSAGE, FusedNormReluDropout
    for cls in (DistGCN, DistSAGE):
        monkeypatch.delenv('ADAQP_FUSED_NORM', raising=False)
        assert not cls(6, 8, 3, 3).fused_norm
        assert isinstance(cls(6, 8, 3, 3).norms[0], torch.nn.LayerNorm)
        assert cls(6, 8, 3, 3, fused_norm=True).fused_norm
        monkeypatch.setenv('ADAQP_FUSED_NORM', '1')
        m = cls(6, 8, 3, 3)
        assert m.fused_norm and isinstance(m.norms[0], FusedNormReluDropout)
        assert m.norms[0].p == 0.5 and m.norms[1].layer == 1
        assert not cls(6, 8, 3, 3, fused_norm=False).fused_norm   # explicit wins
        m = cls(6, 8, 3, 3, use_norm=False, fused_norm=True)
        assert not m.fused_norm and m.norms is None


def test_trainer_passes_fused_norm_from_config(monkeypatch):
    from adaqp_amd.helpers import DistGNNType
    from adaqp_amd.runtime.trainer import Trainer
    monkeypatch.delenv('ADAQP_FUSED_NORM', raising=False)
    for flag, want in ((True, True), (False, False), (None, False)):
        t = Trainer.__new__(Trainer)
        t.cfg = {'model': {'num_layers': 3, 'dropout': 0.5, 'use_norm': True,
                           'hidden_dim': 8, 'aggregator_type': 'mean'},
                 'runtime': {'lr': 0.01}}
        if flag is not None:
            t.cfg['model']['fused_norm'] = flag
        t.model_type = DistGNNType.DistSAGE
        t.feat_dim, t.num_classes = 6, 3
        t.comm = types.SimpleNamespace(device=torch.device('cpu'),
                                       sync_model_params=lambda m: None)
        t._set_model()
        assert t.model.fused_norm is want


def test_main_parses_fused_norm():
    spec = importlib.util.spec_from_file_location(
        'adaqp_main', os.path.join(REPO, 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    assert parser.parse_args(['--fused_norm']).fused_norm is True
    assert parser.parse_args([]).fused_norm is False
