"""Gradients of the fused SAGE dual linear and of FastLinear on the GPU
against float64 products of the exact inputs.

Bound for every GEMM-shaped result (forward, grad_input, grad_weight,
grad_bias as ``ones @ g``): the library accumulates in fp32, one rounding
per term of the reduction plus two for the epilogue (alpha/beta or bias,
and the final combine), each at most U32 relative to S = |a| @ |b|:
``(reduction length + 2) * U32 * S``, plus half a bf16 ulp where the result
is stored as bf16. The reduction length is N for grad_input and M for the
weight and bias grads. Nothing is sized from an output."""
import pytest
import torch

import kernel_oracles as O
from kernel_oracles import U32, bf16_half_ulp, _first

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = O.GEMM_SHAPES          # includes (130, 72, 8, 48) and (77, 40, 72, 16)


def check_product(name, got, a, b, add=None, stored_bf16=None):
    """got == a @ b (+ add) within (a.shape[1] + 2) * U32 * S (+ half a
    bf16 ulp if got is bf16, or holds a value that was: stored_bf16)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ref, S = a @ b, a.abs() @ b.abs()
    if add is not None:
        add = add.detach().cpu().double()
        ref, S = ref + add, S + add.abs()
    tol = (a.shape[1] + 2) * U32 * S
    if stored_bf16 is None:
        stored_bf16 = got.dtype == torch.bfloat16
    if stored_bf16:
        tol = tol + bf16_half_ulp(ref.abs() + tol)
    o = got.detach().cpu().double().reshape(ref.shape)
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f'{name}{list(i)} = {float(o[i])!r}, oracle {float(ref[i])!r} '
            f'(tol {float(tol[i]):.3e}, reduction {a.shape[1]}, {got.dtype}); '
            f'{int(bad.sum())} bad of {o.numel()}')


def _ones(n):
    return torch.ones(1, n, dtype=torch.float64)


def _dual_case(M, K1, K2, N):
    """gemm_case plus a second bias and a seeded bf16 upstream gradient."""
    x, h, w1, w2, b1 = O.gemm_case(M, K1, K2, N)
    gen = torch.Generator().manual_seed(M * 1000 + K2 + 7)
    b2 = torch.randn(N, generator=gen).bfloat16()
    g = torch.randn(M, N, generator=gen).bfloat16()
    return x, h, w1, w2, b1, b2, g


def _check_dual_grads(g, x, h, w1, w2, gx, gh, gw1, gw2, gb1, gb2, bf16=True):
    check_product('gx', gx, g, w1.t(), stored_bf16=bf16)
    check_product('gh', gh, g, w2.t(), stored_bf16=bf16)
    check_product('gw1', gw1, x.t(), g, stored_bf16=bf16)
    check_product('gw2', gw2, h.t(), g, stored_bf16=bf16)
    assert gb1 is not None and gb2 is not None
    assert torch.equal(gb1, gb2)
    check_product('gb', gb1, _ones(g.shape[0]), g, stored_bf16=bf16)


@pytest.mark.parametrize('M,K1,K2,N', SHAPES)
def test_fused_dual_linear_fn_forward_backward(M, K1, K2, N):
    from adaqp_amd.models.common import _FusedDualLinearFn
    x, h, w1, w2, b1, b2, g = _dual_case(M, K1, K2, N)
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, h, w1, w2, b1, b2)]
    out = _FusedDualLinearFn.apply(*leaves)
    assert out.dtype == torch.bfloat16
    O.check_dual_gemm(x, h, w1, w2, (b1 + b2), out)     # bias = bf16(b1 + b2)
    out.backward(g.to(DEV))
    grads = [t.grad for t in leaves]
    assert all(gr is not None and gr.dtype == torch.bfloat16 for gr in grads)
    _check_dual_grads(g, x, h, w1, w2, *grads)


def test_fused_dual_linear_fn_skips_unneeded_grads():
    from adaqp_amd.models.common import _FusedDualLinearFn
    x, h, w1, w2, b1, b2, g = _dual_case(*SHAPES[0])

    class Ctx:
        saved_tensors = tuple(t.to(DEV) for t in (x, h, w1, w2))
        needs_input_grad = (True, False, False, True, False, False)
    gx, gh, gw1, gw2, gb1, gb2 = _FusedDualLinearFn.backward(Ctx, g.to(DEV))
    assert gh is None and gw1 is None and gb1 is None and gb2 is None
    check_product('gx', gx, g, w1.t())
    check_product('gw2', gw2, h.t(), g)


def _linears(w1, w2, b1, b2):
    """FastLinear pair with fp32 master weights holding the case's values."""
    from adaqp_amd.models.common import FastLinear
    lins = []
    for w, b in ((w1, b1), (w2, b2)):
        lin = FastLinear(w.shape[0], w.shape[1]).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(w.float())
            lin.bias.copy_(b.float())
        lins.append(lin)
    return lins


@pytest.mark.parametrize('M,K1,K2,N', SHAPES)
def test_fused_dual_linear_fp32_master_weights(M, K1, K2, N, monkeypatch):
    from adaqp_amd.models.common import fused_dual_linear, fused_dual_linear_ok
    x, h, w1, w2, b1, b2, g = _dual_case(M, K1, K2, N)
    lin1, lin2 = _linears(w1, w2, b1, b2)
    xd = x.to(DEV).requires_grad_(True)
    hd = h.to(DEV).requires_grad_(True)
    monkeypatch.delenv('ADAQP_FUSED_SAGE', raising=False)
    assert fused_dual_linear_ok(xd, hd, N) is False
    monkeypatch.setenv('ADAQP_FUSED_SAGE', '1')
    assert fused_dual_linear_ok(xd, hd, N) is True
    out = fused_dual_linear(xd, hd, lin1, lin2)
    O.check_dual_gemm(x, h, w1, w2, (b1 + b2), out)
    out.backward(g.to(DEV))
    params = (lin1.weight, lin2.weight, lin1.bias, lin2.bias)
    assert all(p.grad is not None and p.grad.dtype == torch.float32
               for p in params)
    assert xd.grad.dtype == torch.bfloat16 and hd.grad.dtype == torch.bfloat16
    _check_dual_grads(g, x, h, w1, w2, xd.grad, hd.grad,
                      *(p.grad for p in params))


class _FakeGraph:
    def __init__(self, n):
        self.num_inner = n


class _FakeEngine:
    compute_dtype = torch.bfloat16

    def __init__(self, n):
        self.graph = _FakeGraph(n)


@pytest.mark.parametrize('M,K,N', [(130, 72, 48), (77, 40, 16)])
@pytest.mark.parametrize('fused', [True, False])
def test_sage_conv_fused_and_unfused(M, K, N, fused, monkeypatch):
    """DistSAGEConv 'mean' on a fixed h_neigh. Fused: the kernel's oracle.
    Unfused (two bf16 linears under autocast, then an add): the same fp32
    count — K + 2 roundings per GEMM against its own S, which sum to at
    most (2K + 2) * U32 * S, the add being exact in fp32 before it is
    stored — and three bf16 stores instead of one: each linear's output
    and their sum."""
    import adaqp_amd.models.sage as sage_mod
    x, h, w1, w2, b1, b2, _ = _dual_case(M, K, K, N)
    x_all = torch.cat([x, x[:9] + 1]).to(DEV)        # inner + 9 remote rows
    conv = sage_mod.DistSAGEConv(K, N, layer=0, aggregator_type='mean').to(DEV)
    with torch.no_grad():
        conv.fc_self.weight.copy_(w1.float())
        conv.fc_self.bias.copy_(b1.float())
        conv.fc_neigh.weight.copy_(w2.float())
        conv.fc_neigh.bias.copy_(b2.float())
    hd = h.to(DEV)
    monkeypatch.setattr(sage_mod, 'dist_aggregate',
                        lambda x_, e, layer, training: hd)
    if fused:
        monkeypatch.setenv('ADAQP_FUSED_SAGE', '1')
    else:
        monkeypatch.delenv('ADAQP_FUSED_SAGE', raising=False)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        out = conv(_FakeEngine(M), x_all)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    if fused:
        O.check_dual_gemm(x, h, w1, w2, (b1 + b2), out)
        return
    xd, hh, w1d, w2d = (t.double() for t in (x, h, w1, w2))
    r1 = xd @ w1d + b1.double()
    r2 = hh @ w2d + b2.double()
    ref = r1 + r2
    S = xd.abs() @ w1d.abs() + hh.abs() @ w2d.abs() + b1.double().abs() \
        + b2.double().abs()
    tol = (2 * K + 2) * U32 * S
    tol = tol + bf16_half_ulp(r1.abs() + tol) + bf16_half_ulp(r2.abs() + tol)
    tol = tol + bf16_half_ulp(ref.abs() + tol)
    o = out.cpu().double()
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        i, j = _first(bad)
        raise AssertionError(
            f'out[{i}, {j}] = {float(o[i, j])!r}, oracle {float(ref[i, j])!r} '
            f'(tol {float(tol[i, j]):.3e}); {int(bad.sum())} bad of {o.numel()}')


@pytest.mark.parametrize('bf16', [False, True])
def test_fast_linear_grads(bf16):
    """FastLinear forward and all three grads, M = 130 and then M = 77
    (a second ``_ones_row`` entry next to the first), fp32 and bf16 under
    autocast with fp32 master weights."""
    from adaqp_amd.models.common import FastLinear
    K, N = 72, 48
    gen = torch.Generator().manual_seed(4242)
    lin = FastLinear(K, N).to(DEV)
    w = torch.randn(K, N, generator=gen)
    b = torch.randn(N, generator=gen)
    if bf16:
        w, b = w.bfloat16().float(), b.bfloat16().float()
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    for M in (130, 77):
        x = torch.randn(M, K, generator=gen)
        g = torch.randn(M, N, generator=gen)
        if bf16:
            x, g = x.bfloat16().float(), g.bfloat16()
        xd = x.to(DEV).requires_grad_(True)
        lin.zero_grad()
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
            out = lin(xd)
        assert out.dtype == (torch.bfloat16 if bf16 else torch.float32)
        check_product('out', out, x, w, add=b.expand(M, N))
        out.backward(g.to(DEV))
        for t in (xd.grad, lin.weight.grad, lin.bias.grad):
            assert t is not None and t.dtype == torch.float32
        check_product('grad_bias', lin.bias.grad, _ones(M), g, stored_bf16=bf16)
        check_product('grad_weight', lin.weight.grad, x.t(), g, stored_bf16=bf16)
        check_product('grad_input', xd.grad, g, w.t(), stored_bf16=bf16)
