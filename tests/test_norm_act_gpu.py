"""Fused LayerNorm -> ReLU -> dropout HIP kernels vs the float64 oracles of
norm_oracles.py (GPU only). Shapes are the smallest that reach each path:
every vector width, idle lanes (F < 64), the register-staging limit
(F = 1024), a partial last block (N = 37) and a second trip of the
backward row loop."""
import os

import pytest
import torch

import norm_oracles as O
from adaqp_amd.ops import norm_relu_dropout
from adaqp_amd.ops.norm_act import (MAX_FEATS, bwd_launch_geometry,
                                    drop_scale, keep_mask)

pytestmark = pytest.mark.gpu

SEED = O.NORM_SEED
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['fp32', 'bf16']
FILL = -3.0


def _native():
    from adaqp_amd.ops.kernels import native
    return native()


def _fwd(x, w, b, p, seed, training, y=None):
    """Raw forward launch -> (y, mean, rstd) on the GPU."""
    N = x.shape[0]
    y = torch.empty_like(x) if y is None else y
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    rstd = torch.empty(N, dtype=torch.float32, device=x.device)
    _native().norm_act_fwd(x, w, b, 1e-5, p, seed & 0xFFFFFFFF, training,
                           y, mean, rstd)
    return y, mean, rstd


def _bwd(dy, x, mean, rstd, w, b, p, seed, training, dx=None):
    dx = torch.empty_like(x) if dx is None else dx
    dwb = _native().norm_act_bwd(dy, x, mean, rstd, w, b, p,
                                 seed & 0xFFFFFFFF, training, dx)
    return dx, dwb[0], dwb[1]


def _case(N, F, dtype):
    x, w, b, dy = O.norm_case(N, F, dtype)
    return (x, w, b, dy), tuple(t.cuda() for t in (x, w, b, dy))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('p', O.NORM_PS)
@pytest.mark.parametrize('F', O.NORM_FS)
def test_forward_exact(F, p, dtype):
    (x, w, b, _), (xg, wg, bg, _) = _case(O.NORM_N, F, dtype)
    y, mean, rstd = _fwd(xg, wg, bg, p, SEED, True)
    O.check_norm_act_fwd(x, w, b, p, SEED, True, y.cpu(), mean.cpu(), rstd.cpu())
    # eval ignores p (and the seed): the p = 0 result, bit for bit
    y0, _, _ = _fwd(xg, wg, bg, 0.0, 0, True)
    ye, _, _ = _fwd(xg, wg, bg, p, SEED, False)
    assert torch.equal(ye, y0)
    O.check_norm_act_fwd(x, w, b, p, SEED, False, ye.cpu())
    if p > 0:
        # weight 0, bias 1: y = keep * s exactly -> the mask, bit for bit
        ym, _, _ = _fwd(xg, torch.zeros_like(wg), torch.ones_like(bg), p, SEED, True)
        keep = keep_mask(SEED, O.NORM_N, F, p)
        assert torch.equal(ym.cpu() != 0, keep)
        s = torch.tensor(drop_scale(p)).to(dtype)
        assert torch.equal(ym.cpu()[keep], s.expand(int(keep.sum())))


def _autograd_bwd(N, F, p, dtype):
    (x, w, b, dy), (xg, wg, bg, dyg) = _case(N, F, dtype)
    xg = xg.clone().requires_grad_(True)
    wg = wg.clone().requires_grad_(True)
    bg = bg.clone().requires_grad_(True)
    y = norm_relu_dropout(xg, wg, bg, p, SEED, True)
    assert y.dtype == dtype
    y.backward(dyg)
    assert xg.grad.dtype == dtype and wg.grad.dtype == torch.float32
    O.check_norm_act_fwd(x, w, b, p, SEED, True, y.detach().cpu())
    O.check_norm_act_bwd(x, w, b, p, SEED, True, dy, xg.grad.cpu(),
                         wg.grad.cpu(), bg.grad.cpu())


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('p', O.NORM_PS)
@pytest.mark.parametrize('F', O.NORM_FS)
@pytest.mark.parametrize('N', [O.NORM_N, 1, 5])
def test_backward_exact(N, F, p, dtype):
    _autograd_bwd(N, F, p, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_backward_row_loop_second_trip(dtype):
    max_blocks, waves = bwd_launch_geometry()
    N = max_blocks * waves + 1
    assert N > max_blocks * waves        # some wave must visit a second row
    _autograd_bwd(N, 8, 0.5, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_backward_bit_reproducible(dtype):
    _, (xg, wg, bg, dyg) = _case(4101, 256, dtype)
    _, mean, rstd = _fwd(xg, wg, bg, 0.5, SEED, True)
    a = _bwd(dyg, xg, mean, rstd, wg, bg, 0.5, SEED, True)
    b = _bwd(dyg, xg, mean, rstd, wg, bg, 0.5, SEED, True)
    for name, t0, t1 in zip(('dx', 'dweight', 'dbias'), a, b):
        assert torch.equal(t0, t1), name


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('F', [17, 100, 256])
def test_nothing_else_written(F, dtype):
    """y and dx are row slices of larger filled buffers; the rows outside
    keep their fill."""
    N, lo = O.NORM_N, 3
    (x, w, b, dy), (xg, wg, bg, dyg) = _case(N, F, dtype)
    ybig = torch.full((N + 8, F), FILL, dtype=dtype, device='cuda')
    dbig = torch.full((N + 8, F), FILL, dtype=dtype, device='cuda')
    y, mean, rstd = _fwd(xg, wg, bg, 0.5, SEED, True, y=ybig[lo:lo + N])
    dx, dw, db = _bwd(dyg, xg, mean, rstd, wg, bg, 0.5, SEED, True,
                      dx=dbig[lo:lo + N])
    for big in (ybig, dbig):
        assert (big[:lo] == FILL).all() and (big[lo + N:] == FILL).all()
    O.check_norm_act_fwd(x, w, b, 0.5, SEED, True, y.cpu(), mean.cpu(), rstd.cpu())
    O.check_norm_act_bwd(x, w, b, 0.5, SEED, True, dy, dx.cpu(), dw.cpu(), db.cpu())


def test_dispatch_wide_rows_take_the_torch_path():
    F = O.NORM_F_TORCH
    assert F > MAX_FEATS
    (x, w, b, _), (xg, wg, bg, _) = _case(O.NORM_N, F, torch.float32)
    y = norm_relu_dropout(xg, wg, bg, 0.5, SEED, True)
    assert y.is_cuda
    O.check_norm_act_fwd(x, w, b, 0.5, SEED, True, y.cpu())
    with pytest.raises(RuntimeError, match='F <= 1024'):
        _fwd(xg, wg, bg, 0.5, SEED, True)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_dispatch_empty_input(dtype):
    x = torch.empty(0, 256, dtype=dtype, device='cuda', requires_grad=True)
    w = torch.ones(256, device='cuda', requires_grad=True)
    b = torch.zeros(256, device='cuda', requires_grad=True)
    y = norm_relu_dropout(x, w, b, 0.5, SEED, True)
    assert y.shape == (0, 256) and y.dtype == dtype
    y.sum().backward()
    assert x.grad.shape == (0, 256)
    assert torch.equal(w.grad, torch.zeros_like(w))
    assert torch.equal(b.grad, torch.zeros_like(b))


def test_dispatch_rejects_bad_inputs():
    _, (xg, wg, bg, _) = _case(O.NORM_N, 256, torch.float32)
    with pytest.raises(RuntimeError, match='x must be contiguous'):
        norm_relu_dropout(xg[:, ::2], wg[:128], bg[:128], 0.5, SEED, True)
    with pytest.raises(RuntimeError, match='weight must be fp32'):
        norm_relu_dropout(xg, wg.bfloat16(), bg, 0.5, SEED, True)
    with pytest.raises(ValueError):
        norm_relu_dropout(xg, wg, bg, 1.0, SEED, True)


def test_autocast_bf16():
    (x, w, b, dy), (xg, wg, bg, dyg) = _case(O.NORM_N, 256, torch.bfloat16)
    xg = xg.clone().requires_grad_(True)
    wp = torch.nn.Parameter(wg.clone())
    bp = torch.nn.Parameter(bg.clone())
    with torch.autocast('cuda', dtype=torch.bfloat16):
        y = norm_relu_dropout(xg, wp, bp, 0.5, SEED, True)
    assert y.dtype == torch.bfloat16
    y.backward(dyg)
    assert wp.grad.dtype == torch.float32 and bp.grad.dtype == torch.float32
    assert xg.grad.dtype == torch.bfloat16
    O.check_norm_act_fwd(x, w, b, 0.5, SEED, True, y.detach().cpu())
    O.check_norm_act_bwd(x, w, b, 0.5, SEED, True, dy, xg.grad.cpu(),
                         wp.grad.cpu(), bp.grad.cpu())


def test_model_wiring_gpu():
    """One train epoch of a fused DistSAGE in fp32 and under a bf16 engine
    on the tiny world-1 graph: norms[0]'s output passes the forward
    checker for the seed it used, and every norms.* grad is finite and
    non-zero."""
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29787')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import global_train_count, train_epoch
    _native()
    comm = Communicator()
    try:
        g = random_partitioned_graph(2000, 20000, 64, 10, 1, seed=3)
        lg = partition_all(g, 1)[0]
        for cdt in (torch.float32, torch.bfloat16):
            engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                                 msg_dims=[64, 32, 32], device=comm.device)
            engine.compute_dtype = cdt
            engine.set_uniform_assignment(8)
            torch.manual_seed(0)
            model = DistSAGE(64, 32, 10, 3, dropout=0.5,
                             fused_norm=True).to(comm.device)
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            cap = []
            model.norms[0].register_forward_hook(
                lambda m, inp, out: cap.append(
                    (inp[0].detach().cpu(), out.detach().cpu(), m.last_seed,
                     m.weight.detach().cpu().clone(),
                     m.bias.detach().cpu().clone())))
            gc = global_train_count(engine)
            loss = train_epoch(engine, model, opt, gc, multilabel=False)
            torch.cuda.synchronize()
            assert torch.isfinite(loss), (cdt, loss)
            x, y, seed, w, b = cap[0]
            assert x.dtype == cdt and y.dtype == cdt
            O.check_norm_act_fwd(x, w, b, 0.5, seed, True, y)
            for name, prm in model.named_parameters():
                if name.startswith('norms.'):
                    assert prm.grad is not None and prm.grad.dtype == torch.float32
                    assert torch.isfinite(prm.grad).all(), (cdt, name)
                    assert prm.grad.abs().max() > 0, (cdt, name)
    finally:
        Communicator.shutdown()
