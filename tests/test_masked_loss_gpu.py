"""Masked-loss HIP kernels against the float64 oracle of loss_oracles.py
(GPU only). Shapes are the smallest that reach each path: every
sub-wavefront width, one, two and three trips of the class loop, the widest
row (C = 1024), partial last blocks and a second trip of the row loop."""
import os

import pytest
import torch

import loss_oracles as O
from adaqp_amd.ops import loss as L
from adaqp_amd.ops import masked_loss, masked_loss_torch
from adaqp_amd.runtime.utils import compute_loss

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['fp32', 'bf16']
KINDS = [False, True]
KIND_IDS = ['ce', 'bce']


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _gpu(case):
    return tuple(t.cuda() for t in case)


def _run(zg, labels, mask, multilabel, g=O.LOSS_G, fn=masked_loss):
    """forward + backward with the upstream gradient as a device scalar"""
    zg = zg.detach().requires_grad_(True)
    loss = fn(zg, labels, mask, multilabel)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    gt = torch.full((), g, dtype=torch.float32, device='cuda')
    loss.backward(gt)
    assert zg.grad.dtype == zg.dtype and zg.grad.is_contiguous()
    return loss.detach(), zg.grad


def _check(case, multilabel, loss, dz):
    z, labels, mask = case
    a = O.check_loss(z, labels, mask, multilabel, loss.cpu())
    b = O.check_grad(z, labels, mask, multilabel, O.LOSS_G, dz.cpu())
    print(f'share of bound: loss {a:.3f} grad {b:.3f}')


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('C', O.LOSS_CS)
def test_within_bounds(C, multilabel, dtype):
    """Random mask at 0.66 with the planted extremes, every N."""
    for N in O.LOSS_NS:
        case = O.loss_case(N, C, multilabel, dtype)
        before = L.calls
        loss, dz = _run(*_gpu(case), multilabel)
        assert L.calls == before + 1
        _check(case, multilabel, loss, dz)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_within_bounds_without_extremes(multilabel, dtype):
    """No planted 1e4 logits: the loss scale, and with it the loss bound,
    is that of ordinary logits, as tight as the bound gets."""
    for C in (47, 107):
        case = O.loss_case(257, C, multilabel, dtype, extremes=False)
        _check(case, multilabel, *_run(*_gpu(case), multilabel))


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('scale', [1.0, 30.0])
def test_within_bounds_other_logit_scales(scale, multilabel):
    for C in (47, 107):
        case = O.loss_case(257, C, multilabel, torch.float32, scale=scale)
        _check(case, multilabel, *_run(*_gpu(case), multilabel))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_row_loop_second_trip(multilabel, dtype):
    C = 65
    max_blocks, rows = L.launch_geometry(C)
    N = max_blocks * rows + 1
    assert N > max_blocks * rows         # some block must make a second trip
    case = O.loss_case(N, C, multilabel, dtype)
    _check(case, multilabel, *_run(*_gpu(case), multilabel))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('density', [0.0, 1.0])
def test_uniform_masks(density, multilabel, dtype):
    """All false: loss +0.0, every dz bit zero, and the garbage labels and
    NaN/inf logits of the unmasked rows reach nothing. All true: in bounds."""
    for C in (47, 107):
        case = O.loss_case(257, C, multilabel, dtype, density=density)
        loss, dz = _run(*_gpu(case), multilabel)
        _check(case, multilabel, loss, dz)
        if density == 0.0:
            assert not _bits(loss).any() and not _bits(dz).any()


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_empty_input(multilabel, dtype):
    z = torch.empty(0, 47, dtype=dtype, device='cuda')
    labels = (torch.empty(0, 47, device='cuda') if multilabel
              else torch.empty(0, dtype=torch.int64, device='cuda'))
    mask = torch.empty(0, dtype=torch.bool, device='cuda')
    loss, dz = _run(z, labels, mask, multilabel)
    assert not _bits(loss).any()
    assert dz.shape == (0, 47) and dz.dtype == dtype


def test_out_of_range_label_in_a_masked_row():
    """NaN loss, no fault, finite gradients, zeros in unmasked rows."""
    z, labels, mask = O.loss_case(257, 47, False, torch.float32)
    labels = labels.clone()
    rows = torch.nonzero(mask).flatten()
    labels[rows[5]] = 47
    labels[rows[6]] = -1
    labels[rows[7]] = 2 ** 40
    loss, dz = _run(z.cuda(), labels.cuda(), mask.cuda(), False)
    assert torch.isnan(loss)
    assert torch.isfinite(dz[mask.cuda()]).all()
    assert not _bits(dz[~mask.cuda()]).any()


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_input_layouts(multilabel, dtype):
    """A view with a storage offset (row base 2 or 4 bytes off any wider
    alignment) and a non-contiguous column slice give the contiguous
    copy's bits."""
    case = O.loss_case(257, 47, multilabel, dtype)
    z, labels, mask = _gpu(case)
    loss0, dz0 = _run(z, labels, mask, multilabel)
    flat = torch.zeros(z.numel() + 1, dtype=dtype, device='cuda')
    flat[1:] = z.flatten()
    off = flat[1:].view_as(z)
    assert off.storage_offset() == 1 and off.is_contiguous()
    wide = torch.zeros(257, 2 * 47, dtype=dtype, device='cuda')
    wide[:, ::2] = z
    sl = wide[:, ::2]
    assert not sl.is_contiguous()
    for view in (off, sl):
        loss, dz = _run(view, labels, mask, multilabel)
        assert torch.equal(_bits(loss), _bits(loss0))
        assert torch.equal(_bits(dz), _bits(dz0))
    _check(case, multilabel, loss, dz)


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('C', [47, 107, 1024])
def test_bf16_is_the_fp32_result_rounded_once(C, multilabel):
    z, labels, mask = _gpu(O.loss_case(257, C, multilabel, torch.bfloat16))
    loss_b, dz_b = _run(z, labels, mask, multilabel)
    loss_f, dz_f = _run(z.float(), labels, mask, multilabel)
    assert torch.equal(_bits(loss_b), _bits(loss_f))
    assert torch.equal(_bits(dz_b), _bits(dz_f.to(torch.bfloat16)))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_bit_reproducible(multilabel, dtype):
    z, labels, mask = _gpu(O.loss_case(4101, 107, multilabel, dtype))
    a = _run(z, labels, mask, multilabel)
    b = _run(z, labels, mask, multilabel)
    for t0, t1 in zip(a, b):
        assert torch.equal(_bits(t0), _bits(t1))


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_wide_rows_take_the_torch_path(multilabel):
    C = O.LOSS_C_TORCH
    assert C > L.MAX_CLASSES
    case = O.loss_case(65, C, multilabel, torch.float32)
    z, labels, mask = _gpu(case)
    loss, dz = _run(z, labels, mask, multilabel)
    _check(case, multilabel, loss, dz)
    ref, dref = _run(z, labels, mask, multilabel, fn=masked_loss_torch)
    assert torch.equal(loss, ref) and torch.equal(dz, dref)
    from adaqp_amd.ops.kernels import native
    lab = labels if multilabel else labels.clamp(0, C - 1)
    with pytest.raises(RuntimeError, match='C <= 1024'):
        native().masked_loss_fwd(z, lab, mask, multilabel)


def test_rejects_bad_inputs():
    z, labels, mask = _gpu(O.loss_case(65, 47, False, torch.float32))
    from adaqp_amd.ops.kernels import native
    with pytest.raises(RuntimeError, match='contiguous'):
        native().masked_loss_fwd(z[:, ::2], labels, mask, False)
    with pytest.raises(RuntimeError, match='int64'):
        native().masked_loss_fwd(z, labels.int(), mask, False)
    with pytest.raises(RuntimeError, match='mask'):
        native().masked_loss_fwd(z, labels, mask.cpu(), False)
    with pytest.raises(ValueError):
        masked_loss(z, labels, mask[:-1], False)


@pytest.mark.parametrize('multilabel', KINDS, ids=KIND_IDS)
def test_no_host_sync(multilabel):
    """The fused forward + backward completes with host syncs forbidden;
    the unfused chain (boolean indexing) raises there."""
    if not hasattr(torch.cuda, 'set_sync_debug_mode'):
        pytest.skip('this torch build has no cuda sync debug mode')
    case = O.loss_case(257, 47, multilabel, torch.float32, extremes=False)
    z, labels, mask = _gpu(case)
    gc = torch.full((1,), 64.0, device='cuda')
    gt = torch.full((), O.LOSS_G, dtype=torch.float32, device='cuda')
    zg = z.clone().requires_grad_(True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = compute_loss(zg, labels, mask, multilabel, gc, fused=True)
        loss.backward(gt.reshape(1))
        with pytest.raises(RuntimeError):
            compute_loss(z, labels, mask, multilabel, gc, fused=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    O.check_loss(*case, multilabel, (loss.detach() * 64.0).reshape(()).cpu())
    O.check_grad(*case, multilabel, O.LOSS_G / 64.0, zg.grad.cpu())


# ---------------------------------------------------------------------------
# one-rank train_epoch
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world1():
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29788')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.ops.kernels import native
    native()
    comm = Communicator()
    try:
        yield comm
    finally:
        Communicator.shutdown()


@pytest.mark.parametrize('cdt', DTYPES, ids=DT_IDS)
def test_train_epoch(world1, cdt, monkeypatch):
    from adaqp_amd.graph import partition_all, random_partitioned_graph
    from adaqp_amd.helpers import DistGNNType, RunMode
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import global_train_count, train_epoch
    monkeypatch.delenv('ADAQP_FUSED_LOSS', raising=False)
    g = random_partitioned_graph(300, 3000, 16, 7, 1, seed=5,
                                 teacher_labels=True)
    lg = partition_all(g, 1)[0]

    def run(epochs, fused):
        engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                             msg_dims=[16, 16, 16], device=world1.device)
        engine.compute_dtype = cdt
        engine.set_uniform_assignment(8)
        torch.manual_seed(0)
        model = DistSAGE(16, 16, 7, 3, dropout=0.0).to(world1.device)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        cap = []
        model.register_forward_hook(
            lambda m, inp, out: cap.append(out.detach().clone()))
        gc = global_train_count(engine)
        before = L.calls
        losses = [train_epoch(engine, model, opt, gc, False, fused_loss=fused)
                  for _ in range(epochs)]
        torch.cuda.synchronize()
        return cap[0], losses, L.calls - before, engine, float(gc)

    z_on, l_on, n_on, engine, gc = run(10, True)
    z_off, l_off, n_off, _, _ = run(1, False)
    assert n_on == 10 and n_off == 0         # once per epoch, never when off
    assert z_on.dtype == z_off.dtype
    assert torch.equal(_bits(z_on), _bits(z_off))
    if cdt == torch.float32:
        assert z_on.dtype == torch.float32
    labels = engine.graph.labels.cpu()
    mask = engine.graph.train_mask.cpu()
    zc = z_on.cpu()
    assert zc.dtype in (torch.float32, torch.bfloat16)
    # the division by the train count is one more rounding: u * |L|
    for loss in (l_on[0], l_off[0]):
        raw = loss.double().reshape(()).cpu() * gc
        O.check_loss(zc, labels, mask, False, raw,
                     extra=O.U32 * abs(float(raw)))
    vals = [float(v) for v in l_on]
    assert all(v == v and abs(v) != float('inf') for v in vals), vals
    assert vals[-1] < vals[0], vals
