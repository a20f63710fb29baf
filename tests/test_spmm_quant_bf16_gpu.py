"""SpMM on bf16 rows gathering remote columns straight from the quantized wire
buffer (``spmm(..., quant_bf16=True)``, csrc/spmm_quant_bf16.hip). For bf16 out
it must equal the dense bf16 kernel, for fp32 out the mixed kernel, each fed
``mixed_dequantize``'s bf16 block on the same wire bytes, bit for bit, and pass
the float64 oracle's counted bound with that block as the remote operand."""
import functools
import itertools

import pytest
import torch

import kernel_oracles as K

pytestmark = pytest.mark.gpu

# VE/SW per F: 256 8/32 (64-bit windows at 8 bits), 136 8/32 (17 lanes), 104
# 8/16 (26-byte rows at 2 bits: rows start at any byte), 20 4/16 (5-byte rows),
# 602 2/64 (five chunks), 6 2/16 (4-bit steps: first bit not byte aligned)
FEATS = (256, 136, 104, 20, 602, 6)
PEERS = (70, 0, 50)
SEED = 77


@functools.lru_cache(maxsize=None)
def _view():
    from adaqp_amd.ops.kernels import SpmmView, native
    native()
    indptr, indices, _, _ = K.split_rows_graph()
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, K.SR_R).to('cuda')
    assert view.n_part > 0 and view.zero_rows.numel() > 0
    return view


@functools.lru_cache(maxsize=None)
def _wire(F):
    """(payload, params, recv plan) on the GPU: 120 source rows (row 3
    constant: scale 0) quantized at random bits for three peers, one of them
    empty, received into a permutation of the 120 remote rows."""
    from adaqp_amd.comm.buffers import _layout
    from adaqp_amd.ops.kernels import mixed_quantize
    gen = torch.Generator().manual_seed(500 + F)
    x = K.quant_input(150, F, gen)
    send_rows = torch.randperm(150, generator=gen)[:K.SR_NR]
    x[send_rows[3]] = 0.75
    recv_rows = torch.randperm(K.SR_NR, generator=gen)
    choices = torch.tensor([2, 4, 8])
    bits, srows, rrows, base = [], [], [], 0
    for k in PEERS:
        bits.append(choices[torch.randint(0, 3, (k,), generator=gen)] if k else None)
        srows.append(send_rows[base:base + k] if k else None)
        rrows.append(recv_rows[base:base + k] if k else None)
        base += k
    send, recv = _layout(bits, srows, F).to('cuda'), _layout(bits, rrows, F).to('cuda')
    assert recv.row_tab.shape == (K.SR_NR, 4)
    assert set(recv.row_tab[:, 2].tolist()) == {2, 4, 8}
    payload, params = mixed_quantize(x.cuda(), send, SEED)
    assert (params[0::2] == 0).any()          # the constant row's scale
    return payload, params, recv


def _operands(F):
    from adaqp_amd.ops.kernels import QuantRemote, mixed_dequantize
    payload, params, recv = _wire(F)
    xl = K.split_rows_x(F, torch.bfloat16)[:K.SR_NL].cuda()
    xr = mixed_dequantize(payload, params, recv, torch.full(
        (K.SR_NR, F), float('nan'), dtype=torch.bfloat16, device='cuda'))
    assert not torch.isnan(xr).any()
    return xl, xr, QuantRemote(payload, params, recv, F)


@pytest.mark.parametrize('F', FEATS)
@pytest.mark.parametrize('out_dtype', [torch.bfloat16, torch.float32])
def test_bf16_quant_gather_equals_dequantize_then_spmm(F, out_dtype):
    from adaqp_amd.ops.kernels import spmm
    indptr, indices, src, dst = K.split_rows_graph()
    view = _view()
    xl, xr, qr = _operands(F)
    assert qr.fusable_bf16(xl) and not qr.fusable(xl) and qr.rows == K.SR_NR
    mixed = out_dtype == torch.float32
    bits = torch.int32 if mixed else torch.int16
    od = {'out_dtype': torch.float32} if mixed else {}
    x_all = torch.cat([xl, xr]).float().cpu()
    addend = torch.randn(K.SR_R, F, generator=torch.Generator().manual_seed(3)
                         ).to(out_dtype).cuda()
    segs = K.segs_per_row(view)
    for ss, ds in itertools.product([False, True], repeat=2):
        s, d = (src if ss else None), (dst if ds else None)
        kw = dict(src_scale=s.cuda() if ss else None,
                  dst_scale=d.cuda() if ds else None, **od)
        for ad in (False, True):
            a = addend if ad else None
            ref = spmm(view, xl, xr, addend=a, **kw)
            out = torch.full((K.SR_R, F), float('nan'), dtype=out_dtype,
                             device='cuda')
            qr._desc = None
            got = spmm(view, xl, qr, addend=a, out=out, quant_bf16=True, **kw)
            assert qr._desc is not None       # the wire was gathered
            assert got.data_ptr() == out.data_ptr() and got.dtype == out_dtype
            assert torch.equal(got.view(bits), ref.view(bits)), (F, ss, ds, ad)
            if not ad:
                K.check_spmm(indptr, indices, x_all, s, d, got.cpu(), segs)


@pytest.mark.parametrize('out_dtype', [None, torch.float32])
def test_keyword_left_at_its_default_still_dequantizes(out_dtype):
    from adaqp_amd.ops.kernels import spmm
    _, _, src, dst = K.split_rows_graph()
    xl, xr, qr = _operands(136)
    dense = spmm(_view(), xl, xr, src.cuda(), dst.cuda(), out_dtype=out_dtype)
    got = spmm(_view(), xl, qr, src.cuda(), dst.cuda(), out_dtype=out_dtype)
    assert torch.equal(got, dense)
    assert qr._desc is None                   # no descriptors were built
