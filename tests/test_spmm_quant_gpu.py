"""SpMM gathering remote columns straight from the quantized wire buffer
(``QuantRemote``, csrc/spmm_quant.hip). It must equal the dense kernel fed
``mixed_dequantize``'s block on the same wire bytes bit for bit, and pass the
float64 oracle's counted bound with that block as the remote operand."""
import functools
import itertools

import pytest
import torch

import kernel_oracles as K

pytestmark = pytest.mark.gpu

# VE/SW per F: 256 4/64, 136 4/64, 104 4/32 (26-byte rows at 2 bits),
# 602 2/64 (5 chunks), 17 1/32 (odd row starts, pad bits), 6 2/16
FEATS = (256, 136, 104, 602, 17, 6)
PEERS = (70, 0, 50)
SEED = 77


def _i32(t):
    return t.contiguous().view(torch.int32)


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
    constant: scale 0) quantized at random bits for three peers, received
    into a permutation of the 120 remote rows."""
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
    assert recv.row_tab.shape == (K.SR_NR, 4) and (recv.row_tab[:, 2] > 0).all()
    payload, params = mixed_quantize(x.cuda(), send, SEED)
    assert (params[0::2] == 0).any()          # the constant row's scale
    return payload, params, recv


@pytest.mark.parametrize('F', FEATS)
def test_quant_gather_equals_dequantize_then_dense(F):
    from adaqp_amd.ops.kernels import QuantRemote, mixed_dequantize, spmm
    indptr, indices, src, dst = K.split_rows_graph()
    view = _view()
    payload, params, recv = _wire(F)
    xl = K.split_rows_x(F, torch.float32)[:K.SR_NL].cuda()
    xr = mixed_dequantize(payload, params, recv,
                          torch.full((K.SR_NR, F), float('nan'), device='cuda'))
    assert not torch.isnan(xr).any()
    qr = QuantRemote(payload, params, recv, F)
    assert qr.fusable(xl) and qr.rows == K.SR_NR
    x_all = torch.cat([xl, xr]).cpu()
    addend = torch.randn(K.SR_R, F, generator=torch.Generator().manual_seed(3)).cuda()
    segs = K.segs_per_row(view)
    for ss, ds in itertools.product([False, True], repeat=2):
        s, d = (src if ss else None), (dst if ds else None)
        kw = dict(src_scale=s.cuda() if ss else None,
                  dst_scale=d.cuda() if ds else None)
        plain = None
        for ad in (False, True):
            a = addend if ad else None
            dense = spmm(view, xl, xr, addend=a, **kw)
            out = torch.full((K.SR_R, F), float('nan'), device='cuda')
            got = spmm(view, xl, qr, addend=a, out=out, **kw)
            assert got.data_ptr() == out.data_ptr()
            assert torch.equal(_i32(got), _i32(dense)), (F, ss, ds, ad)
            if not ad:
                K.check_spmm(indptr, indices, x_all, s, d, got.cpu(), segs)
                plain = got
            else:   # the oracle's bound through round_add's rule
                assert torch.equal(got, plain + addend), (F, ss, ds)


def test_bf16_local_takes_the_dequantize_path():
    from adaqp_amd.ops.kernels import QuantRemote, mixed_dequantize, spmm
    F = 136
    _, _, src, dst = K.split_rows_graph()
    payload, params, recv = _wire(F)
    xl = K.split_rows_x(F, torch.bfloat16)[:K.SR_NL].cuda()
    xr = mixed_dequantize(payload, params, recv,
                          torch.zeros(K.SR_NR, F, dtype=torch.bfloat16, device='cuda'))
    qr = QuantRemote(payload, params, recv, F)
    assert not qr.fusable(xl)
    dense = spmm(_view(), xl, xr, src.cuda(), dst.cuda())
    got = spmm(_view(), xl, qr, src.cuda(), dst.cuda())
    assert got.dtype == torch.bfloat16 and torch.equal(got, dense)
    assert qr._desc is None                   # no descriptors were built
