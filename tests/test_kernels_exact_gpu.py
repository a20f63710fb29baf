"""HIP kernels vs the float64 oracles of kernel_oracles.py (GPU only).

Shapes are the smallest that reach each code path: the unstaged pack
branch (F > 1024), the SpMM grid-stride loop (> 65 536 segments), split
rows with scales and a remote block, ``out=`` row slices, zero-row views
and K values that end the dual GEMM's pipeline on an odd 32-wide chunk.
"""
import pytest
import torch

import kernel_oracles as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _native():
    from adaqp_amd.ops.kernels import native
    return native()


def _plan_to(plan, device):
    import copy
    return copy.copy(plan).to(device)


# --------------------------------------------------------------------------
# quant_pack / quant_unpack
# --------------------------------------------------------------------------

def _gpu_pack(c, seed):
    C = _native()
    payload = torch.full((c.payload_len,), O.PAYLOAD_FILL, dtype=torch.uint8,
                         device='cuda')
    params = torch.full((2 * c.n_slots,), O.PARAMS_FILL, dtype=torch.bfloat16,
                        device='cuda')
    C.quant_pack(c.x.cuda(), c.rows.cuda(), c.pos.cuda(), c.off.cuda(),
                 c.bits, seed, payload, params)
    return payload.cpu(), params.cpu()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F', O.PACK_FS)
@pytest.mark.parametrize('bits', [2, 4, 8])
def test_quant_pack_exact(bits, F, dtype):
    """Every level equals the float64 oracle except within delta of a
    rounding boundary; params are bit-exact; nothing else is written.
    F > 1024 takes the unstaged two-pass branch."""
    c = O.PackCase(F, bits, dtype)
    by_seed = {}
    for seed in O.PACK_SEEDS + (5,):
        payload, params = _gpu_pack(c, seed)
        scale, rmin = c.node_params(params)
        O.check_packed(c.x_rows, bits, seed, c.pos, c.node_payload(payload),
                       scale, rmin)
        c.check_untouched(payload, params)
        by_seed[seed] = payload
    # the launcher keeps the low 32 bits of the seed
    assert torch.equal(by_seed[2 ** 32 + 5], by_seed[5])
    if F > 1:
        assert not torch.equal(by_seed[1234], by_seed[5])


@pytest.mark.parametrize('F', [100, 1030])
def test_mixed_plan_exact(F):
    """Three bit groups share one payload (mixed_quantize through _layout),
    then feed mixed_dequantize through the matching recv-side plan."""
    from adaqp_amd.ops.kernels import mixed_quantize, mixed_dequantize
    from adaqp_amd.comm.buffers import BITS_SET
    _native()
    x, send, recv, n_out = O.mixed_plans(F)
    assert send.node_splits[1] == 0 and send.total_nodes > 55
    seed = 77
    payload_g, params_g = mixed_quantize(x.cuda(), _plan_to(send, 'cuda'), seed)
    payload, params = payload_g.cpu(), params_g.cpu()
    for b in BITS_SET:
        assert send.rows[b].numel() > 0
        pos = send.pos[b]
        O.check_packed(x[send.rows[b]], b, seed, pos,
                       O.plan_payload(payload, send, b),
                       params[2 * pos], params[2 * pos + 1])
    for dtype in DTYPES:
        out_g = torch.full((n_out, F), -3.0, dtype=dtype, device='cuda')
        mixed_dequantize(payload_g, params_g, _plan_to(recv, 'cuda'), out_g)
        out = out_g.cpu()
        touched = torch.zeros(n_out, dtype=torch.bool)
        for b in BITS_SET:
            pos = recv.pos[b]
            O.check_unpacked(O.plan_payload(payload, recv, b), b,
                             params[2 * pos], params[2 * pos + 1], F,
                             out[recv.rows[b]])
            touched[recv.rows[b]] = True
        assert int((~touched).sum()) == 9
        assert (out[~touched].float() == -3.0).all(), 'spare rows written'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F', [17, 602, 1030])
@pytest.mark.parametrize('bits', [2, 4, 8])
def test_quant_unpack_exact(bits, F, dtype):
    """Payload from pack_torch (independent of the pack kernel), scattered
    through a permutation into a larger out."""
    from adaqp_amd.ops import quant as Q
    C = _native()
    c = O.PackCase(F, bits)
    pl, scale, rmin = Q.pack_torch(c.x_rows, bits, 1234, node_tag=c.pos)
    payload = torch.full((c.payload_len,), O.PAYLOAD_FILL, dtype=torch.uint8)
    idx = c.off[:, None] + torch.arange(c.bpn)
    payload[idx.reshape(-1)] = pl.reshape(-1)
    params = torch.full((2 * c.n_slots,), O.PARAMS_FILL, dtype=torch.bfloat16)
    params[2 * c.pos] = scale
    params[2 * c.pos + 1] = rmin
    n_out = c.n + 12
    gen = torch.Generator().manual_seed(5)
    out_rows = torch.randperm(n_out, generator=gen)[:c.n]
    out_g = torch.full((n_out, F), -3.0, dtype=dtype, device='cuda')
    C.quant_unpack(payload.cuda(), params.cuda(), out_rows.cuda(), c.pos.cuda(),
                   c.off.cuda(), bits, F, out_g)
    out = out_g.cpu()
    O.check_unpacked(pl, bits, scale, rmin, F, out[out_rows])
    spare = torch.ones(n_out, dtype=torch.bool)
    spare[out_rows] = False
    assert (out[spare].float() == -3.0).all(), 'rows outside `rows` written'


# --------------------------------------------------------------------------
# spmm_csr
# --------------------------------------------------------------------------

def _gpu_spmm(indptr, indices, x, nl, src, dst, col_block=0, out=None):
    from adaqp_amd.ops.kernels import SpmmView, spmm
    _native()
    R = indptr.numel() - 1
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, R,
                    col_block=col_block).to('cuda')
    xg = x.cuda()
    xr = xg[nl:].contiguous() if nl < x.shape[0] else None
    y = spmm(view, xg[:nl].contiguous(), xr,
             None if src is None else src.cuda(),
             None if dst is None else dst.cuda(), out=out)
    return y, view


@pytest.mark.parametrize('dtype,F,col_block', [(torch.float32, 132, 0),
                                               (torch.float32, 132, 256),
                                               (torch.bfloat16, 264, 0)])
def test_spmm_grid_stride_exact(dtype, F, col_block):
    """More segments than 16384 blocks x 4 sub-wavefronts cover: the
    kernel's grid-stride loop takes a second trip under the XCD swizzle."""
    indptr, indices, src, dst = O.grid_stride_graph()
    x = O.grid_stride_x(F, dtype)
    y, view = _gpu_spmm(indptr, indices, x, O.GS_NL, src, dst, col_block)
    assert view.seg_row.numel() > 65536
    assert y.dtype == dtype
    yc = y.cpu()
    O.check_spmm(indptr, indices, x, src, dst, yc, O.segs_per_row(view))
    assert (yc[65901] == 0).all()


@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype,F', O.SR_CASES)
def test_spmm_split_rows_scaled_remote_exact(dtype, F, col_block):
    """Rows split across segments with src/dst scales and a remote block all
    at once, as GCN forward/backward run them."""
    indptr, indices, src, dst = O.split_rows_graph()
    x = O.split_rows_x(F, dtype)
    y, view = _gpu_spmm(indptr, indices, x, O.SR_NL, src, dst, col_block)
    segs = O.segs_per_row(view)
    assert all(int(segs[r]) > 1 for r in O.SR_HUBS)
    O.check_spmm(indptr, indices, x, src, dst, y.cpu(), segs)


@pytest.mark.parametrize('dtype,F', [(torch.bfloat16, 6), (torch.float32, 17)])
def test_spmm_out_slice_exact(dtype, F):
    """``out=`` a row slice at an odd row offset (decomposed_propagation
    writes y[:C] and y[C:]); rows outside the slice keep their fill."""
    indptr, indices, src, dst = O.split_rows_graph()
    x = O.split_rows_x(F, dtype)
    R = O.SR_R
    big = torch.full((R + 7, F), -3.0, dtype=dtype, device='cuda')
    y, view = _gpu_spmm(indptr, indices, x, O.SR_NL, src, dst, out=big[5:5 + R])
    assert y.data_ptr() == big[5:5 + R].data_ptr()
    bc = big.cpu()
    O.check_spmm(indptr, indices, x, src, dst, bc[5:5 + R], O.segs_per_row(view))
    assert (bc[:5].float() == -3.0).all() and (bc[5 + R:].float() == -3.0).all()


@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype', DTYPES)
def test_spmm_degenerate_views(dtype, col_block):
    """nrows == 0 (a partition without central or marginal nodes) gives an
    empty [0, F] result; a view whose rows are all empty gives zeros."""
    F = 8
    x = torch.randn(5, F, generator=torch.Generator().manual_seed(1)).to(dtype)
    empty_idx = torch.empty(0, dtype=torch.int64)
    y, _ = _gpu_spmm(torch.zeros(1, dtype=torch.int64), empty_idx, x, 5,
                     None, None, col_block)
    torch.cuda.synchronize()
    assert y.shape == (0, F) and y.dtype == dtype
    src, dst = torch.ones(5), torch.ones(4)
    indptr = torch.zeros(5, dtype=torch.int64)
    y, view = _gpu_spmm(indptr, empty_idx, x, 5, src, dst, col_block)
    assert y.shape == (4, F)
    assert (y.cpu().float() == 0).all()
    O.check_spmm(indptr, empty_idx, x, src, dst, y.cpu(), O.segs_per_row(view))


# --------------------------------------------------------------------------
# fused_dual_gemm_bf16
# --------------------------------------------------------------------------

@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('shape', O.GEMM_SHAPES)
def test_fused_dual_gemm_exact(shape, with_bias):
    """K = 72 ends the double-buffered pipeline after three 32-wide chunks,
    K = 40 leaves the second chunk partly empty, K = 136 after five."""
    C = _native()
    M, K1, K2, N = shape
    a1, a2, w1, w2, bias = O.gemm_case(*shape)
    out = torch.full((M, N), -3.0, dtype=torch.bfloat16, device='cuda')
    bias_g = (bias.cuda() if with_bias
              else torch.empty(0, device='cuda', dtype=torch.bfloat16))
    C.fused_dual_gemm_bf16(a1.cuda(), a2.cuda(), w1.t().contiguous().cuda(),
                           w2.t().contiguous().cuda(), bias_g, out)
    O.check_dual_gemm(a1, a2, w1, w2, bias if with_bias else None, out.cpu())


def test_fused_dual_gemm_transpose_exact():
    """One-hot A with asymmetric W: a transposed C write cannot hide."""
    C = _native()
    M, K, N = 32, 32, 32
    a1 = torch.zeros(M, K)
    a1[torch.arange(M), torch.arange(M) % K] = 1.0
    a1 = a1.bfloat16()
    a2 = torch.zeros(M, K).bfloat16()
    w1 = (torch.arange(K)[:, None] * 100.0 + torch.arange(N)[None, :]).bfloat16()
    w2 = torch.zeros(K, N).bfloat16()
    out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
    C.fused_dual_gemm_bf16(a1.cuda(), a2.cuda(), w1.t().contiguous().cuda(),
                           w2.t().contiguous().cuda(),
                           torch.empty(0, device='cuda', dtype=torch.bfloat16),
                           out)
    O.check_dual_gemm(a1, a2, w1, w2, None, out.cpu())
    assert torch.equal(out.cpu(), w1[torch.arange(M) % K])
