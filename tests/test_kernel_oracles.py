"""CPU tests of the float64 checkers in kernel_oracles.py: they must accept
the project's own CPU paths at the shapes the GPU tests use, and reject
realistic kernel bugs, so that a green GPU run means something."""
import pytest
import torch

import kernel_oracles as O
from adaqp_amd.ops import quant as Q
from adaqp_amd.ops.kernels import (SEG_EDGES, SpmmView, spmm, mixed_quantize,
                                   mixed_dequantize)
from adaqp_amd.comm.buffers import BITS_SET

DTYPES = [torch.float32, torch.bfloat16]


# --------------------------------------------------------------------------
# accept: the CPU reference paths
# --------------------------------------------------------------------------

@pytest.mark.parametrize('seed', O.PACK_SEEDS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F', O.PACK_FS)
@pytest.mark.parametrize('bits', [2, 4, 8])
def test_accepts_pack_torch(bits, F, dtype, seed):
    c = O.PackCase(F, bits, dtype)
    pl, scale, rmin = Q.pack_torch(c.x_rows, bits, seed, node_tag=c.pos)
    O.check_packed(c.x_rows, bits, seed, c.pos, pl, scale, rmin)
    assert float(scale[O.CONST_NODE]) == 0.0
    if F > 1 and dtype == torch.float32:
        i = O.INEXACT_NODE
        assert float(rmin[i]) != float(c.x_rows[i].min())


def test_seed_is_taken_mod_2_32():
    c = O.PackCase(100, 4)
    a = Q.pack_torch(c.x_rows, 4, 2 ** 32 + 5, node_tag=c.pos)[0]
    b = Q.pack_torch(c.x_rows, 4, 5, node_tag=c.pos)[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('F', [17, 602, 1030])
@pytest.mark.parametrize('bits', [2, 4, 8])
def test_accepts_unpack_torch(bits, F, dtype):
    c = O.PackCase(F, bits)
    pl, scale, rmin = Q.pack_torch(c.x_rows, bits, 1234, node_tag=c.pos)
    out = Q.unpack_torch(pl, bits, scale, rmin, F).to(dtype)
    O.check_unpacked(pl, bits, scale, rmin, F, out)


@pytest.mark.parametrize('F', [100, 1030])
def test_accepts_mixed_cpu(F):
    x, send, recv, n_out = O.mixed_plans(F)
    assert send.node_splits[1] == 0 and send.total_nodes > 55
    payload, params = mixed_quantize(x, send, 77)
    for b in BITS_SET:
        assert send.rows[b].numel() > 0
        pos = send.pos[b]
        O.check_packed(x[send.rows[b]], b, 77, pos, O.plan_payload(payload, send, b),
                       params[2 * pos], params[2 * pos + 1])
    out = torch.full((n_out, F), -3.0)
    mixed_dequantize(payload, params, recv, out)
    touched = torch.zeros(n_out, dtype=torch.bool)
    for b in BITS_SET:
        pos = recv.pos[b]
        O.check_unpacked(O.plan_payload(payload, recv, b), b, params[2 * pos],
                         params[2 * pos + 1], F, out[recv.rows[b]])
        touched[recv.rows[b]] = True
    assert (~touched).sum() == 9 and (out[~touched] == -3.0).all()


def _cpu_spmm(indptr, indices, x, nl, src, dst):
    """CPU spmm through the dual-tensor interface; bf16 is computed as fp32
    and rounded once."""
    view = SpmmView(indptr, indices, 0, indptr.numel() - 1)
    xf = x.float()
    y = spmm(view, xf[:nl].contiguous(), xf[nl:].contiguous(), src, dst)
    return y.to(x.dtype), O.segs_per_row(view)


@pytest.mark.parametrize('dtype,F', [(torch.float32, 132), (torch.bfloat16, 264)])
def test_accepts_cpu_spmm_grid_stride(dtype, F):
    indptr, indices, src, dst = O.grid_stride_graph()
    x = O.grid_stride_x(F, dtype)
    y, segs = _cpu_spmm(indptr, indices, x, O.GS_NL, src, dst)
    assert int(segs.sum()) > 65536
    assert int(segs[10]) == 4 and int(segs[65900]) == 2
    O.check_spmm(indptr, indices, x, src, dst, y, segs)


@pytest.mark.parametrize('dtype,F', O.SR_CASES)
def test_accepts_cpu_spmm_split_rows(dtype, F):
    indptr, indices, src, dst = O.split_rows_graph()
    x = O.split_rows_x(F, dtype)
    y, segs = _cpu_spmm(indptr, indices, x, O.SR_NL, src, dst)
    O.check_spmm(indptr, indices, x, src, dst, y, segs)


def test_spmm_reference_counts_duplicate_edges():
    indptr = torch.tensor([0, 3, 3, 4])
    indices = torch.tensor([1, 1, 0, 1])
    x = torch.tensor([[1.0, 2.0], [10.0, 20.0]])
    ref, S, deg = O.spmm_reference(indptr, indices, x, None, None)
    assert ref.tolist() == [[21.0, 42.0], [0.0, 0.0], [10.0, 20.0]]
    assert deg.tolist() == [3, 0, 1]
    O.check_spmm(indptr, indices, x, None, None, ref.float())


def _gemm_ref32(a1, a2, w1, w2, bias):
    r = a1.float() @ w1.float() + a2.float() @ w2.float()
    return r + bias.float() if bias is not None else r


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('shape', O.GEMM_SHAPES)
def test_accepts_fp32_dual_gemm(shape, with_bias):
    a1, a2, w1, w2, bias = O.gemm_case(*shape)
    bias = bias if with_bias else None
    O.check_dual_gemm(a1, a2, w1, w2, bias,
                      _gemm_ref32(a1, a2, w1, w2, bias).bfloat16())


# --------------------------------------------------------------------------
# reject: realistic kernel bugs
# --------------------------------------------------------------------------

def _pack_base(bits, F=2051):
    c = O.PackCase(F, bits)
    pl, scale, rmin = Q.pack_torch(c.x_rows, bits, 1234, node_tag=c.pos)
    q64, lo, hi, _ = O.packed_reference(c.x_rows, bits, 1234, c.pos)
    lv = O.unpack_levels(pl, bits)
    lv[:, :F] = q64                      # start from the oracle's own levels
    return c, lv, scale.clone(), rmin.clone(), q64, lo, hi


def _mut_tail_flip(bits=4):
    c, lv, s, r, *_ = _pack_base(bits)
    lv[6, c.F - 1] ^= 2 ** bits - 1
    return c, bits, O.pack_levels(lv, bits), s, r


def _mut_off1_interior(bits=8):
    c, lv, s, r, q64, lo, hi = _pack_base(bits)
    ok = (lo == hi) & (q64 >= 1) & (q64 < 2 ** bits - 1)
    i, f = torch.nonzero(ok)[100].tolist()
    lv[i, f] += 1
    return c, bits, O.pack_levels(lv, bits), s, r


def _mut_off2_boundary(bits=8):
    c, lv, s, r, q64, lo, hi = _pack_base(bits)
    up = (hi > q64) & (q64 + 2 <= 2 ** bits - 1)     # oracle below the boundary
    dn = (lo < q64) & (q64 - 2 >= 0)                 # oracle above it
    assert up.any() and dn.any(), 'case has no value within delta of a boundary'
    i, f = torch.nonzero(up)[0].tolist()
    lv[i, f] = q64[i, f] + 2
    return c, bits, O.pack_levels(lv, bits), s, r


def _mut_off2_boundary_down(bits=8):
    c, lv, s, r, q64, lo, hi = _pack_base(bits)
    dn = (lo < q64) & (q64 - 2 >= 0)
    i, f = torch.nonzero(dn)[0].tolist()
    lv[i, f] = q64[i, f] - 2
    return c, bits, O.pack_levels(lv, bits), s, r


def _mut_off1_wrong_side(bits=8):
    """at a boundary only the level on the boundary's side is admissible"""
    c, lv, s, r, q64, lo, hi = _pack_base(bits)
    up = (hi > q64) & (q64 >= 1)
    i, f = torch.nonzero(up)[0].tolist()
    lv[i, f] = q64[i, f] - 1
    return c, bits, O.pack_levels(lv, bits), s, r


def _mut_pad_bit(bits=4):
    c, lv, s, r, *_ = _pack_base(bits)
    pl = O.pack_levels(lv, bits)
    pl[9, -1] |= 0x80
    return c, bits, pl, s, r


def _mut_swap_nodes(bits=4):
    c, lv, s, r, *_ = _pack_base(bits)
    pl = O.pack_levels(lv, bits)
    pl[[0, 1]] = pl[[1, 0]]
    return c, bits, pl, s, r


def _mut_tag_wid(bits=4):
    c = O.PackCase(2051, bits)
    assert not torch.equal(c.pos, torch.arange(c.n))
    pl, s, r = Q.pack_torch(c.x_rows, bits, 1234, node_tag=torch.arange(c.n))
    return c, bits, pl, s, r


def _mut_scale_lsb(bits=4):
    c, lv, s, r, *_ = _pack_base(bits)
    s.view(torch.int16)[7] ^= 1
    return c, bits, O.pack_levels(lv, bits), s, r


PACK_MUTATIONS = [_mut_tail_flip, _mut_off1_interior, _mut_off2_boundary,
                  _mut_off2_boundary_down, _mut_off1_wrong_side, _mut_pad_bit,
                  _mut_swap_nodes, _mut_tag_wid, _mut_scale_lsb]


@pytest.mark.parametrize('bits', [4, 8])
def test_oracle_levels_accepted(bits):
    c, lv, s, r, *_ = _pack_base(bits)
    O.check_packed(c.x_rows, bits, 1234, c.pos, O.pack_levels(lv, bits), s, r)


@pytest.mark.parametrize('mut', PACK_MUTATIONS, ids=lambda m: m.__name__[5:])
def test_rejects_pack_bug(mut):
    c, bits, pl, s, r = mut()
    with pytest.raises(AssertionError):
        O.check_packed(c.x_rows, bits, 1234, c.pos, pl, s, r)


def test_boundary_positions_are_rare_and_off_by_one():
    """fp32 pack_torch vs the float64 oracle: every difference lies within
    delta of a boundary and is exactly one level."""
    n_elig = n_diff = total = 0
    for bits in (2, 4, 8):
        c = O.PackCase(2051, bits)
        pl = Q.pack_torch(c.x_rows, bits, 1234, node_tag=c.pos)[0]
        q = O.unpack_levels(pl, bits)[:, :c.F]
        q64, lo, hi, _ = O.packed_reference(c.x_rows, bits, 1234, c.pos)
        diff = q != q64
        assert (lo != hi)[diff].all() and ((q - q64).abs()[diff] == 1).all()
        n_elig += int((lo != hi).sum()); n_diff += int(diff.sum())
        total += q.numel()
    assert n_elig < 5e-4 * total, (n_elig, total)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('bug', ['off_by_step', 'wrong_row'])
def test_rejects_unpack_bug(bug, dtype):
    bits, F = 8, 602
    c = O.PackCase(F, bits)
    pl, scale, rmin = Q.pack_torch(c.x_rows, bits, 1234, node_tag=c.pos)
    out = Q.unpack_torch(pl, bits, scale, rmin, F)
    O.check_unpacked(pl, bits, scale, rmin, F, out.to(dtype))
    if bug == 'off_by_step':
        out[4, 9] += 1.0 / scale.float()[4]
    else:
        out[[0, 1]] = out[[1, 0]]
    with pytest.raises(AssertionError):
        O.check_unpacked(pl, bits, scale, rmin, F, out.to(dtype))


def _spmm64(row_of_edge, cols, x64, src, dst, R, col_read=None):
    """float64 SpMM from an explicit edge list, so edges can be dropped or
    redirected (col_read: the x row each edge actually reads)."""
    rd = cols if col_read is None else col_read
    contrib = x64[rd] * src.double()[cols, None]
    y = torch.zeros(R, x64.shape[1], dtype=torch.float64)
    y.index_add_(0, row_of_edge, contrib)
    return y * dst.double()[:, None]


def _trunc_bf16(y32):
    return (y32.contiguous().view(torch.int32) & -65536).view(torch.float32) \
        .bfloat16()


SPMM_BUGS = ['edge_dropped', 'hub_partial_dropped', 'dst_twice',
             'remote_read_local', 'bf16_truncated']


@pytest.mark.parametrize('bug', SPMM_BUGS)
def test_rejects_spmm_bug(bug):
    indptr, indices, src, dst = O.split_rows_graph()
    R, F = O.SR_R, 136
    dtype = torch.bfloat16 if bug == 'bf16_truncated' else torch.float32
    x = O.split_rows_x(F, dtype)
    x64 = x.double()
    deg = indptr[1:] - indptr[:-1]
    roe = torch.repeat_interleave(torch.arange(R), deg)
    segs = O.segs_per_row(SpmmView(indptr, indices, 0, R))
    good = _spmm64(roe, indices, x64, src, dst, R)
    O.check_spmm(indptr, indices, x, src, dst, good.to(dtype), segs)
    keep = torch.ones(indices.numel(), dtype=torch.bool)
    if bug == 'edge_dropped':
        keep[indptr[7]] = False
        y = _spmm64(roe[keep], indices[keep], x64, src, dst, R).float()
    elif bug == 'hub_partial_dropped':
        keep[indptr[0] + SEG_EDGES:indptr[0] + 2 * SEG_EDGES] = False
        y = _spmm64(roe[keep], indices[keep], x64, src, dst, R).float()
    elif bug == 'dst_twice':
        y = good.clone()
        y[0] *= dst.double()[0]
        y = y.float()
    elif bug == 'remote_read_local':
        e = int(torch.nonzero((indices >= O.SR_NL) & (roe == 0))[0])
        rd = indices.clone()
        rd[e] -= O.SR_NL
        y = _spmm64(roe, indices, x64, src, dst, R, col_read=rd).float()
    else:
        y = _trunc_bf16(good.float())
    with pytest.raises(AssertionError):
        O.check_spmm(indptr, indices, x, src, dst, y, segs)


def test_rejects_spmm_row_left_at_sentinel():
    """a row only reached in the second grid-stride trip keeps its fill"""
    indptr, indices, src, dst = O.grid_stride_graph()
    x = O.grid_stride_x(132, torch.float32)
    ref, _, deg = O.spmm_reference(indptr, indices, x, src, dst)
    y = ref.float()
    O.check_spmm(indptr, indices, x, src, dst, y)
    r = 65990                      # beyond the 65 536 segments of trip one
    assert deg[r] > 0
    y[r] = -3.0
    with pytest.raises(AssertionError, match=r'y\[65990, 0\]'):
        O.check_spmm(indptr, indices, x, src, dst, y)


@pytest.mark.parametrize('bug', ['tile_transposed', 'last_k_chunk_dropped'])
def test_rejects_dual_gemm_bug(bug):
    a1, a2, w1, w2, bias = O.gemm_case(77, 40, 72, 16)
    out = _gemm_ref32(a1, a2, w1, w2, bias).bfloat16()
    if bug == 'tile_transposed':
        out[16:32, 0:16] = out[16:32, 0:16].t().clone()
    else:
        out = _gemm_ref32(a1, a2[:, :64], w1, w2[:64], bias).bfloat16()
    with pytest.raises(AssertionError):
        O.check_dual_gemm(a1, a2, w1, w2, bias, out)
