"""HIP kernel numerics vs plain PyTorch fp32 references (GPU only)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _native():
    from adaqp_amd.ops.kernels import native
    return native()


@pytest.mark.parametrize('bits', [2, 4, 8])
@pytest.mark.parametrize('F', [100, 256, 602])
def test_quant_pack_matches_cpu_oracle(bits, F):
    """GPU pack must agree with the CPU torch oracle (same hash RNG)."""
    from adaqp_amd.ops import quant as Q
    from adaqp_amd.comm.buffers import bytes_per_node
    C = _native()
    torch.manual_seed(0)
    n, N = 37, 80
    x = torch.randn(N, F)
    rows = torch.randperm(N)[:n].to(torch.int64)
    pos = torch.arange(n, dtype=torch.int64)
    bpn = bytes_per_node(F, bits)
    off = pos * bpn
    seed = 1234

    xg = x.cuda()
    payload = torch.zeros(n * bpn, dtype=torch.uint8, device='cuda')
    params = torch.zeros(2 * n, dtype=torch.bfloat16, device='cuda')
    C.quant_pack(xg, rows.cuda(), pos.cuda(), off.cuda(), bits, seed,
                 payload, params)

    pl_cpu, scale, rmin = Q.pack_torch(x[rows], bits, seed, node_tag=pos)
    params_cpu = torch.zeros(2 * n, dtype=torch.bfloat16)
    params_cpu[0::2] = scale
    params_cpu[1::2] = rmin
    assert torch.equal(params.cpu(), params_cpu)
    g = payload.cpu().view(n, bpn)
    # every level equals the float64 oracle; only values within delta of a
    # rounding boundary (where fp contraction may land on the other side)
    # may be off, by exactly one level
    from kernel_oracles import check_packed
    check_packed(x[rows], bits, seed, pos, g, params.cpu()[0::2],
                 params.cpu()[1::2])


@pytest.mark.parametrize('bits', [2, 4, 8])
def test_quant_roundtrip_gpu(bits):
    from adaqp_amd.comm.buffers import bytes_per_node
    C = _native()
    torch.manual_seed(1)
    n, F = 64, 256
    x = torch.randn(n, F, device='cuda')
    rows = torch.arange(n, dtype=torch.int64, device='cuda')
    pos = rows.clone()
    bpn = bytes_per_node(F, bits)
    off = pos * bpn
    payload = torch.zeros(n * bpn, dtype=torch.uint8, device='cuda')
    params = torch.zeros(2 * n, dtype=torch.bfloat16, device='cuda')
    C.quant_pack(x, rows, pos, off, bits, 7, payload, params)
    out = torch.zeros(n, F, device='cuda')
    C.quant_unpack(payload, params, rows, pos, off, bits, F, out)
    rng = x.max(1).values - x.min(1).values
    step = rng / (2 ** bits - 1)
    err = (out - x).abs().max(1).values
    assert (err <= step * 1.05 + rng * 0.01).all()


def test_quant_unbiased_gpu():
    from adaqp_amd.comm.buffers import bytes_per_node
    C = _native()
    torch.manual_seed(2)
    n, F, bits = 16, 64, 2
    x = torch.randn(n, F, device='cuda')
    rows = torch.arange(n, dtype=torch.int64, device='cuda')
    bpn = bytes_per_node(F, bits)
    off = rows * bpn
    acc = torch.zeros_like(x)
    K = 300
    payload = torch.zeros(n * bpn, dtype=torch.uint8, device='cuda')
    params = torch.zeros(2 * n, dtype=torch.bfloat16, device='cuda')
    out = torch.zeros(n, F, device='cuda')
    for s in range(K):
        C.quant_pack(x, rows, rows, off, bits, s * 9973 + 5, payload, params)
        C.quant_unpack(payload, params, rows, rows, off, bits, F, out)
        acc += out
    mean = acc / K
    rng = (x.max(1).values - x.min(1).values)[:, None]
    step = rng / (2 ** bits - 1)
    tol = step * (4.0 / K ** 0.5) + rng * 0.01 + 1e-3
    assert ((mean - x).abs() <= tol).all()


@pytest.mark.parametrize('F', [64, 100, 256, 602, 17])
def test_spmm_matches_torch(F):
    from adaqp_amd.graph import random_partitioned_graph, partition_all
    from adaqp_amd.ops.kernels import SpmmView, spmm
    _native()
    torch.manual_seed(3)
    g = random_partitioned_graph(500, 4000, 4, 3, 1, seed=9)
    lg = partition_all(g, 1)[0]
    x = torch.randn(lg.num_nodes, F, device='cuda')
    src = torch.rand(lg.num_nodes, device='cuda') + 0.5
    dst = torch.rand(lg.num_inner, device='cuda') + 0.5
    # exercise the dual-tensor path: split x arbitrarily at num_inner
    xl = x[:lg.num_inner].contiguous()
    xr = x[lg.num_inner:].contiguous()
    view = SpmmView(lg.indptr.cuda(), lg.indices.cuda(), 0, lg.num_inner).to('cuda')
    y = spmm(view, xl, xr, src, dst)
    sp = torch.sparse_csr_tensor(lg.indptr, lg.indices,
                                 torch.ones(lg.num_edges),
                                 size=(lg.num_inner, lg.num_nodes))
    ref = (torch.sparse.mm(sp, (x.cpu() * src.cpu()[:, None]))
           * dst.cpu()[:, None])
    assert torch.allclose(y.cpu(), ref, atol=1e-3, rtol=1e-4), \
        (y.cpu() - ref).abs().max()
    from kernel_oracles import check_spmm, segs_per_row
    check_spmm(lg.indptr, lg.indices, x.cpu(), src.cpu(), dst.cpu(), y.cpu(),
               segs_per_row(view))


def test_spmm_long_row_segmentation():
    """A hub row longer than SEG_EDGES must be split and its partial sums
    combined; result must still match the dense reference."""
    from adaqp_amd.ops.kernels import SpmmView, spmm, SEG_EDGES
    _native()
    torch.manual_seed(4)
    N, F = 300, 128
    hub_deg = 3 * SEG_EDGES + 17
    rows = [torch.randint(0, N, (hub_deg,))] + \
           [torch.randint(0, N, (torch.randint(1, 9, (1,)).item(),))
            for _ in range(49)]
    indptr = torch.zeros(51, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    indices = torch.cat(rows)
    x = torch.randn(N, F, device='cuda')
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, 50).to('cuda')
    assert view.zero_rows.numel() >= 1
    y = spmm(view, x, None, None, None)
    A = torch.zeros(50, N)
    for r in range(50):
        for c in indices[indptr[r]:indptr[r + 1]]:
            A[r, c] += 1
    ref = A @ x.cpu()
    assert torch.allclose(y.cpu(), ref, atol=1e-2, rtol=1e-4)
    from kernel_oracles import check_spmm, segs_per_row
    check_spmm(indptr, indices, x.cpu(), None, None, y.cpu(),
               segs_per_row(view))


@pytest.mark.parametrize('col_block', [0, 64])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_spmm_split_rows_bit_reproducible(dtype, col_block):
    """Rows split across segments (several hubs, an empty row, more
    segments than one block holds) are combined in a fixed order: repeated
    calls give bit-identical results, and fp32 matches the dense reference
    (same bound as test_spmm_long_row_segmentation: ~800 fp32 terms)."""
    from adaqp_amd.ops.kernels import SpmmView, spmm, SEG_EDGES
    _native()
    gen = torch.Generator().manual_seed(11)
    N, F, R = 300, 136, 70            # F: no multiple of the 64x4 lane tile
    degs = [3 * SEG_EDGES + 17, 0, 2 * SEG_EDGES, SEG_EDGES + 1, SEG_EDGES] + \
        torch.randint(1, 9, (R - 5,), generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.randint(0, N, (int(indptr[-1]),), generator=gen)
    x = torch.randn(N, F, generator=gen).to('cuda', dtype)
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, R,
                    col_block=col_block).to('cuda')
    assert view.n_part >= 3 + 2 + 2
    assert int(view.part_ptr[-1]) == view.n_part
    assert int(view.seg_part.max()) == view.n_part - 1
    y0 = spmm(view, x, None, None, None).clone()
    for _ in range(3):
        assert torch.equal(spmm(view, x, None, None, None), y0)
    assert torch.equal(y0[1], torch.zeros(F, device='cuda', dtype=dtype))
    A = torch.zeros(R, N)
    A.index_put_((torch.repeat_interleave(torch.arange(R),
                                          torch.tensor(degs)), indices),
                 torch.ones(indices.numel()), accumulate=True)
    ref = A @ x.float().cpu()          # exact inputs, fp32 accumulate
    if dtype == torch.float32:
        assert torch.allclose(y0.cpu(), ref, atol=1e-2, rtol=1e-4)
    else:
        # fp32 accumulate, ONE rounding to bf16 (8 significand bits: half
        # an ulp is 2^-9 relative) on top of the fp32 bound above
        assert torch.allclose(y0.float().cpu(), ref, atol=1e-2, rtol=2 ** -8)


def test_spmm_empty_rows():
    from adaqp_amd.ops.kernels import SpmmView, spmm
    _native()
    indptr = torch.tensor([0, 0, 2, 2], dtype=torch.int64, device='cuda')
    indices = torch.tensor([0, 2], dtype=torch.int64, device='cuda')
    x = torch.randn(4, 8, device='cuda')
    view = SpmmView(indptr, indices, 0, 3).to('cuda')
    y = spmm(view, x, None, None, None)
    assert torch.allclose(y[0], torch.zeros(8, device='cuda'))
    assert torch.allclose(y[1].cpu(), x[0].cpu() + x[2].cpu(), atol=1e-5)
    assert torch.allclose(y[2], torch.zeros(8, device='cuda'))


def test_e2e_train_step_gpu():
    """One AdaQP train epoch on 1 GPU, native kernels on the hot path."""
    import os
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29781')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import train_epoch, global_train_count
    from adaqp_amd.models import DistGCN
    from adaqp_amd.helpers import RunMode, DistGNNType
    from adaqp_amd.graph import random_partitioned_graph, partition_all
    comm = Communicator()
    try:
        g = random_partitioned_graph(3000, 30000, 32, 7, 1, seed=5)
        lg = partition_all(g, 1)[0]
        engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistGCN,
                             msg_dims=[32, 16, 16], device=comm.device)
        engine.set_uniform_assignment(4)
        model = DistGCN(32, 16, 7, 3).to(comm.device)
        opt = torch.optim.Adam(model.parameters())
        gc = global_train_count(engine)
        engine.timer.enabled = True    # event-based spans must not break
        l0 = float(train_epoch(engine, model, opt, gc, False))
        for _ in range(20):
            l = float(train_epoch(engine, model, opt, gc, False))
        row = engine.timer.epoch_rollup()
        assert sum(row) > 0, 'event timer recorded nothing'
        assert torch.isfinite(torch.tensor(l))
        assert l < l0  # training must reduce loss on a learnable graph
    finally:
        Communicator.shutdown()


def test_spmm_bf16_matches_fp32(etol=0.02):
    from adaqp_amd.graph import random_partitioned_graph, partition_all
    from adaqp_amd.ops.kernels import SpmmView, spmm
    _native()
    torch.manual_seed(6)
    g = random_partitioned_graph(800, 8000, 4, 3, 1, seed=12)
    lg = partition_all(g, 1)[0]
    for F in (100, 256, 602):
        x = torch.randn(lg.num_nodes, F, device='cuda')
        src = torch.rand(lg.num_nodes, device='cuda') + 0.5
        dst = torch.rand(lg.num_inner, device='cuda') + 0.5
        view = SpmmView(lg.indptr.cuda(), lg.indices.cuda(), 0, lg.num_inner).to('cuda')
        y32 = spmm(view, x, None, src, dst)
        y16 = spmm(view, x.bfloat16(), None, src, dst)
        assert y16.dtype == torch.bfloat16
        scale = y32.abs().max()
        err = (y16.float() - y32).abs().max() / scale
        assert err < etol, (F, float(err))
        from kernel_oracles import check_spmm, segs_per_row
        for xin, yout in ((x, y32), (x.bfloat16(), y16)):
            check_spmm(lg.indptr, lg.indices, xin.cpu(), src.cpu(), dst.cpu(),
                       yout.cpu(), segs_per_row(view))


def test_quant_roundtrip_bf16():
    from adaqp_amd.comm.buffers import bytes_per_node
    C = _native()
    torch.manual_seed(7)
    n, F, bits = 32, 256, 8
    x = torch.randn(n, F, device='cuda', dtype=torch.bfloat16)
    rows = torch.arange(n, dtype=torch.int64, device='cuda')
    bpn = bytes_per_node(F, bits)
    off = rows * bpn
    payload = torch.zeros(n * bpn, dtype=torch.uint8, device='cuda')
    params = torch.zeros(2 * n, dtype=torch.bfloat16, device='cuda')
    C.quant_pack(x, rows, rows, off, bits, 11, payload, params)
    out = torch.zeros(n, F, device='cuda', dtype=torch.bfloat16)
    C.quant_unpack(payload, params, rows, rows, off, bits, F, out)
    xf = x.float()
    rng = xf.max(1).values - xf.min(1).values
    step = rng / (2 ** bits - 1)
    err = (out.float() - xf).abs().max(1).values
    assert (err <= step * 1.05 + rng * 0.02).all()


def test_e2e_train_step_bf16():
    import os
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29785')
    os.environ.setdefault('RANK', '0')
    os.environ.setdefault('WORLD_SIZE', '1')
    from adaqp_amd.comm import Communicator
    from adaqp_amd.runtime import GraphEngine
    from adaqp_amd.runtime.utils import train_epoch, global_train_count
    from adaqp_amd.models import DistSAGE
    from adaqp_amd.helpers import RunMode, DistGNNType
    from adaqp_amd.graph import random_partitioned_graph, partition_all
    if Communicator.ctx is None:
        comm = Communicator()
    else:
        comm = Communicator.ctx
    g = random_partitioned_graph(3000, 30000, 32, 7, 1, seed=5,
                                 teacher_labels=True)
    lg = partition_all(g, 1)[0]
    engine = GraphEngine(lg, RunMode('AdaQP'), DistGNNType.DistSAGE,
                         msg_dims=[32, 16, 16], device=comm.device)
    engine.compute_dtype = torch.bfloat16
    engine.set_uniform_assignment(8)
    model = DistSAGE(32, 16, 7, 3, dropout=0.0).to(comm.device)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    gc = global_train_count(engine)
    l0 = float(train_epoch(engine, model, opt, gc, False))
    for _ in range(25):
        l = float(train_epoch(engine, model, opt, gc, False))
    assert torch.isfinite(torch.tensor(l)) and l < l0
    Communicator.shutdown()


def test_fused_dual_gemm_bf16():
    """Hand-written MFMA kernel vs torch reference. Uses ASYMMETRIC
    weights (guide G9: symmetric B hides transposed C-writes)."""
    C = _native()
    torch.manual_seed(9)
    for (M, K1, K2, N) in [(1000, 104, 256, 256), (64, 32, 32, 64),
                           (77, 8, 16, 48)]:
        a1 = torch.randn(M, K1, device='cuda').bfloat16()
        a2 = torch.randn(M, K2, device='cuda').bfloat16()
        w1 = torch.randn(K1, N, device='cuda').bfloat16()
        w2 = torch.randn(K2, N, device='cuda').bfloat16()
        bias = torch.randn(N, device='cuda').bfloat16()
        out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
        C.fused_dual_gemm_bf16(a1, a2, w1.t().contiguous(),
                               w2.t().contiguous(), bias, out)
        ref = (a1.float() @ w1.float() + a2.float() @ w2.float()
               + bias.float())
        scale = ref.abs().max().clamp(min=1.0)
        err = (out.float() - ref).abs().max() / scale
        assert err < 0.02, (M, K1, K2, N, float(err))
        from kernel_oracles import check_dual_gemm
        check_dual_gemm(a1, a2, w1, w2, bias, out)
    # transpose detection: A = one-hot rows, W asymmetric
    M, K, N = 32, 32, 32
    a1 = torch.zeros(M, K, device='cuda')
    a1[torch.arange(M), torch.arange(M) % K] = 1.0
    a1 = a1.bfloat16()
    a2 = torch.zeros(M, K, device='cuda').bfloat16()
    w1 = (torch.arange(K, device='cuda')[:, None] * 100.0
          + torch.arange(N, device='cuda')[None, :]).bfloat16()
    w2 = torch.zeros(K, N, device='cuda').bfloat16()
    out = torch.empty(M, N, device='cuda', dtype=torch.bfloat16)
    C.fused_dual_gemm_bf16(a1, a2, w1.t().contiguous(), w2.t().contiguous(),
                           torch.empty(0, device='cuda', dtype=torch.bfloat16),
                           out)
    ref = a1.float() @ w1.float()
    assert torch.allclose(out.float(), ref, atol=2.0), \
        (out.float() - ref).abs().max()


def test_spmm_blocked_matches_plain():
    """Column-blocked edge ordering must give identical results (up to
    fp reordering) to the plain row-major layout."""
    from adaqp_amd.graph import random_partitioned_graph, partition_all
    from adaqp_amd.ops.kernels import SpmmView, spmm
    _native()
    torch.manual_seed(13)
    g = random_partitioned_graph(2000, 40000, 4, 3, 1, seed=31)
    lg = partition_all(g, 1)[0]
    F = 128
    x = torch.randn(lg.num_nodes, F, device='cuda')
    src = torch.rand(lg.num_nodes, device='cuda') + 0.5
    dst = torch.rand(lg.num_inner, device='cuda') + 0.5
    v0 = SpmmView(lg.indptr.cuda(), lg.indices.cuda(), 0, lg.num_inner).to('cuda')
    v1 = SpmmView(lg.indptr.cuda(), lg.indices.cuda(), 0, lg.num_inner,
                  col_block=256).to('cuda')
    y0 = spmm(v0, x, None, src, dst)
    y1 = spmm(v1, x, None, src, dst)
    assert torch.allclose(y0, y1, atol=1e-3, rtol=1e-4), \
        (y0 - y1).abs().max()
