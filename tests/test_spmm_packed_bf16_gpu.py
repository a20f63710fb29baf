"""``pack_rows_bf16`` decoded from the layout in csrc/spmm_packed_bf16.hip, and
the bf16 packed-gather SpMM, which must equal the dense bf16 kernel bit for
bit. The graph, inputs and engines are those of the fp32 tests."""
import copy
import itertools

import pytest
import torch

from kernel_oracles import check_spmm, segs_per_row
from test_sage_packed_layer_gpu import _engine, comm            # noqa: F401
from test_spmm_packed_gpu import R, _graph, _view, _xs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def _special_rows(F, gen):
    half = F // 2
    def with_nnz(pos):
        v = torch.randn(len(pos), generator=gen) + 3.0
        return torch.zeros(F).index_put_((pos,), v)
    perm = torch.randperm(F, generator=gen)
    rows = [torch.zeros(F), with_nnz(perm[:half]), with_nnz(perm[:half + 1]),
            torch.randn(F, generator=gen) + 5.0, torch.zeros(F)]
    rows[4][0], rows[4][1] = -0.0, 1e-40             # bf16 denormal
    rows[4][half], rows[4][F - 1] = float('nan'), float('inf')
    for _ in range(6):                               # ~25 % dense
        r = torch.randn(F, generator=gen)
        r[torch.rand(F, generator=gen) >= 0.25] = 0.0
        rows.append(r)
    rows.append(with_nnz(torch.arange(F - half, F)))  # run ends at F - 1
    rows.append(with_nnz(torch.arange(half)))        # last: capacity full early
    x = torch.stack(rows).to(BF)
    nnz = (_bits(x) != 0).sum(1)
    assert nnz[:5].tolist() == [0, half, half + 1, F, 4]
    return x, (nnz > half).tolist()


def _decode(buf, n, F, meta, stride):
    # overflow rows decode to None; odd: rows with a group at an odd halfword
    raw, out, odd = buf.cpu(), [], set()
    for r in range(n):
        row = raw[r * stride:(r + 1) * stride]
        words = _bits(row[:F // 4]).tolist()
        if all(w == 0xFFFF for w in words):
            out.append(None)
            continue
        vals = _bits(row[meta:meta + F])
        dec, run = torch.zeros(F, dtype=torch.int32), 0
        for g, w in enumerate(words):
            assert w >> 8 == run, 'offset is not the count of values before'
            odd |= {r} if run & 1 and w & 0xFF else set()
            for k in range(8):
                if w >> k & 1:
                    dec[8 * g + k] = vals[run]
                    run += 1
        assert run <= F // 2
        out.append(dec)
    return out, odd


@pytest.mark.parametrize('F', [256, 104, 48, 8])
def test_pack_round_trip(F):
    from adaqp_amd.ops.kernels import pack_rows_bf16
    x, want_ovf = _special_rows(F, torch.Generator().manual_seed(11 + F))
    n = len(want_ovf)
    p = pack_rows_bf16(x.cuda())
    assert p is not None and (p.rows, p.feats) == (n, F)
    assert p.meta_bytes == (2 * (F // 8) + 15) // 16 * 16
    assert p.stride == (p.meta_bytes + F + 127) // 128 * 128
    assert p.buf.dtype == torch.uint8 and p.buf.numel() == n * p.stride + 20
    assert F != 256 or (p.meta_bytes, p.stride) == (64, 384)
    dec, odd = _decode(p.buf, n, F, p.meta_bytes, p.stride)
    assert [d is None for d in dec] == want_ovf
    assert odd & set(range(5, 11)) or F == 8    # among the ~25 % dense rows
    xi = _bits(x)
    for r, d in enumerate(dec):
        assert d is None or torch.equal(d, xi[r]), f'row {r}'


@pytest.mark.parametrize('density', [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize('F', [256, 104, 8])
def test_packed_spmm_equals_dense(F, density):
    from adaqp_amd.ops.kernels import pack_rows_bf16, spmm
    xl, xr = (t.to(BF).cuda() for t in _xs(F, density))
    p = pack_rows_bf16(xl)
    nnz = (_bits(xl) != 0).sum(1)
    if F == 256 and density == 0.5:                  # a mix of both kinds
        assert (nnz > F // 2).any() and (nnz <= F // 2).any()
    addend = torch.randn(R, F).to(BF).cuda()
    for remote, ss, ds, ad in itertools.product([False, True], repeat=4):
        indptr, indices, src, dst = _graph(remote)
        view = _view(remote)
        kw = dict(x_remote=xr if remote else None,
                  src_scale=src.cuda() if ss else None,
                  dst_scale=dst.cuda() if ds else None)
        kw['addend'] = addend if ad else None
        dense = spmm(view, xl, **kw)
        for depth in (4, 8):
            out = torch.full((R, F), float('nan'), dtype=BF, device='cuda')
            got = spmm(view, xl, out=out, packed=p, packed_depth=depth, **kw)
            assert torch.equal(_bits(got), _bits(dense)), \
                (remote, ss, ds, ad, depth)
        if remote and ss and ds and not ad:
            check_spmm(indptr, indices, torch.cat([xl, xr]).cpu(), src, dst,
                       got.cpu(), segs_per_row(view))


def _count_packs(monkeypatch):
    import adaqp_amd.ops.kernels as K
    calls, real = [], K.pack_rows_bf16
    monkeypatch.setattr(K, 'pack_rows_bf16',
                        lambda x: calls.append(real(x)) or calls[-1])
    return calls


def _same(res):
    assert len(res['0']) == len(res['1']) >= 6
    for a, b in zip(res['0'], res['1']):
        assert a is not None and torch.equal(a, b)


def test_bf16_layer_switch_on_off(comm, monkeypatch):           # noqa: F811
    from adaqp_amd.models.common import FastLinear, sage_mean_layer
    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    calls = _count_packs(monkeypatch)
    f_in, f_out = 256, 48
    engine = _engine(comm, [64, f_in, f_in])
    engine.compute_dtype = BF
    dev, n = comm.device, engine.graph.num_inner
    gen = torch.Generator().manual_seed(7)
    x0 = torch.relu(torch.randn(n, f_in, generator=gen))
    x0 = (x0 * (torch.rand(n, f_in, generator=gen) < 0.5) * 2.0).to(dev)
    g = torch.randn(n, f_out, generator=gen).to(dev)
    torch.manual_seed(5)
    lins = [FastLinear(f_in, f_out).to(dev) for _ in range(2)]
    res = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('ADAQP_SPMM_PACKED_BF16', flag)
        l1, l2 = copy.deepcopy(lins)
        x = x0.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=BF):
            out = sage_mean_layer(engine, x, l1, l2, 1, True, pack=True)
        out.backward(g.to(out.dtype))
        res[flag] = [out.detach(), x.grad] + [p.grad for lin in (l1, l2)
                                              for p in lin.parameters()]
        assert len(calls) == int(flag) and None not in calls
    _same(res)


def test_bf16_distsage_switch_on_off(comm, monkeypatch):        # noqa: F811
    from adaqp_amd.models import DistSAGE
    monkeypatch.setenv('ADAQP_AGG0_CACHE', '0')
    monkeypatch.delenv('ADAQP_FUSED_NORM', raising=False)
    monkeypatch.delenv('ADAQP_SPMM_PACKED', raising=False)
    calls = _count_packs(monkeypatch)
    engine = _engine(comm, [64, 256, 256])
    engine.compute_dtype = BF
    torch.manual_seed(2)
    model0 = DistSAGE(64, 256, 10, 3).to(comm.device)
    res = {}
    for flag in ('0', '1'):
        monkeypatch.setenv('ADAQP_SPMM_PACKED_BF16', flag)
        model = copy.deepcopy(model0).train()
        torch.manual_seed(123)
        with torch.autocast('cuda', dtype=BF):
            logits = model(engine, engine.graph.feats)
        logits.float().square().sum().backward()
        res[flag] = [logits.detach()] + [p.grad for p in model.parameters()]
        assert len(calls) == 2 * int(flag) and None not in calls
    _same(res)
