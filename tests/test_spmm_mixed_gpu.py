"""The bf16-gather SpMM pieces (csrc/spmm_mixed.hip). ``round_rows_bf16`` on
the GPU must give the CPU definition's bits and round every finite value to
one of its two bf16 neighbours; the mixed ``spmm`` (bf16 rows in, fp32
accumulators, addend and output) must equal the fp32 kernel fed the widened
rows bit for bit, and pass the float64 oracle's counted bound."""
import functools
import itertools

import pytest
import torch

import kernel_oracles as K
from test_spmm_mixed_cpu import special_rows

pytestmark = pytest.mark.gpu

ROUND_FEATS = (256, 104, 17, 6)
# VE/SW per F: 256 8/32, 136 8/32, 104 8/16, 602 2/64 (5 chunks), 20 4/16,
# 6 2/16
GATHER_FEATS = (256, 136, 104, 602, 20, 6)
ROWS = 150


def _i32(t):
    return t.contiguous().view(torch.int32)


def _i16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize('F', ROUND_FEATS)
def test_round_rows_matches_cpu_and_rounds_to_a_neighbour(F):
    from adaqp_amd.ops.kernels import native, round_rows_bf16
    native()
    gen = torch.Generator().manual_seed(900 + F)
    x = torch.cat([special_rows(F), K.quant_input(ROWS - 3, F, gen)])
    b = x.view(torch.int32)
    assert all(((b & 0xFFFF) == lo).any() for lo in (0, 0xFFFF))
    assert torch.isnan(x).any() and torch.isinf(x).any()
    got = {}
    for seed, tag_base in ((1234, 0), (2 ** 32 + 5, 180)):
        g = round_rows_bf16(x.cuda(), seed, tag_base)
        assert g.dtype == torch.bfloat16 and g.shape == x.shape
        assert torch.equal(_i16(g), _i16(round_rows_bf16(x.cuda(), seed, tag_base)))
        g = got[seed] = g.cpu()
        assert torch.equal(_i16(g), _i16(round_rows_bf16(x, seed, tag_base)))
    assert not torch.equal(_i16(got[1234]), _i16(got[2 ** 32 + 5]))
    # the two neighbours: the truncated pattern and the next one away from 0
    fin = torch.isfinite(x)
    down = (b >> 16).to(torch.int16)
    o = _i16(got[1234])
    exact = (b & 0xFFFF) == 0
    assert ((o == down) | ((o == down + 1) & ~exact))[fin].all()
    assert (o == down)[fin & exact].all()
    assert torch.equal(torch.isnan(got[1234]), torch.isnan(x))
    assert torch.equal(got[1234][torch.isinf(x)], x[torch.isinf(x)].bfloat16())


@functools.lru_cache(maxsize=None)
def _view():
    from adaqp_amd.ops.kernels import SpmmView, native
    native()
    indptr, indices, _, _ = K.split_rows_graph()
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, K.SR_R).to('cuda')
    assert view.n_part > 0 and view.zero_rows.numel() > 0
    return view


@pytest.mark.parametrize('F', GATHER_FEATS)
def test_bf16_gather_equals_fp32_kernel_on_widened_rows(F):
    from adaqp_amd.ops.kernels import spmm
    indptr, indices, src, dst = K.split_rows_graph()
    view = _view()
    x = K.split_rows_x(F, torch.bfloat16)
    xb, xrb = x[:K.SR_NL].cuda(), x[K.SR_NL:].cuda()
    addend = torch.randn(K.SR_R, F, generator=torch.Generator().manual_seed(3)).cuda()
    segs = K.segs_per_row(view)
    for ss, ds in itertools.product([False, True], repeat=2):
        s, d = (src if ss else None), (dst if ds else None)
        kw = dict(src_scale=s.cuda() if ss else None,
                  dst_scale=d.cuda() if ds else None)
        for ad in (False, True):
            a = addend if ad else None
            wide = spmm(view, xb.float(), xrb.float(), addend=a, **kw)
            out = torch.full((K.SR_R, F), float('nan'), device='cuda')
            got = spmm(view, xb, xrb, addend=a, out=out,
                       out_dtype=torch.float32, **kw)
            assert got.data_ptr() == out.data_ptr()
            assert got.dtype == torch.float32
            assert torch.equal(_i32(got), _i32(wide)), (F, ss, ds, ad)
            if not ad:
                K.check_spmm(indptr, indices, x.float(), s, d, got.cpu(), segs)
