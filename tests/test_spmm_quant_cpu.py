"""CPU side of the quantized-gather SpMM: ``QuantRemote`` dequantizes on the
CPU, the plan's per-row table, and the ``fused_dequant`` switch."""
import importlib.util
import os

import torch

import kernel_oracles as K
from adaqp_amd.comm.buffers import BITS_SET
from adaqp_amd.ops import kernels as OK


def test_cpu_spmm_with_quant_remote_equals_dequantized():
    F = 17
    x, send, recv, n_out = K.mixed_plans(F)
    payload, params = OK.mixed_quantize(x, send, 5)
    qr = OK.QuantRemote(payload, params, recv, F, rows=n_out)
    xl = torch.randn(40, F, generator=torch.Generator().manual_seed(1))
    assert not qr.fusable(xl)
    gen = torch.Generator().manual_seed(2)
    deg = torch.randint(0, 6, (30,), generator=gen)
    indptr = torch.zeros(31, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.randint(0, 40 + n_out, (int(indptr[-1]),), generator=gen)
    view = OK.SpmmView(indptr, indices, 0, 30)
    assert view.max_col == int(indices.max())
    xr = OK.mixed_dequantize(payload, params, recv, torch.zeros(n_out, F))
    src = torch.rand(40 + n_out, generator=gen)
    assert torch.equal(qr.dequantize(), xr)
    assert torch.equal(OK.spmm(view, xl, qr, src, None),
                       OK.spmm(view, xl, xr, src, None))


def test_row_table_agrees_with_rows_pos_off():
    _, send, recv, n_out = K.mixed_plans(24)
    tab = recv.row_tab
    assert tab.dtype == torch.int32 and tab.shape[1] == 4
    covered = torch.zeros(tab.shape[0], dtype=torch.bool)
    for b in BITS_SET:
        r = recv.rows[b]
        assert r.numel()
        covered[r] = True
        assert torch.equal(tab[r, 0].long(), recv.off[b])
        assert torch.equal(tab[r, 1].long(), recv.pos[b])
        assert (tab[r, 2] == b).all() and (tab[r, 3] == 0).all()
    assert tab.shape[0] == int(torch.nonzero(covered).max()) + 1 <= n_out
    assert not covered.all() and (tab[~covered] == 0).all()
    assert OK.QuantRemote(torch.zeros(recv.total_bytes, dtype=torch.uint8),
                          torch.zeros(2 * recv.total_nodes, dtype=torch.bfloat16),
                          recv, 24).rows == tab.shape[0]


def test_fused_dequant_flag_resolution(monkeypatch):
    spec = importlib.util.spec_from_file_location(
        'adaqp_main_dequant',
        os.path.join(os.path.dirname(os.path.dirname(__file__)), 'main.py'))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    monkeypatch.delenv('ADAQP_FUSED_DEQUANT', raising=False)
    assert not OK.resolve_fused_dequant(None)
    monkeypatch.setenv('ADAQP_FUSED_DEQUANT', '1')      # read at resolution
    assert OK.resolve_fused_dequant(None)
    assert not OK.resolve_fused_dequant(False) and OK.resolve_fused_dequant(True)
    monkeypatch.delenv('ADAQP_FUSED_DEQUANT')
    assert OK.resolve_fused_dequant(True) and not OK.resolve_fused_dequant(None)
    parser = main.build_parser()
    assert parser.parse_args(['--fused_dequant']).fused_dequant is True
    assert parser.parse_args([]).fused_dequant is False
