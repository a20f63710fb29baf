"""CPU side of the one-launch quantizer: the plan's send-slot table, the
``fused_quant`` switch, and ``mixed_quantize_fused`` off the GPU."""
import importlib.util
import os

import torch

import kernel_oracles as K
from adaqp_amd.comm.buffers import BITS_SET, _layout
from adaqp_amd.ops import kernels as OK


def test_send_table_agrees_with_rows_pos_off():
    gen = torch.Generator().manual_seed(11)
    counts = [31, 0, 7, 22]            # an empty peer, a single-width peer
    bits = [torch.tensor(BITS_SET)[torch.randint(0, 3, (k,), generator=gen)]
            if k else None for k in counts]
    bits[2] = torch.full((7,), 4)
    rows = [torch.randint(0, 40, (k,), generator=gen) if k else None
            for k in counts]
    plan = _layout(bits, rows, 24, row_tab=False, send_tab=True)
    tab = plan.send_tab
    assert tab.dtype == torch.int32 and tab.shape == (sum(counts), 4)
    assert plan.row_tab is None and plan.send_max_row == int(tab[:, 0].max())
    assert torch.equal(plan.send_rows, torch.cat([r for r in rows if r is not None]))
    assert torch.equal(tab[:, 0].long(), plan.send_rows)
    assert torch.equal(tab[:, 3].long(), torch.cat([b for b in bits if b is not None]))
    for b in BITS_SET:                 # slot order within a width is wire order
        s = torch.nonzero(tab[:, 3] == b, as_tuple=True)[0]
        assert torch.equal(tab[s, 0].long(), plan.rows[b])
        assert torch.equal(tab[s, 1].long(), plan.off[b])
        assert torch.equal(tab[s, 2].long(), plan.pos[b])
    assert _layout(bits, rows, 24).send_tab is None          # only when asked
    empty = _layout([None, None], [None, None], 24, send_tab=True)
    assert empty.send_tab.shape == (0, 4) and empty.send_max_row == -1


def test_send_table_is_none_past_32_bits():
    F = 2 ** 24                        # 16 MiB per 8-bit node, no allocation
    rows = [torch.arange(200), torch.arange(56)]
    bits = [torch.full((200,), 8), torch.full((56,), 8)]
    plan = _layout(bits, rows, F, row_tab=False, send_tab=True)
    assert plan.total_bytes == 2 ** 32 and plan.send_tab is None
    rows[1] = rows[1][:55]
    ok = _layout(bits[:1] + [bits[1][:55]], rows, F, row_tab=False, send_tab=True)
    assert ok.send_tab is not None
    assert int(ok.send_tab[-1, 1]) + 2 ** 32 == ok.off[8][-1]   # u32 bits
    rows[0] = rows[0] + 2 ** 31
    assert _layout(bits[:1] + [bits[1][:55]], rows, 4, row_tab=False,
                   send_tab=True).send_tab is None


def test_fused_quant_flag_resolution(monkeypatch):
    spec = importlib.util.spec_from_file_location(
        'adaqp_main_fused_quant',
        os.path.join(os.path.dirname(os.path.dirname(__file__)), 'main.py'))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    monkeypatch.delenv('ADAQP_FUSED_QUANT', raising=False)
    assert not OK.resolve_fused_quant(None)
    monkeypatch.setenv('ADAQP_FUSED_QUANT', '1')         # read at resolution
    assert OK.resolve_fused_quant(None)
    assert not OK.resolve_fused_quant(False) and OK.resolve_fused_quant(True)
    monkeypatch.delenv('ADAQP_FUSED_QUANT')
    assert OK.resolve_fused_quant(True) and not OK.resolve_fused_quant(None)
    parser = main.build_parser()
    assert parser.parse_args(['--fused_quant']).fused_quant is True
    assert parser.parse_args([]).fused_quant is False


def test_cpu_tensor_takes_the_per_bit_path():
    gen = torch.Generator().manual_seed(12)
    x = K.quant_input(50, 24, gen)
    rows = [torch.randint(0, 50, (30,), generator=gen),
            torch.randint(0, 50, (20,), generator=gen)]
    bits = [torch.tensor(BITS_SET)[torch.arange(k) % 3] for k in (30, 20)]
    plan = _layout(bits, rows, 24, row_tab=False, send_tab=True)
    assert not OK.quant_mixed_fast(x, plan)
    acc = torch.zeros(50)
    ref_p, ref_q = OK.mixed_quantize(x, plan, 9)
    for _ in range(2):
        got_p, got_q = OK.mixed_quantize_fused(x, plan, 9, trace=acc)
    assert torch.equal(got_p, ref_p) and torch.equal(got_q, ref_q)
    assert torch.equal(acc, 2 * OK.trace_rows(x[torch.cat(rows)]))
