"""One-launch mixed-bit quantizer (csrc/quant_mixed.hip) on the GPU: the
same wire bytes and params as the per-bit launches of ``mixed_quantize``,
nothing written outside them, levels inside the float64 oracle's admissible
set, and a variance trace equal to ``GraphEngine.trace``'s bit for bit."""
import types

import pytest
import torch

import kernel_oracles as K
from adaqp_amd.comm.buffers import BITS_SET, _layout
from adaqp_amd.ops import kernels as OK
from adaqp_amd.runtime.engine import GraphEngine

pytestmark = pytest.mark.gpu

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}
PATTERNS = {'all2': (2,), 'all4': (4,), 'all8': (8,), 'mix': BITS_SET}
# 4: one live lane of 16; 104: 26-byte rows at 2 bits, every alignment;
# 128: two rows per wave; 256: one full pass; 260: a second chunk with one
# live lane; 1024: the register-staging limit
FEATS = (4, 104, 128, 256, 260, 1024)
N, SEED, PAD = 150, 12345, 13
BOTH, CONST, NEGZERO, PAIR = 5, 7, 11, 13


def make_case(dtype, pattern, F, send_tab=True):
    """(x [N, F] on the GPU, send SidePlan on the GPU): 110 + 90 send slots
    over two peers; row BOTH goes to both, CONST is constant, NEGZERO holds
    -0.0 entries, PAIR a +-1e15 pair among O(1) values."""
    gen = torch.Generator().manual_seed(3000 + F)
    x = K.quant_input(N, F, gen)
    x[CONST] = 0.75
    x[NEGZERO, ::3] = -0.0
    x[PAIR, 0], x[PAIR, F - 1] = 1e15, -1e15
    rows = [torch.cat([torch.tensor([BOTH, CONST, NEGZERO, PAIR]),
                       torch.randperm(N, generator=gen)[:106]]),
            torch.cat([torch.tensor([BOTH]),
                       torch.randperm(N, generator=gen)[:89]])]
    pat = torch.tensor(PATTERNS[pattern])
    bits = [pat[torch.arange(r.numel()) % pat.numel()] for r in rows]
    plan = _layout(bits, rows, F, row_tab=False, send_tab=send_tab)
    return x.to(dtype).cuda(), plan.to('cuda')


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8),
                                              b.view(torch.uint8))


@pytest.mark.parametrize('F', FEATS)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dt', DTYPES)
def test_fused_equals_per_bit(dt, pattern, F):
    x, plan = make_case(DTYPES[dt], pattern, F)
    assert OK.quant_mixed_fast(x, plan)
    ref_p, ref_q = OK.mixed_quantize(x, plan, SEED)
    got_p, got_q = OK.mixed_quantize_fused(x, plan, SEED)
    assert same_bits(got_p, ref_p) and same_bits(got_q, ref_q)
    # the same launch into the middle of poisoned buffers, at an odd offset
    S, B = plan.total_nodes, plan.total_bytes
    pbuf = torch.full((B + 2 * PAD,), 0xA5, dtype=torch.uint8, device='cuda')
    qbuf = torch.full((2 * S + 8,), -7.0, dtype=torch.bfloat16, device='cuda')
    OK.native().quant_pack_mixed(x, plan.send_tab, SEED, pbuf[PAD:PAD + B],
                                 qbuf[4:4 + 2 * S],
                                 torch.empty(0, device='cuda'))
    assert same_bits(pbuf[PAD:PAD + B], ref_p)
    assert same_bits(qbuf[4:4 + 2 * S], ref_q)
    assert (pbuf[:PAD] == 0xA5).all() and (pbuf[PAD + B:] == 0xA5).all()
    assert (qbuf[:4] == -7.0).all() and (qbuf[4 + 2 * S:] == -7.0).all()


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_levels_against_float64_oracle(dt):
    F = 104
    x, plan = make_case(DTYPES[dt], 'mix', F)
    payload, params = (t.cpu() for t in OK.mixed_quantize_fused(x, plan, SEED))
    for b in BITS_SET:
        rows, pos = plan.rows[b].cpu(), plan.pos[b].cpu()
        idx = plan.off[b].cpu()[:, None] + torch.arange(K.Q.bytes_per_node(F, b))
        K.check_packed(x.cpu()[rows].float(), b, SEED, pos, payload[idx],
                       params[2 * pos], params[2 * pos + 1])


@pytest.mark.parametrize('F', (128, 260))
@pytest.mark.parametrize('dt', DTYPES)
def test_trace_equals_engine_trace(dt, F):
    x, plan = make_case(DTYPES[dt], 'mix', F)
    acc = torch.zeros(plan.total_nodes, device='cuda')
    ref_p, _ = OK.mixed_quantize(x, plan, SEED + 1)
    for seed in (SEED, SEED + 1):
        got_p, _ = OK.mixed_quantize_fused(x, plan, seed, trace=acc)
    assert same_bits(got_p, ref_p)
    send = x.index_select(0, plan.send_rows)
    eng = types.SimpleNamespace(traced={})
    for _ in range(2):
        GraphEngine.trace(eng, 'k', send)
    assert same_bits(acc, eng.traced['k'])
    # float64: rng has one fp32 rounding (bf16: plus half a bf16 ulp, e = 2^-8
    # relative), squared: 2e + e^2; the square, c, the product and the sum
    # round once each. 8 * U32 covers the fp32 roundings.
    s64 = send.double()
    ref = 2 * (F / 6.0) * (s64.max(dim=1).values - s64.min(dim=1).values) ** 2
    rel = 8 * K.U32 + (2 * 2.0 ** -8 + 2.0 ** -16 if dt == 'bf16' else 0.0)
    assert ((acc.double() - ref).abs() <= rel * ref).all()
    assert float(acc[1]) == 0.0 and float(acc[3]) > 1e29    # CONST, PAIR slots


@pytest.mark.parametrize('dt,F,send_tab', [('fp32', 6, True), ('bf16', 1028, True),
                                           ('fp32', 128, False)])
def test_fallback_takes_the_per_bit_path(dt, F, send_tab):
    x, plan = make_case(DTYPES[dt], 'mix', F)
    if not send_tab:
        plan.send_tab = None
    assert not OK.quant_mixed_fast(x, plan)
    acc = torch.zeros(plan.total_nodes, device='cuda')
    ref_p, ref_q = OK.mixed_quantize(x, plan, SEED)
    got_p, got_q = OK.mixed_quantize_fused(x, plan, SEED, trace=acc)
    assert same_bits(got_p, ref_p) and same_bits(got_q, ref_q)
    assert same_bits(acc, OK.trace_rows(x.index_select(0, plan.send_rows)))


def test_exchange_start_same_wire_and_trace_with_the_switch_on():
    from adaqp_amd.ops.dist_agg import _exchange_start
    from adaqp_amd.runtime.timer import Timer
    x, plan = make_case(torch.float32, 'mix', 128)
    out = {}
    for fused in (False, True):
        eng = types.SimpleNamespace(
            plans={'k': types.SimpleNamespace(send=plan)}, is_tracing=True,
            traced={}, fused_quant=fused, timer=Timer(enabled=False),
            device=x.device, next_seed=lambda: SEED,
            graph=types.SimpleNamespace(total_send_idx=plan.send_rows,
                                        num_send=plan.total_nodes))
        for name in ('trace', 'trace_accumulator'):
            setattr(eng, name, types.MethodType(getattr(GraphEngine, name), eng))
        for _ in range(2):
            _, payload, params, _ = _exchange_start(eng, x, 'k', True)
        out[fused] = (payload, params, eng.traced['k'])
    assert all(same_bits(a, b) for a, b in zip(out[False], out[True]))
