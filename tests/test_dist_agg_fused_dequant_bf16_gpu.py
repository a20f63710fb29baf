"""The bf16 aggregation oracles of test_dist_agg_gpu.py with
``ADAQP_FUSED_DEQUANT=1`` and ``ADAQP_FUSED_DEQUANT_BF16=1``: on three ranks
sharing cuda:0 the quantized cases' SpMMs gather remote columns from the wire
buffer (``QuantRemote``, csrc/spmm_quant_bf16.hip) instead of a dequantized
bf16 block. The spawned ranks inherit the variables."""
import types

import pytest
import torch

import agg_oracles as A

pytestmark = pytest.mark.gpu

PORT = 29837
CASES = A.case_list(('bf16',))


@pytest.fixture(scope='module')
def results():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('ADAQP_FUSED_DEQUANT', '1')
        mp.setenv('ADAQP_FUSED_DEQUANT_BF16', '1')
        return A.spawn_workers(PORT, 'cuda:0', ('bf16',), ())


@pytest.mark.parametrize('cid', CASES)
def test_case_on_gpu_fused_dequant_bf16(results, cid):
    bad, n = A.failures(results, cid)
    assert n >= 3 * 6, f'{cid}: only {n} checks ran'
    assert not bad, '\n'.join(f'[{label}] {text}' for _, label, text in bad)


def test_bf16_exchange_is_fused_only_with_both_switches_on():
    from adaqp_amd.ops.dist_agg import _fused_dequant
    plan = types.SimpleNamespace(recv=types.SimpleNamespace(row_tab=object()))
    x = torch.zeros(2, 4, dtype=torch.bfloat16, device='cuda')
    for fd, fb in ((True, True), (True, False), (False, True)):
        engine = types.SimpleNamespace(plans={'forward0': plan},
                                       fused_dequant=fd, fused_dequant_bf16=fb)
        assert _fused_dequant(engine, x, 'forward0', True) is (fd and fb)
        assert _fused_dequant(engine, x.float(), 'forward0', True) is fd
