"""The fp32 aggregation oracles of test_dist_agg_gpu.py with
``ADAQP_FUSED_DEQUANT=1``: on three ranks sharing cuda:0 the quantized
cases' SpMMs gather remote columns from the wire buffer (``QuantRemote``)
instead of a dequantized block. The spawned ranks inherit the variable."""
import pytest

import agg_oracles as A

pytestmark = pytest.mark.gpu

PORT = 29831
CASES = A.case_list(('fp32',))


@pytest.fixture(scope='module')
def results():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('ADAQP_FUSED_DEQUANT', '1')
        return A.spawn_workers(PORT, 'cuda:0', ('fp32',), ())


@pytest.mark.parametrize('cid', CASES)
def test_case_on_gpu_fused_dequant(results, cid):
    bad, n = A.failures(results, cid)
    assert n >= 3 * 6, f'{cid}: only {n} checks ran'
    assert not bad, '\n'.join(f'[{label}] {text}' for _, label, text in bad)
