"""The fp32 and bf16 aggregation oracles of test_dist_agg_gpu.py with
``ADAQP_FUSED_QUANT=1``: on three ranks sharing cuda:0 every quantized
exchange packs its send set with the one-launch quantizer
(csrc/quant_mixed.hip). The spawned ranks inherit the variable."""
import pytest

import agg_oracles as A

pytestmark = pytest.mark.gpu

PORT = 29841
DTYPES = ('fp32', 'bf16')
CASES = A.case_list(DTYPES)


@pytest.fixture(scope='module')
def results():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('ADAQP_FUSED_QUANT', '1')
        return A.spawn_workers(PORT, 'cuda:0', DTYPES, ())


@pytest.mark.parametrize('cid', CASES)
def test_case_on_gpu_fused_quant(results, cid):
    bad, n = A.failures(results, cid)
    assert n >= 3 * 6, f'{cid}: only {n} checks ran'
    assert not bad, '\n'.join(f'[{label}] {text}' for _, label, text in bad)
