"""The aggregation oracles (tests/agg_oracles.py) on the GPU path: three
ranks share cuda:0 over the gloo-staged transport, so the HIP quant /
SpMM kernels, the comm stream, the ``out=`` row slices and the bf16 casts
are what is checked — forward AND backward, with two peers per rank and
mixed bit widths. RCCL itself is out of scope (one GPU per process group
member). The three workers are spawned once for the whole module; with
the pytest process that makes four processes holding the GPU."""
import pytest

import agg_oracles as A

pytestmark = pytest.mark.gpu

PORT = 29821
DTYPES = ('fp32', 'bf16')
CASES = A.case_list(DTYPES)


@pytest.fixture(scope='module')
def results():
    return A.spawn_workers(PORT, 'cuda:0', DTYPES, ())


@pytest.mark.parametrize('cid', CASES)
def test_case_on_gpu(results, cid):
    bad, n = A.failures(results, cid)
    assert n >= 3 * 6, f'{cid}: only {n} checks ran'
    assert not bad, '\n'.join(f'[{label}] {text}' for _, label, text in bad)
