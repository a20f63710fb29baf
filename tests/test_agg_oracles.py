"""CPU run of the aggregation oracles (tests/agg_oracles.py): three gloo
ranks run every fp32 case through the torch reference path, then each
planted fault, and the checkers' own unit tests. The GPU run of the same
worker is tests/test_dist_agg_gpu.py."""
import pytest
import torch

import agg_oracles as A
from adaqp_amd.ops import quant as Q

PORT = 29811
CASES = A.case_list(('fp32',))


@pytest.fixture(scope='module')
def results():
    """One spawn of the three ranks for the whole module."""
    return A.spawn_workers(PORT, 'cpu', ('fp32',), tuple(A.FAULTS))


def test_case_shape():
    g, lgs = A.build_case()
    assert len(lgs) == 3 and g.num_nodes == A.N_NODES
    assert len(CASES) == 12


@pytest.mark.parametrize('cid', CASES)
def test_case_on_cpu(results, cid):
    bad, n = A.failures(results, cid)
    assert n >= 3 * 6, f'{cid}: only {n} checks ran'
    assert not bad, '\n'.join(f'[{label}] {text}' for _, label, text in bad)


@pytest.mark.parametrize('fault', list(A.FAULTS))
def test_fault_is_caught(results, fault):
    """Each planted fault must make its checker raise on every rank."""
    cid, label = A.FAULTS[fault]
    bad, n = A.failures(results, cid, fault)
    assert n, f'{fault}: case {cid} did not run'
    ranks = sorted(r for r, l, _ in bad if l == label)
    assert ranks == [0, 1, 2], \
        f'{fault}: check {label} raised on ranks {ranks} only; failures: {bad}'


# ---- the operator oracle against itself ----

@pytest.mark.parametrize('kind,agg', A.MODELS)
def test_backward_is_transpose_of_forward(kind, agg):
    """<G, fwd(X)> == <bwd(G), X> in float64 (1e-12 relative: ~1200-term
    float64 sums of O(100) products)."""
    g, _ = A.build_case()
    X, G = A.case_tensors(24, torch.float32)
    yf, _ = A.global_operator(g, kind, agg, A.FWD, X)
    yb, _ = A.global_operator(g, kind, agg, A.BWD, G)
    a = (G.double() * yf).sum()
    b = (yb * X.double()).sum()
    assert abs(float(a - b)) <= 1e-12 * abs(float(a))


# ---- check_dequantized from pack_torch / unpack_torch ----

def _roundtrip(bits, dtype=torch.float32, wide=False):
    X, _ = A.case_tensors(24, torch.float32)
    x = X[:90]
    if wide:
        # range ~64 around 4: the bf16 rounding of rmin (<= 2^-4) is at
        # most a quarter of the 8-bit step (~0.25). The 8-bit bound is then
        # 1 step + 2^-8 * range (255/256 step) + that quarter, about 2.25
        # steps, and a row shifted by two steps has an element beyond it
        # (stochastic-rounding errors fill (-1, 1) steps). On the case
        # rows (range ~4, rmin ~6) rmin's rounding alone is ~0.8 step.
        x = torch.randn(90, 24, generator=torch.Generator().manual_seed(8)) * 16 + 4
    tag = torch.arange(90)
    pl, scale, rmin = Q.pack_torch(x, bits, 1234, tag)
    out = Q.unpack_torch(pl, bits, scale, rmin, 24).to(dtype)
    return x, torch.full((90,), bits), out, scale


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('bits', A.BITS)
def test_check_dequantized_accepts_roundtrip(bits, dtype):
    x, b, out, _ = _roundtrip(bits, dtype)
    assert A.check_dequantized(x, b, out) <= 1.0


@pytest.mark.parametrize('bits', A.BITS)
def test_check_dequantized_rejects_two_steps(bits):
    x, b, out, scale = _roundtrip(bits, wide=True)
    A.check_dequantized(x, b, out)
    out = out.clone()
    out[17] += 2.0 / scale.float()[17]
    with pytest.raises(AssertionError, match=r'remote\[17, '):
        A.check_dequantized(x, b, out)


def test_check_dequantized_mixed_bits_and_constant_row():
    X, _ = A.case_tensors(24, torch.float32)
    x = X[:90].clone()
    x[5] = 0.75
    bits = A.fwd_bits(torch.arange(90))
    out = torch.empty_like(x)
    for b in A.BITS:
        sel = torch.nonzero(bits == b, as_tuple=True)[0]
        pl, scale, rmin = Q.pack_torch(x[sel], b, 99, sel)
        out[sel] = Q.unpack_torch(pl, b, scale, rmin, 24)
    A.check_dequantized(x, bits, out)
    with pytest.raises(AssertionError):     # 2-bit rows judged as 8-bit
        A.check_dequantized(x, torch.full_like(bits, 8), out)
