"""CPU tensors never take the packed path: ``pack_rows`` gives no handle,
a ``packed`` keyword is ignored, and results are what they were."""
import torch


def test_cpu_ignores_packed_operand():
    from adaqp_amd.ops.kernels import (PackedRows, SpmmView, pack_rows,
                                       packable, spmm)
    gen = torch.Generator().manual_seed(1)
    R, N, F = 12, 20, 8
    degs = torch.randint(0, 6, (R,), generator=gen)
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(degs, 0)
    indices = torch.randint(0, N, (int(indptr[-1]),), generator=gen)
    x = torch.relu(torch.randn(N, F, generator=gen))
    dst = torch.rand(R, generator=gen) + 0.5
    view = SpmmView(indptr, indices, 0, R)
    assert not packable(x) and pack_rows(x) is None
    want = spmm(view, x, None, None, dst)
    assert torch.equal(spmm(view, x, None, None, dst, packed=None), want)
    # even a handle is ignored on the CPU (no native code is touched)
    fake = PackedRows.__new__(PackedRows)
    assert torch.equal(spmm(view, x, None, None, dst, packed=fake), want)
    ref = torch.zeros(R, F)
    for r in range(R):
        for c in indices[indptr[r]:indptr[r + 1]].tolist():
            ref[r] += x[c]
    assert torch.allclose(want, ref * dst[:, None], rtol=1e-6, atol=1e-6)

