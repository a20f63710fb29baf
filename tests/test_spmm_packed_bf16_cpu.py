"""What ``packable_bf16`` refuses, and that ``pack_rows_bf16`` gives no
handle for it without touching the extension."""
from types import SimpleNamespace

import pytest
import torch


def _gpu_shaped(n, F, dtype):
    """Stands in for a contiguous GPU tensor: shape, dtype and flags only."""
    return SimpleNamespace(is_cuda=True, shape=(n, F), dtype=dtype,
                           dim=lambda: 2, is_contiguous=lambda: True)


@pytest.mark.parametrize('x', [
    torch.zeros(4, 8, dtype=torch.bfloat16),             # CPU
    _gpu_shaped(4, 8, torch.float32),
    _gpu_shaped(4, 12, torch.bfloat16),
    _gpu_shaped(4, 264, torch.bfloat16),
], ids=['cpu', 'fp32', 'F12', 'F264'])
def test_unqualified_inputs(x, monkeypatch):
    import adaqp_amd.ops.kernels as K
    monkeypatch.setattr(K, 'native', lambda: pytest.fail('extension used'))
    assert not K.packable_bf16(x) and K.pack_rows_bf16(x) is None
    assert K.packable_bf16(_gpu_shaped(4, 256, torch.bfloat16))
