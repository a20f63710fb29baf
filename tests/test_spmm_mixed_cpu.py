"""CPU side of the bf16-gather backward SpMM: ``round_rows_bf16`` against a
direct numpy evaluation of its definition, the mixed ``spmm`` call against
the widened fp32 call, and the ``bwd_gather_bf16`` switch."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import torch

import kernel_oracles as K
from adaqp_amd.ops import dist_agg as DA
from adaqp_amd.ops import kernels as OK

M32 = np.uint64(0xFFFFFFFF)


def special_rows(F):
    """fp32 [3, F] cycling through +-0, denormals, +-inf, NaNs (one with a
    payload in the low half only) and low halves 0x0000 / 0xFFFF."""
    pats = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000,
            0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000,
            0x3F80FFFF, 0xC2FFFFFF, 0x7F7FFFFF, 0x40490000]
    b = np.array([pats[i % len(pats)] for i in range(3 * F)], dtype=np.uint32)
    return torch.from_numpy(b.view(np.float32).reshape(3, F).copy())


def numpy_round(x, seed, tag_base):
    """The issue's formula, element by element in uint64 masked to 32 bits."""
    b = x.numpy().view(np.uint32).astype(np.uint64)
    N, F = b.shape
    t = (np.uint64(tag_base) + np.arange(N, dtype=np.uint64)) & M32
    f = np.arange(F, dtype=np.uint64)
    h = (np.uint64(seed & 0xFFFFFFFF) ^ ((t * np.uint64(0x9E3779B9)) & M32)[:, None]
         ^ ((f * np.uint64(0x85EBCA6B)) & M32)[None, :])
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x7FEB352D)) & M32
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x846CA68B)) & M32
    h ^= h >> np.uint64(16)
    special = (b & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    quiet = np.where((b & np.uint64(0x007FFFFF)) != 0, 0x40, 0).astype(np.uint64)
    out = np.where(special, (b >> np.uint64(16)) | quiet,
                   (b + (h >> np.uint64(16))) >> np.uint64(16))
    return out.astype(np.uint16)


def test_cpu_round_rows_matches_the_formula():
    F = 42
    x = torch.cat([special_rows(F), K.quant_input(21, F, torch.Generator().manual_seed(4))])
    assert x.numel() >= 1000
    for seed, tag_base in ((1234, 0), (2 ** 32 + 5, 0xFFFFFFF0)):
        got = OK.round_rows_bf16(x, seed, tag_base)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        want = numpy_round(x, seed, tag_base)
        assert np.array_equal(got.view(torch.int16).numpy().view(np.uint16), want)


def test_cpu_mixed_spmm_equals_widened():
    F = 20
    indptr, indices, src, dst = K.split_rows_graph()
    view = OK.SpmmView(indptr, indices, 0, K.SR_R)
    x = K.split_rows_x(F, torch.bfloat16)
    xl, xr = x[:K.SR_NL], x[K.SR_NL:]
    addend = torch.randn(K.SR_R, F, generator=torch.Generator().manual_seed(3))
    got = OK.spmm(view, xl, xr, src, dst, addend=addend,
                  out_dtype=torch.float32)
    assert got.dtype == torch.float32
    assert torch.equal(got, OK.spmm(view, xl.float(), xr.float(), src, dst,
                                    addend=addend))


def test_bwd_gather_switch_resolution(monkeypatch):
    spec = importlib.util.spec_from_file_location(
        'adaqp_main_gather',
        os.path.join(os.path.dirname(os.path.dirname(__file__)), 'main.py'))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    parser = main.build_parser()
    assert parser.parse_args(['--bwd_gather_bf16']).bwd_gather_bf16 is True
    assert parser.parse_args([]).bwd_gather_bf16 is False
    monkeypatch.delenv('ADAQP_BWD_GATHER_BF16', raising=False)
    assert not OK.resolve_bwd_gather_bf16(None)
    assert OK.resolve_bwd_gather_bf16(True)
    monkeypatch.setenv('ADAQP_BWD_GATHER_BF16', '1')      # read at resolution
    assert OK.resolve_bwd_gather_bf16(None)
    assert not OK.resolve_bwd_gather_bf16(False)
    # the callers' rule: switch on, fp32 engine, fp32 operand with even F;
    # the engine's flag (config key runtime.bwd_gather_bf16) beats the env
    eng = SimpleNamespace(bwd_gather_bf16=None, compute_dtype=torch.float32,
                          base_seed=2026, bwd_gather_calls=0)
    x = torch.zeros(3, 6)
    s0 = DA.next_bwd_gather_seed(eng, x, 1)
    s1 = DA.next_bwd_gather_seed(eng, x, 1)
    assert (s0, s1) == (DA.bwd_gather_seed(eng, 1, 0), DA.bwd_gather_seed(eng, 1, 1))
    assert s0 != s1 and eng.bwd_gather_calls == 2
    assert DA.next_bwd_gather_seed(eng, torch.zeros(3, 7), 1) is None
    assert DA.next_bwd_gather_seed(eng, x.bfloat16(), 1) is None
    eng.compute_dtype = torch.bfloat16
    assert DA.next_bwd_gather_seed(eng, x, 1) is None
    eng.compute_dtype, eng.bwd_gather_bf16 = torch.float32, False
    assert DA.next_bwd_gather_seed(eng, x, 1) is None
    assert eng.bwd_gather_calls == 2
    monkeypatch.delenv('ADAQP_BWD_GATHER_BF16')
    eng.bwd_gather_bf16 = True
    assert DA.next_bwd_gather_seed(eng, x, 1) == DA.bwd_gather_seed(eng, 1, 2)
