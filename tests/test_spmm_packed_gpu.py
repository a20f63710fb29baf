"""Packed sparse rows (``pack_rows``) and the packed-gather SpMM.

Round trip: the packed buffer is decoded here, on the host, from the
documented layout (csrc/spmm_packed.hip) and must give back ``x`` bit for
bit; rows with more than F/2 non-zero bit patterns must be flagged as
overflow rows instead.

SpMM: the packed kernel does the same arithmetic as ``spmm_csr_kernel`` in
the same order (only the fetch of a gathered value differs), so its result
must be ``torch.equal`` to the dense kernel's on the same view."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

FEATS = [256, 104, 48, 8]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _special_rows(F, gen):
    """Rows the layout has to get right, first and last row of the buffer
    included. Returns (x, expected overflow flag per row)."""
    half = F // 2
    rows, ovf = [], []

    def add(r, o):
        rows.append(r)
        ovf.append(o)

    def with_nnz(k, where=None):
        r = torch.zeros(F)
        pos = torch.randperm(F, generator=gen)[:k] if where is None else where
        r[pos] = torch.randn(len(pos), generator=gen) + 3.0
        return r

    add(torch.zeros(F), False)                       # first row: all zero
    add(with_nnz(half), False)                       # exactly F/2: packed
    add(with_nnz(half + 1), True)                    # F/2 + 1: overflow
    add(torch.randn(F, generator=gen) + 5.0, True)   # fully dense
    r = torch.zeros(F)                               # non-zero bit patterns
    r[0], r[1], r[3] = -0.0, 1e-40, -1.5             # (3 and 2 <= F/2 kept)
    add(r, False)
    r = torch.zeros(F)
    r[F // 2], r[F - 1] = float('nan'), float('inf')
    add(r, False)
    for _ in range(6):                               # ~25 % dense
        r = torch.randn(F, generator=gen)
        r[torch.rand(F, generator=gen) >= 0.25] = 0.0
        add(r, int((_i32(r) != 0).sum()) > half)
    add(with_nnz(half, torch.arange(F - half, F)), False)   # run ends at F
    # last row: the run fills the capacity and the trailing groups are
    # empty, so their window starts at the end of the value capacity
    add(with_nnz(half, torch.arange(half)), False)
    x = torch.stack(rows)
    assert int((_i32(x[4]) != 0).sum()) == 3         # -0.0 and 1e-40 count
    return x, ovf


def _decode(buf, n, F, meta, stride):
    """Plain decoder of the packed layout: (decoded rows, overflow flags).
    An overflow row decodes to None."""
    G = F // 4
    raw = buf.cpu()
    out, flags = [], []
    for r in range(n):
        row = raw[r * stride:(r + 1) * stride]
        words = row[:2 * G].view(torch.int16).to(torch.int32) & 0xFFFF
        o = ((words >> 15) & 1).tolist()
        assert len(set(o)) == 1, 'overflow bit differs inside a row'
        flags.append(bool(o[0]))
        if o[0]:
            out.append(None)
            continue
        vals = row[meta:meta + 2 * F].view(torch.int32)
        dec = torch.zeros(F, dtype=torch.int32)
        run = 0
        for g in range(G):
            off, mask = int(words[g]) & 0xFF, (int(words[g]) >> 8) & 0xF
            assert off == run, 'offset is not the count of values before'
            assert (int(words[g]) >> 12) & 0x7 == 0
            for k in range(4):
                if mask >> k & 1:
                    dec[4 * g + k] = vals[run]
                    run += 1
        assert run <= F // 2
        out.append(dec)
    return out, flags


@pytest.mark.parametrize('F', FEATS)
def test_pack_round_trip(F):
    from adaqp_amd.ops.kernels import native, pack_rows
    native()
    gen = torch.Generator().manual_seed(11 + F)
    x, want_ovf = _special_rows(F, gen)
    p = pack_rows(x.cuda())
    assert p is not None and p.rows == x.shape[0] and p.feats == F
    G = F // 4
    assert p.meta_bytes == (2 * G + 15) // 16 * 16
    assert p.stride == (p.meta_bytes + 2 * F + 127) // 128 * 128
    assert p.buf.dtype == torch.uint8 and p.buf.data_ptr() % 128 == 0
    assert p.buf.numel() == x.shape[0] * p.stride + 16
    if F == 256:
        assert (p.meta_bytes, p.stride) == (128, 640)
    dec, flags = _decode(p.buf, x.shape[0], F, p.meta_bytes, p.stride)
    assert flags == want_ovf
    xi = _i32(x)
    for r, d in enumerate(dec):
        if d is not None:
            assert torch.equal(d, xi[r]), f'row {r}'


# ---------------------------------------------------------------------------
# SpMM
# ---------------------------------------------------------------------------
R, NL, NR = 40, 150, 90
HUB = 700                                   # > SEG_EDGES: split segments


@functools.lru_cache(maxsize=None)
def _graph(remote):
    gen = torch.Generator().manual_seed(31 + remote)
    degs = [0] + list(range(1, 10)) + [0, HUB]
    degs += torch.randint(0, 12, (R - len(degs),), generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    ncols = NL + NR if remote else NL
    indices = torch.randint(0, ncols, (int(indptr[-1]),), generator=gen)
    if remote:
        assert (indices >= NL).any() and (indices < NL).any()
    # negative scales too: products with an absent (+0.0) value are -0.0
    src = torch.rand(NL + NR, generator=gen) - 0.4
    dst = torch.rand(R, generator=gen) + 0.5
    return indptr, indices, src, dst


@functools.lru_cache(maxsize=None)
def _xs(F, density):
    gen = torch.Generator().manual_seed(int(1000 * density) + F)
    xl = torch.randn(NL, F, generator=gen)
    xl[torch.rand(NL, F, generator=gen) >= density] = 0.0
    xr = torch.randn(NR, F, generator=gen)           # remote: read dense
    return xl, xr


@functools.lru_cache(maxsize=None)
def _view(remote):
    from adaqp_amd.ops.kernels import SpmmView, native
    native()
    indptr, indices, _, _ = _graph(remote)
    view = SpmmView(indptr.cuda(), indices.cuda(), 0, R).to('cuda')
    assert view.n_part > 0 and view.zero_rows.numel() > 0
    return view


@pytest.mark.parametrize('density', [0.0, 0.25, 0.5, 1.0])
@pytest.mark.parametrize('F', [256, 104, 8])
def test_packed_spmm_equals_dense(F, density):
    from adaqp_amd.ops.kernels import pack_rows, spmm
    xl, xr = (t.cuda() for t in _xs(F, density))
    p = pack_rows(xl)
    nnz = (_i32(xl) != 0).sum(1)
    if F == 256 and density == 0.5:                  # a mix of both kinds
        assert (nnz > F // 2).any() and (nnz <= F // 2).any()
    gen = torch.Generator().manual_seed(3)
    addend = torch.randn(R, F, generator=gen).cuda()
    for remote, ss, ds, ad in itertools.product([False, True], repeat=4):
        _, _, src, dst = _graph(remote)
        view = _view(remote)
        kw = dict(x_remote=xr if remote else None,
                  src_scale=src.cuda() if ss else None,
                  dst_scale=dst.cuda() if ds else None)
        a = addend if ad else None
        dense = spmm(view, xl, addend=a, **kw)
        for depth in (4, 8):
            out = torch.full((R, F), float('nan'), device='cuda')
            got = spmm(view, xl, addend=a, out=out, packed=p,
                       packed_depth=depth, **kw)
            assert torch.equal(_i32(got), _i32(dense)), \
                (remote, ss, ds, ad, depth)


def test_unqualified_inputs_take_the_dense_path():
    """F = 6 and bf16 cannot be packed: ``pack_rows`` gives no handle and
    the public ``spmm`` runs the dense kernel."""
    from adaqp_amd.ops.kernels import pack_rows, packable, spmm
    view = _view(False)
    _, _, src, dst = _graph(False)
    gen = torch.Generator().manual_seed(9)
    for F, dtype in ((6, torch.float32), (256, torch.bfloat16)):
        x = torch.randn(NL, F, generator=gen)
        x[torch.rand(NL, F, generator=gen) >= 0.25] = 0.0
        x = x.to(dtype).cuda()
        assert not packable(x) and pack_rows(x) is None
        y0 = spmm(view, x, None, src.cuda(), dst.cuda())
        y1 = spmm(view, x, None, src.cuda(), dst.cuda(), packed=pack_rows(x))
        assert y1.dtype == dtype and torch.equal(y0, y1)
    assert pack_rows(torch.zeros(4, 8)) is None      # CPU tensor
