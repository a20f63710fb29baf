"""Float64 oracles and exact checkers for the HIP kernels (no GPU code).

Every checker takes the kernel's output as CPU tensors, recomputes the
operation in float64 from the exact inputs and raises ``AssertionError``
naming the first offending index. No tolerance is sized from a kernel's
output: each bound counts the fp32 roundings the kernel performs
(2^-24 relative each, half an fp32 ulp) plus half a bf16 ulp of the
result's binade where the result is stored as bf16.

The input builders at the bottom are shared by the CPU tests of the
checkers (``test_kernel_oracles.py``) and the GPU tests
(``test_kernels_exact_gpu.py``) so both run the same shapes.

Known untested corner: rows whose range is below about 1e-36, where the
bf16 wire scale (2^bits - 1)/range overflows to inf. Inf/NaN inputs are
not covered either.
"""
from __future__ import annotations

import functools
from typing import Optional

import torch
from torch import Tensor

from adaqp_amd.ops import quant as Q
from adaqp_amd.ops.kernels import SEG_EDGES

U32 = 2.0 ** -24          # one fp32 rounding, relative (half an ulp)


def bf16_half_ulp(v: Tensor) -> Tensor:
    """Half a bf16 ulp at magnitude |v| (float64): 2^(e - 8) for
    2^e <= |v| < 2^(e+1), since bf16 keeps 8 significand bits. Relative to
    |v| that is between 2^-9 and 2^-8, so a flat 2^-9 * |v| would refuse
    correctly rounded results in the lower half of every binade. 0 at 0;
    bf16 subnormals are not modelled."""
    a = v.abs()
    _, e = torch.frexp(a)                     # a = m * 2^e, m in [0.5, 1)
    h = torch.ldexp(torch.ones_like(a), e - 9)
    return torch.where(a > 0, h, torch.zeros_like(a))


def _first(mask: Tensor):
    return tuple(torch.nonzero(mask)[0].tolist())


def _bits16(t: Tensor) -> Tensor:
    assert t.dtype == torch.bfloat16, t.dtype
    return t.contiguous().view(torch.int16)


def unpack_levels(payload: Tensor, bits: int) -> Tensor:
    """uint8 [n, bpn] -> int64 levels [n, bpn * (8 // bits)], pad included."""
    vpb = 8 // bits
    shifts = torch.arange(vpb, dtype=torch.int64) * bits
    b = payload.to(torch.int64)[:, :, None]
    return ((b >> shifts) & (2 ** bits - 1)).reshape(payload.shape[0], -1)


def pack_levels(levels: Tensor, bits: int) -> Tensor:
    """Inverse of unpack_levels (levels already padded to whole bytes)."""
    vpb = 8 // bits
    shifts = torch.arange(vpb, dtype=torch.int64) * bits
    q = levels.reshape(levels.shape[0], -1, vpb)
    return (q << shifts).sum(dim=2).to(torch.uint8)


# --------------------------------------------------------------------------
# quant_pack
# --------------------------------------------------------------------------

def pack_delta(bits: int) -> float:
    """Half-width of the band around an integer w inside which fp32 may
    land on the other side. The fp32 evaluation of (x - rmin)*scale + u
    has three roundings (sub, mul, add; or sub plus one fma), each at most
    2^-24 relative on a value of magnitude at most L + 2; the factor 4
    leaves a margin of one extra rounding."""
    return 4 * U32 * (2 ** bits - 1 + 2)


def packed_reference(x_rows_f32: Tensor, bits: int, seed: int, tag: Tensor):
    """Float64 oracle of the stochastic rounding. Returns (q64, lo, hi, w):
    q64 = clamp(floor(w), 0, L); lo/hi = the same with w shifted by -/+
    delta, so lo == hi == q64 except within delta of a rounding boundary,
    where the neighbouring level on that side is admissible too."""
    x = x_rows_f32
    assert x.dtype == torch.float32 and x.dim() == 2
    L = 2 ** bits - 1
    scale, rmin = Q.qparams(x, bits)
    s = scale.double()[:, None]
    r = rmin.double()[:, None]
    u = Q.uniform_noise(seed, tag, x.shape[1]).double()
    w = (x.double() - r) * s + u
    d = pack_delta(bits)
    live = (s > 0).expand_as(w)
    zero = torch.zeros_like(w)

    def lvl(v):
        return torch.where(live, torch.floor(v).clamp(0, L), zero).to(torch.int64)
    return lvl(w), lvl(w - d), lvl(w + d), w


def check_packed(x_rows_f32: Tensor, bits: int, seed: int, tag: Tensor,
                 payload: Tensor, scale_bf16: Tensor, rmin_bf16: Tensor) -> None:
    """payload uint8 [n, bytes_per_node] (node i quantizes x_rows_f32[i] with
    RNG tag tag[i]); scale/rmin bf16 [n] as written to the wire."""
    x = x_rows_f32
    n, F = x.shape
    bpn = Q.bytes_per_node(F, bits)
    payload = payload.reshape(n, bpn)
    es, er = Q.qparams(x, bits)
    for name, got, exp in (('scale', scale_bf16, es), ('rmin', rmin_bf16, er)):
        bad = _bits16(got) != _bits16(exp)
        if bad.any():
            i = _first(bad)[0]
            raise AssertionError(
                f'{name}[{i}] = {float(got[i])!r} differs from qparams '
                f'{float(exp[i])!r} (bits={bits}, F={F})')
    lv = unpack_levels(payload, bits)
    pad = lv[:, F:] != 0
    if pad.any():
        i, j = _first(pad)
        raise AssertionError(
            f'pad bits set: node {i} pad level {j} = {int(lv[i, F + j])} '
            f'(bits={bits}, F={F})')
    q = lv[:, :F]
    q64, lo, hi, w = packed_reference(x, bits, seed, tag)
    bad = (q != lo) & (q != hi)
    if bad.any():
        i, f = _first(bad)
        raise AssertionError(
            f'level[{i}, {f}] = {int(q[i, f])}, oracle {int(q64[i, f])} '
            f'(admissible {int(lo[i, f])}..{int(hi[i, f])}, w = '
            f'{float(w[i, f])!r}, delta = {pack_delta(bits):.3e}, bits={bits}, '
            f'F={F}); {int(bad.sum())} bad of {q.numel()}')


# --------------------------------------------------------------------------
# quant_unpack
# --------------------------------------------------------------------------

def check_unpacked(payload: Tensor, bits: int, scale: Tensor, rmin: Tensor,
                   F: int, out: Tensor) -> None:
    """out [n, F] fp32 or bf16: the rows the kernel wrote for payload
    [n, bytes_per_node], in payload order."""
    n = payload.shape[0]
    payload = payload.reshape(n, Q.bytes_per_node(F, bits))
    assert out.shape == (n, F), (out.shape, n, F)
    q = unpack_levels(payload, bits)[:, :F].double()
    s32 = scale.float()
    inv = torch.where(s32 > 0, 1.0 / s32, torch.zeros_like(s32))   # fp32 divide
    qi = q * inv.double()[:, None]
    r = rmin.double()[:, None]
    ref = qi + r
    # one rounding each for the product and the sum (or one for the fma)
    tol = 2 * U32 * (qi.abs() + r.abs())
    if out.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(ref.abs() + tol)
    else:
        assert out.dtype == torch.float32, out.dtype
    o = out.double()
    const = (s32 <= 0)[:, None].expand_as(o)
    bad = torch.where(const, o != r, ~((o - ref).abs() <= tol))
    if bad.any():
        i, f = _first(bad)
        raise AssertionError(
            f'out[{i}, {f}] = {float(o[i, f])!r}, oracle {float(ref[i, f])!r} '
            f'(tol {float(tol[i, f]):.3e}, level {int(q[i, f])}, scale '
            f'{float(s32[i])!r}, bits={bits}, F={F}, {out.dtype}); '
            f'{int(bad.sum())} bad of {o.numel()}')


# --------------------------------------------------------------------------
# spmm_csr
# --------------------------------------------------------------------------

def segs_per_row(view) -> Tensor:
    """Number of work-item segments an SpmmView gives each row."""
    return torch.bincount(view.seg_row.cpu().to(torch.int64),
                          minlength=view.nrows)


def spmm_reference(indptr: Tensor, indices: Tensor, x_all: Tensor,
                   src: Optional[Tensor], dst: Optional[Tensor]):
    """(ref, S, deg) in float64: ref = dst * (A @ (src * x)),
    S = |dst| * (A @ |src * x|). A counts duplicate edges."""
    indptr = indptr.cpu().to(torch.int64)
    indices = indices.cpu().to(torch.int64)
    R = indptr.numel() - 1
    xs = x_all.cpu().double()
    if src is not None:
        xs = xs * src.cpu().double()[:xs.shape[0], None]
    A = torch.sparse_csr_tensor(indptr, indices,
                                torch.ones(indices.numel(), dtype=torch.float64),
                                size=(R, xs.shape[0]))
    ref = torch.sparse.mm(A, xs)
    S = torch.sparse.mm(A, xs.abs())
    if dst is not None:
        d = dst.cpu().double()[:, None]
        ref = ref * d
        S = S * d.abs()
    return ref, S, indptr[1:] - indptr[:-1]


def check_spmm(indptr: Tensor, indices: Tensor, x_all: Tensor,
               src: Optional[Tensor], dst: Optional[Tensor], y: Tensor,
               n_segs_per_row: Optional[Tensor] = None) -> None:
    """x_all = cat(x_local, x_remote) exactly as the kernel read it (bf16 is
    upcast); y [R, F] in x's dtype. Roundings per output: one per edge
    (fma), one per segment in the partial combine, one for acc0 + acc1 and
    one for the dst scale, each relative to at most S."""
    ref, S, deg = spmm_reference(indptr, indices, x_all, src, dst)
    R = deg.numel()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    segs = (torch.ones(R, dtype=torch.int64) if n_segs_per_row is None
            else n_segs_per_row.cpu().to(torch.int64))
    tol = (deg + segs + 2).double()[:, None] * U32 * S
    if y.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(ref.abs() + tol)
    else:
        assert y.dtype == torch.float32, y.dtype
    o = y.cpu().double()
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        r, f = _first(bad)
        raise AssertionError(
            f'y[{r}, {f}] = {float(o[r, f])!r}, oracle {float(ref[r, f])!r} '
            f'(tol {float(tol[r, f]):.3e}, deg {int(deg[r])}, segs '
            f'{int(segs[r])}, {y.dtype}); {int(bad.sum())} bad of {o.numel()} '
            f'in {int(bad.any(dim=1).sum())} rows')


# --------------------------------------------------------------------------
# fused_dual_gemm_bf16
# --------------------------------------------------------------------------

def check_dual_gemm(a1: Tensor, a2: Tensor, w1: Tensor, w2: Tensor,
                    bias: Optional[Tensor], out: Tensor) -> None:
    """out = a1 @ w1 + a2 @ w2 + bias; w1 [K1, N], w2 [K2, N], bf16 out."""
    a1, a2, w1, w2 = (t.cpu().double() for t in (a1, a2, w1, w2))
    N = w1.shape[1]
    b = (bias.cpu().double() if bias is not None and bias.numel()
         else torch.zeros(N, dtype=torch.float64))
    ref = a1 @ w1 + a2 @ w2 + b
    S = a1.abs() @ w1.abs() + a2.abs() @ w2.abs() + b.abs()
    tol = (a1.shape[1] + a2.shape[1] + 2) * U32 * S
    tol = tol + bf16_half_ulp(ref.abs() + tol)
    o = out.cpu().double()
    assert o.shape == ref.shape, (o.shape, ref.shape)
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        i, j = _first(bad)
        raise AssertionError(
            f'out[{i}, {j}] = {float(o[i, j])!r}, oracle {float(ref[i, j])!r} '
            f'(tol {float(tol[i, j]):.3e}, M={a1.shape[0]}, K1={a1.shape[1]}, '
            f'K2={a2.shape[1]}, N={N}); {int(bad.sum())} bad of {o.numel()}')


# --------------------------------------------------------------------------
# shared inputs (CPU tensors, fixed generators)
# --------------------------------------------------------------------------

PACK_FS = (1, 17, 100, 602, 1024, 1025, 1030, 2051)
PACK_SEEDS = (1234, 2 ** 32 + 5)
PACK_N, PACK_ROWS, PACK_POS0, PACK_BASE = 80, 37, 11, 3
PAYLOAD_FILL = 0xA5
PARAMS_FILL = -7.0
CONST_NODE, INEXACT_NODE = 3, 5


def quant_input(N: int, F: int, gen: torch.Generator) -> Tensor:
    """fp32 [N, F] with per-row scale 10^(i mod 5 - 2) and offset i mod 3."""
    i = torch.arange(N)
    x = torch.randn(N, F, generator=gen)
    return x * (10.0 ** ((i % 5) - 2).double()).float()[:, None] \
        + (i % 3).float()[:, None]


class PackCase:
    """n = 37 rows gathered by a permutation from N = 80; pos a permutation
    of [POS0, POS0 + n); node offsets pos_rank * bpn + 3 (odd base)."""

    def __init__(self, F: int, bits: int, dtype=torch.float32):
        gen = torch.Generator().manual_seed(1000 + F)
        n = PACK_ROWS
        x = quant_input(PACK_N, F, gen)
        self.rows = torch.randperm(PACK_N, generator=gen)[:n]
        x[self.rows[CONST_NODE]] = 0.75                 # constant row
        if F > 1:      # row minimum not representable in bf16
            x[self.rows[INEXACT_NODE], F // 2] = -(1.0 + 2.0 ** -12) * 1000.0
        self.x = x.to(dtype)
        self.x_rows = self.x[self.rows].float()         # what the kernel reads
        self.F, self.bits, self.n = F, bits, n
        self.bpn = Q.bytes_per_node(F, bits)
        self.pos_rank = torch.randperm(n, generator=gen)
        self.pos = self.pos_rank + PACK_POS0
        self.off = self.pos_rank * self.bpn + PACK_BASE
        self.payload_len = PACK_BASE + n * self.bpn + 5
        self.n_slots = PACK_POS0 + n + 4

    def node_payload(self, payload: Tensor) -> Tensor:
        """flat wire payload -> [n, bpn] in node order."""
        idx = self.off[:, None] + torch.arange(self.bpn)
        return payload[idx.reshape(-1)].reshape(self.n, self.bpn)

    def node_params(self, params: Tensor):
        return params[2 * self.pos], params[2 * self.pos + 1]

    def check_untouched(self, payload: Tensor, params: Tensor) -> None:
        used = torch.zeros(self.payload_len, dtype=torch.bool)
        used[PACK_BASE:PACK_BASE + self.n * self.bpn] = True
        assert (payload[~used] == PAYLOAD_FILL).all(), \
            'payload written outside the nodes\' byte runs'
        free = torch.ones(2 * self.n_slots, dtype=torch.bool)
        free[2 * self.pos] = False
        free[2 * self.pos + 1] = False
        assert (params[free].float() == PARAMS_FILL).all(), \
            'params written outside the slots in pos'


def mixed_plans(F: int):
    """Send/recv SidePlans for 3 peers (the middle one empty), ~60 nodes,
    random bits over {2,4,8}. Returns (x [100, F], send, recv, n_out_rows):
    recv scatters into a permutation of a larger remote block."""
    from adaqp_amd.comm.buffers import _layout
    gen = torch.Generator().manual_seed(2000 + F)
    x = quant_input(100, F, gen)
    counts = [33, 0, 28]
    choices = torch.tensor([2, 4, 8])
    bits_l, send_rows, recv_rows = [], [], []
    total = sum(counts)
    n_out = total + 9
    out_perm = torch.randperm(n_out, generator=gen)
    base = 0
    for k in counts:
        if k == 0:
            bits_l.append(None); send_rows.append(None); recv_rows.append(None)
            continue
        bits_l.append(choices[torch.randint(0, 3, (k,), generator=gen)])
        send_rows.append(torch.randperm(100, generator=gen)[:k])
        recv_rows.append(out_perm[base:base + k])
        base += k
    return x, _layout(bits_l, send_rows, F), _layout(bits_l, recv_rows, F), n_out


def plan_payload(payload: Tensor, plan, b: int) -> Tensor:
    bpn = Q.bytes_per_node(plan.F, b)
    idx = plan.off[b][:, None] + torch.arange(bpn)
    return payload[idx.reshape(-1)].reshape(-1, bpn)


GS_R, GS_NL, GS_NR = 66000, 600, 400
GS_HUBS = {10: 3 * SEG_EDGES + 17, 65900: SEG_EDGES + 1, 65901: 0}


@functools.lru_cache(maxsize=None)
def grid_stride_graph():
    """66 000 rows of degree 0-3 over 1000 sources, two hubs, one forced
    empty row. Returns (indptr, indices, src, dst) — do not modify."""
    gen = torch.Generator().manual_seed(21)
    deg = torch.randint(0, 4, (GS_R,), generator=gen)
    for r, d in GS_HUBS.items():
        deg[r] = d
    indptr = torch.zeros(GS_R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.randint(0, GS_NL + GS_NR, (int(indptr[-1]),), generator=gen)
    src = torch.rand(GS_NL + GS_NR, generator=gen) + 0.5
    dst = torch.rand(GS_R, generator=gen) + 0.5
    return indptr, indices, src, dst


@functools.lru_cache(maxsize=None)
def grid_stride_x(F: int, dtype) -> Tensor:
    gen = torch.Generator().manual_seed(22 + F)
    return torch.randn(GS_NL + GS_NR, F, generator=gen).to(dtype)


SR_R, SR_NL, SR_NR = 70, 180, 120
SR_HUBS = (0, 2, 3)            # rows longer than SEG_EDGES
# (dtype, F): bf16 needs an even F, so 17 is fp32 only
SR_CASES = [(dt, F) for dt in (torch.float32, torch.bfloat16)
            for F in (136, 6, 17, 602) if not (dt == torch.bfloat16 and F % 2)]


@functools.lru_cache(maxsize=None)
def split_rows_graph():
    """The degrees of test_spmm_split_rows_bit_reproducible over N = 300
    sources split 180 local / 120 remote. Returns (indptr, indices, src,
    dst) — do not modify."""
    gen = torch.Generator().manual_seed(11)
    R = SR_R
    degs = [3 * SEG_EDGES + 17, 0, 2 * SEG_EDGES, SEG_EDGES + 1, SEG_EDGES] + \
        torch.randint(1, 9, (R - 5,), generator=gen).tolist()
    indptr = torch.zeros(R + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.randint(0, SR_NL + SR_NR, (int(indptr[-1]),), generator=gen)
    for r in SR_HUBS:          # hub rows hold local and remote columns
        c = indices[indptr[r]:indptr[r + 1]]
        assert (c < SR_NL).any() and (c >= SR_NL).any()
    src = torch.rand(SR_NL + SR_NR, generator=gen) + 0.5
    dst = torch.rand(R, generator=gen) + 0.5
    return indptr, indices, src, dst


@functools.lru_cache(maxsize=None)
def split_rows_x(F: int, dtype) -> Tensor:
    gen = torch.Generator().manual_seed(33 + F)
    return torch.randn(SR_NL + SR_NR, F, generator=gen).to(dtype)


GEMM_SHAPES = ((77, 40, 72, 16), (130, 72, 8, 48), (64, 136, 64, 256),
               (1, 8, 8, 16))


def gemm_case(M: int, K1: int, K2: int, N: int):
    gen = torch.Generator().manual_seed(M * 1000 + K1)
    mk = lambda *s: torch.randn(*s, generator=gen).bfloat16()
    return mk(M, K1), mk(M, K2), mk(K1, N), mk(K2, N), mk(N)
