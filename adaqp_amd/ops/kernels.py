"""Device dispatch for the hot ops.

GPU (MI355X): hand-written CDNA4 HIP kernels from ``adaqp_amd/csrc``
(built in-tree as ``adaqp_amd._C``). The GPU path REFUSES to fall back —
if the extension is missing on a CUDA device, that is a build error, not
a reason to silently run eager PyTorch.

CPU: torch reference implementations (bit-exact for quant pack/unpack —
same hash RNG) used by unit tests and the CPU/gloo plumbing config.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import quant as Q
from ..comm.buffers import SidePlan, BITS_SET, bytes_per_node

_native = None
_native_err: Optional[Exception] = None


def native():
    global _native, _native_err
    if _native is None and _native_err is None:
        try:
            from .. import _C  # in-tree HIP extension
            _native = _C
        except Exception as e:   # pragma: no cover
            _native_err = e
    if _native is None:
        raise RuntimeError(
            f'adaqp_amd._C HIP extension not built (run `python setup.py '
            f'build_ext --inplace`): {_native_err}')
    return _native


def has_native() -> bool:
    try:
        native()
        return True
    except RuntimeError:
        return False


# --------------------------------------------------------------------------
# mixed-bit quantize / dequantize
# --------------------------------------------------------------------------

def mixed_quantize(x: Tensor, plan: SidePlan, seed: int) -> Tuple[Tensor, Tensor]:
    """Gather plan.rows from x, quantize per bit group, pack into the wire
    payload + params described by plan. Returns (uint8 [B], bf16 [2S])."""
    if x.is_cuda:
        payload = torch.empty(plan.total_bytes, dtype=torch.uint8, device=x.device)
        params = torch.empty(2 * plan.total_nodes, dtype=torch.bfloat16, device=x.device)
        for b in BITS_SET:
            rows = plan.rows[b]
            if rows.numel():
                native().quant_pack(x, rows, plan.pos[b], plan.off[b], b,
                                    seed, payload, params)
        return payload, params
    payload = torch.zeros(plan.total_bytes, dtype=torch.uint8)
    params = torch.zeros(2 * plan.total_nodes, dtype=torch.bfloat16)
    for b in BITS_SET:
        rows, pos, off = plan.rows[b], plan.pos[b], plan.off[b]
        if rows.numel() == 0:
            continue
        pl, scale, rmin = Q.pack_torch(x[rows].float(), b, seed, node_tag=pos)
        bpn = pl.shape[1]
        idx = off[:, None] + torch.arange(bpn, dtype=torch.int64)
        payload[idx.reshape(-1)] = pl.reshape(-1)
        params[2 * pos] = scale
        params[2 * pos + 1] = rmin
    return payload, params


def trace_rows(send: Tensor) -> Tensor:
    """fp32 [S]: the quantization-variance proxy (F/6) * (rmax - rmin)^2 of
    each row of ``send`` [S, F] (``GraphEngine.trace`` accumulates it): the
    range is subtracted in send's dtype, squared and scaled in fp32."""
    rng = send.max(dim=1).values - send.min(dim=1).values
    return (send.shape[1] / 6.0) * rng.float() ** 2


def quant_mixed_fast(x: Tensor, plan: SidePlan) -> bool:
    """True if :func:`mixed_quantize_fused` runs the one-launch kernel
    (csrc/quant_mixed.hip) for this input: a GPU, contiguous fp32 or bf16
    [N, F] tensor with F % 4 == 0, F <= 1024 and rows aligned to the kernel's
    4-feature loads, and a send-slot table in the plan. Everything else takes
    the per-bit path."""
    return (x.is_cuda and x.dim() == 2 and x.is_contiguous()
            and x.dtype in (torch.float32, torch.bfloat16)
            and native().quant_mixed_ok(x.shape[1])
            and x.data_ptr() % (4 * x.element_size()) == 0
            and plan.send_tab is not None and plan.send_tab.is_cuda)


def mixed_quantize_fused(x: Tensor, plan: SidePlan, seed: int,
                         trace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """:func:`mixed_quantize` in one launch for every bit width, same
    (payload, params) bit for bit; no launch for an empty send set.
    ``trace``: fp32 [S] accumulator indexed by send slot (the plan must have
    been built with its send-slot rows); ``trace[s] += trace_rows(x[send
    rows])[s]``, computed in the same kernel. Inputs that do not qualify
    (:func:`quant_mixed_fast`) run :func:`mixed_quantize` and, with ``trace``,
    the torch formula."""
    assert plan.F == x.shape[1]
    if trace is not None:
        assert plan.send_rows is not None, \
            'the plan was built without its send-slot rows'
        assert (trace.dtype == torch.float32 and trace.is_contiguous()
                and trace.shape == (plan.total_nodes,)
                and trace.device == x.device)
    if not quant_mixed_fast(x, plan):
        if trace is not None and plan.total_nodes:
            with torch.no_grad():
                trace += trace_rows(x.index_select(0, plan.send_rows))
        return mixed_quantize(x, plan, seed)
    payload = torch.empty(plan.total_bytes, dtype=torch.uint8, device=x.device)
    params = torch.empty(2 * plan.total_nodes, dtype=torch.bfloat16,
                         device=x.device)
    if plan.total_nodes:
        assert (plan.send_tab.shape[0] == plan.total_nodes
                and plan.send_max_row < x.shape[0]), \
            'the send plan names a row past x'
        native().quant_pack_mixed(
            x, plan.send_tab, int(seed) & Q._M32, payload, params,
            trace if trace is not None
            else torch.empty(0, dtype=torch.float32, device=x.device))
    return payload, params


def resolve_fused_quant(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_FUSED_QUANT=1``; an explicit bool wins.
    (``GraphEngine.fused_quant`` is the flag; ops/dist_agg.py resolves it at
    every quantized exchange.)"""
    if flag is None:
        return _os.environ.get('ADAQP_FUSED_QUANT') == '1'
    return bool(flag)


def mixed_dequantize(payload: Tensor, params: Tensor, plan: SidePlan,
                     out: Tensor) -> Tensor:
    """Unpack wire payload into fp rows of ``out`` (remote block [R, F]),
    fused with the scatter to plan.rows."""
    if payload.is_cuda:
        for b in BITS_SET:
            rows = plan.rows[b]
            if rows.numel():
                native().quant_unpack(payload, params, rows, plan.pos[b],
                                      plan.off[b], b, plan.F, out)
        return out
    for b in BITS_SET:
        rows, pos, off = plan.rows[b], plan.pos[b], plan.off[b]
        if rows.numel() == 0:
            continue
        bpn = bytes_per_node(plan.F, b)
        idx = off[:, None] + torch.arange(bpn, dtype=torch.int64)
        pl = payload[idx.reshape(-1)].reshape(-1, bpn)
        scale = params[2 * pos].clone()
        rmin = params[2 * pos + 1].clone()
        out[rows] = Q.unpack_torch(pl, b, scale, rmin, plan.F).to(out.dtype)
    return out


# --------------------------------------------------------------------------
# CSR SpMM:  y[r] = dst_scale[r] * sum_{c in row r} src_scale[c] * x[c]
# --------------------------------------------------------------------------

_csr_cache: dict = {}

import os as _os
# max edges one sub-wavefront processes serially. 256 measured best on
# the flagship shape in a same-box sweep (128/192/256 flat, 512/1024
# slower); cross-box deltas on other datasets are within run-to-run
# noise (profiles/r02_NOTES.md). ADAQP_SEG_EDGES overrides.
SEG_EDGES = int(_os.environ.get('ADAQP_SEG_EDGES', '256'))
# SW == 64 SpMM (one wavefront per segment: fp32 F > 128, bf16 F > 256):
# False = the per-lane index kernel, True = the wave-uniform index kernel.
# Both give the same bits; the wave-uniform one measured no faster (the
# gather runs at the memory system's rate: profiles/spmm_scalar_NOTES.md),
# so it stays behind this switch. ADAQP_SPMM_WAVE_INDEX=1 turns it on
# (read once, here).
WAVE_INDEX = _os.environ.get('ADAQP_SPMM_WAVE_INDEX', '0') == '1'
# row fetches in flight per lane in the packed-gather SpMM (4 or 8)
PACKED_DEPTH = int(_os.environ.get('ADAQP_SPMM_PACKED_DEPTH', '4'))
# how the dense per-lane, fp32 packed and row-skipping SpMM kernels hand out
# segments: 0 = static swizzle plus grid stride, 1 = ordered sweep (a grid of
# the resident blocks; every wavefront takes tickets of SPMM_CHUNK segments
# from one counter, so the whole GPU walks the rows front to back once).
# Same bits either way. ADAQP_SPMM_ORDER / ADAQP_SPMM_CHUNK, read once, here;
# the measurement behind the defaults is profiles/spmm_order_NOTES.md.
SPMM_ORDER = int(_os.environ.get('ADAQP_SPMM_ORDER', '1'))
SPMM_CHUNK = int(_os.environ.get('ADAQP_SPMM_CHUNK', '4'))
# which kernel an fp32 spmm(..., live=) runs: False = spmm_rowskip_kernel
# (walks every edge, predicates the row fetch), True = spmm_compact_kernel
# (one ballot per chunk of edges, fetch slots spent on live edges only). A
# bf16 call with live= always runs the compacting kernel, the only one it
# has. Same bits either way. ADAQP_SPMM_COMPACT=1 turns it on (read once,
# here); profiles/spmm_compact_NOTES.md has the measurement.
SPMM_COMPACT = _os.environ.get('ADAQP_SPMM_COMPACT', '0') == '1'
# what spmm does with a QuantRemote whose gathered rows are bf16 (a bf16 call,
# or the mixed call with out_dtype=torch.float32): False = dequantize it into
# a bf16 block, True = gather from the wire (csrc/spmm_quant_bf16.hip). Same
# bits either way. ADAQP_FUSED_DEQUANT_BF16=1 turns it on (read once, here);
# profiles/spmm_quant_bf16_NOTES.md has the measurement.
QUANT_BF16 = _os.environ.get('ADAQP_FUSED_DEQUANT_BF16', '0') == '1'


def _auto_seg(num_edges: int, num_rows: int) -> int:
    return SEG_EDGES


class SpmmView:
    """One CSR row range + its work-item segmentation.

    Power-law graphs put 10^4-10^5 edges on hub rows; a single
    sub-wavefront grinding one such row serially becomes the kernel's
    critical path. Rows are split into <=SEG_EDGES-edge segments; each
    segment of a row with >1 segment writes its partial sum to its own
    slot (``seg_part``) and a second pass adds a row's slots
    (``part_ptr``, one range per ``zero_rows`` entry) in segment order,
    so results are bit-identical from run to run (SURVEY.md §7 'hard
    parts': row-binning / load imbalance).

    ``col_block`` > 0 additionally PERMUTES the edge array into
    column-block-major order (segments keyed by (col/col_block, row)):
    the grid sweeps one x column block at a time, so the block stays
    LLC-resident while every consumer reads it — same kernel, different
    work-item layout. Costs a partial-sum combine for every row spanning
    >1 block.
    """

    def __init__(self, indptr: Tensor, indices: Tensor, base: int, nrows: int,
                 col_block: int = 0):
        self.indptr = indptr
        self.base = int(base)
        self.nrows = int(nrows)
        # largest column any edge names (-1: no edges); spmm checks it
        # against the rows a quantized remote operand describes
        self.max_col = int(indices.max()) if indices.numel() else -1
        self.col_blocked = col_block > 0 and indices.numel() > 0
        SEG = _auto_seg(int(indices.numel()), nrows)
        indptr_c = indptr.cpu()
        counts = (indptr_c[1:] - indptr_c[:-1])
        if col_block > 0 and indices.numel():
            idx_c = indices.cpu()
            rows_pe = torch.repeat_interleave(
                torch.arange(nrows, dtype=torch.int64), counts)
            cb = idx_c // col_block
            key = cb * nrows + rows_pe
            order = torch.argsort(key, stable=True)
            self.indices = idx_c[order].to(indices.device)
            key = key[order]
            # run starts: key change points, then chunk runs to SEG_EDGES
            change = torch.ones(key.numel(), dtype=torch.bool)
            change[1:] = key[1:] != key[:-1]
            run_start = torch.nonzero(change, as_tuple=True)[0]
            run_end = torch.cat([run_start[1:],
                                 torch.tensor([key.numel()])])
            run_len = run_end - run_start
            nseg = (run_len + SEG - 1) // SEG
            seg_runs = torch.repeat_interleave(
                torch.arange(run_start.numel()), nseg)
            first = torch.repeat_interleave(torch.cumsum(nseg, 0) - nseg, nseg)
            in_run = torch.arange(seg_runs.numel(), dtype=torch.int64) - first
            e0 = run_start[seg_runs] + in_run * SEG
            e1 = torch.minimum(e0 + SEG, run_end[seg_runs])
            seg_row = (key[run_start[seg_runs]] % nrows)
            segs_per_row = torch.bincount(seg_row, minlength=nrows)
            multi_mask = segs_per_row != 1     # incl. empty rows -> zeroed
            self.seg_row = seg_row.to(torch.int32)
            self.seg_e0 = e0
            self.seg_e1 = e1
            self.seg_multi = multi_mask[seg_row].to(torch.uint8)
            self.zero_rows = torch.nonzero(multi_mask, as_tuple=True)[0].to(torch.int32)
        else:
            self.indices = indices
            nseg = torch.clamp((counts + SEG - 1) // SEG, min=1)
            seg_row = torch.repeat_interleave(torch.arange(nrows, dtype=torch.int64), nseg)
            first = torch.repeat_interleave(torch.cumsum(nseg, 0) - nseg, nseg)
            seg_in_row = torch.arange(seg_row.numel(), dtype=torch.int64) - first
            e0 = indptr_c[seg_row] + seg_in_row * SEG
            e1 = torch.minimum(e0 + SEG, indptr_c[seg_row + 1])
            multi_mask = nseg > 1
            self.seg_row = seg_row.to(torch.int32)
            self.seg_e0 = e0
            self.seg_e1 = e1
            self.seg_multi = multi_mask[seg_row].to(torch.uint8)
            self.zero_rows = torch.nonzero(multi_mask, as_tuple=True)[0].to(torch.int32)
        # partial-sum slots: a split row's segments get consecutive slots
        # in segment order; part_ptr[j]:part_ptr[j+1] is zero_rows[j]'s range
        multi_seg = torch.nonzero(self.seg_multi, as_tuple=True)[0]
        multi_row = self.seg_row[multi_seg].to(torch.int64)
        order = torch.argsort(multi_row, stable=True)
        slot = torch.empty_like(order)
        slot[order] = torch.arange(order.numel(), dtype=torch.int64)
        seg_part = torch.full((self.seg_row.numel(),), -1, dtype=torch.int64)
        seg_part[multi_seg] = slot
        cnt = torch.bincount(multi_row, minlength=nrows)[self.zero_rows.to(torch.int64)]
        self.seg_part = seg_part.to(torch.int32)
        self.part_ptr = torch.cat([torch.zeros(1, dtype=torch.int64),
                                   torch.cumsum(cnt, 0)]).to(torch.int32)
        self.n_part = int(multi_seg.numel())
        # int32 column indices + segment bounds: halves the kernel's
        # index-read bytes (~1 GB -> 0.5 GB per pass on full products);
        # node/edge counts are always < 2^31
        self.indices = self.indices.to(torch.int32)
        self.seg_e0 = self.seg_e0.to(torch.int32)
        self.seg_e1 = self.seg_e1.to(torch.int32)
        self._on = None

    def to(self, device):
        # seg_multi stays on the host: only the slot construction reads it
        for n in ('indices', 'seg_row', 'seg_e0', 'seg_e1', 'zero_rows',
                  'seg_part', 'part_ptr'):
            setattr(self, n, getattr(self, n).to(device))
        return self


PACK_MAX_FEATS = 256


def packable(x: Tensor) -> bool:
    """True if ``x`` can be the packed operand of :func:`spmm`: a GPU fp32
    contiguous [N, F] tensor with at least one row, F % 4 == 0 and
    F <= 256. Everything else (bf16, other F, CPU tensors) runs the dense
    SpMM kernel."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.is_contiguous() and x.shape[0] > 0
            and 0 < x.shape[1] <= PACK_MAX_FEATS and x.shape[1] % 4 == 0)


class PackedRows:
    """Packed copy of a sparse [N, F] fp32 tensor (csrc/spmm_packed.hip has
    the layout): per row ``F/4`` 16-bit words (8-bit value offset, 4-bit
    presence mask, bit 15 = overflow row) padded to ``meta_bytes``, then
    up to ``F/2`` kept fp32 values; rows are ``stride`` bytes apart in the
    uint8 buffer ``buf``. Rows with more than F/2 non-zero bit patterns
    are overflow rows and are read from the dense tensor."""

    def __init__(self, buf: Tensor, rows: int, feats: int):
        C = native()
        self.buf, self.rows, self.feats = buf, rows, feats
        self.meta_bytes = int(C.packed_meta_bytes(feats))
        self.stride = int(C.packed_row_stride(feats))

    def matches(self, x: Tensor) -> bool:
        return (packable(x) and x.shape[0] == self.rows
                and x.shape[1] == self.feats and x.device == self.buf.device)


def pack_rows(x: Tensor) -> Optional[PackedRows]:
    """One pass of the native pack kernel over ``x``; ``None`` when ``x``
    does not qualify (see :func:`packable`), which callers pass on to
    :func:`spmm` as "no packed operand"."""
    if not packable(x):
        return None
    return PackedRows(native().pack_rows(x), x.shape[0], x.shape[1])


def packable_bf16(x: Tensor) -> bool:
    """True if ``x`` can be the packed operand of a bf16 :func:`spmm`: a GPU
    bf16 contiguous [N, F] tensor with at least one row, F % 8 == 0 and
    8 <= F <= 256."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.is_contiguous() and x.shape[0] > 0
            and 8 <= x.shape[1] <= PACK_MAX_FEATS and x.shape[1] % 8 == 0)


class PackedRowsBf16:
    """Packed copy of a sparse [N, F] bf16 tensor (csrc/spmm_packed_bf16.hip
    has the layout): per row ``F/8`` 16-bit words (8-bit presence mask,
    8-bit count of kept values before the group; 0xFFFF in every word of an
    overflow row) padded to ``meta_bytes``, then up to ``F/2`` kept bf16 bit
    patterns; rows are ``stride`` bytes apart in the uint8 buffer ``buf``.
    Rows with more than F/2 non-zero bit patterns are overflow rows and are
    read from the dense tensor."""

    def __init__(self, buf: Tensor, rows: int, feats: int):
        C = native()
        self.buf, self.rows, self.feats = buf, rows, feats
        self.meta_bytes = int(C.packed_bf16_meta_bytes(feats))
        self.stride = int(C.packed_bf16_row_stride(feats))

    def matches(self, x: Tensor) -> bool:
        return (packable_bf16(x) and x.shape[0] == self.rows
                and x.shape[1] == self.feats and x.device == self.buf.device)


def pack_rows_bf16(x: Tensor) -> Optional[PackedRowsBf16]:
    """:func:`pack_rows` for bf16: one pass of the native bf16 pack kernel;
    ``None`` when ``x`` does not qualify (see :func:`packable_bf16`)."""
    if not packable_bf16(x):
        return None
    return PackedRowsBf16(native().pack_rows_bf16(x), x.shape[0], x.shape[1])


def resolve_fused_dequant(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_FUSED_DEQUANT=1``; an explicit bool
    wins. (``GraphEngine.fused_dequant`` is the flag; ops/dist_agg.py
    resolves it at every propagation.)"""
    if flag is None:
        return _os.environ.get('ADAQP_FUSED_DEQUANT') == '1'
    return bool(flag)


def resolve_fused_dequant_bf16(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_FUSED_DEQUANT_BF16=1``; an explicit bool
    wins. (``GraphEngine.fused_dequant_bf16`` is the flag; ops/dist_agg.py
    resolves it at every propagation.)"""
    if flag is None:
        return _os.environ.get('ADAQP_FUSED_DEQUANT_BF16') == '1'
    return bool(flag)


def resolve_bwd_gather_bf16(flag: Optional[bool]) -> bool:
    """``None`` -> on iff env ``ADAQP_BWD_GATHER_BF16=1``; an explicit bool
    wins. (``GraphEngine.bwd_gather_bf16`` is the flag; the two backward
    callers of ``ops/dist_agg.py::propagate`` resolve it at every call.)"""
    if flag is None:
        return _os.environ.get('ADAQP_BWD_GATHER_BF16') == '1'
    return bool(flag)


def round_rows_bf16(x: Tensor, seed: int, tag_base: int = 0) -> Tensor:
    """fp32 [N, F] -> bf16 [N, F] with unbiased stochastic rounding. Element
    (row, f) with tag ``t = tag_base + row`` draws (u32 arithmetic)
    ``h = hash_u32(seed ^ (t * 0x9E3779B9) ^ (f * 0x85EBCA6B))``, the integer
    behind ``quant.uniform_noise``, and keeps the top half of ``b + (h >> 16)``
    where ``b`` is its bit pattern: the dropped 16 bits round up with
    probability ``low16 / 2^16``, so ``E[out] = x`` for finite x. Inf and NaN
    keep their top half (NaN with the quiet bit set). GPU: one pass of the
    native kernel (csrc/spmm_mixed.hip); CPU: the same definition in torch
    integer ops, identical bits."""
    assert x.dtype == torch.float32 and x.dim() == 2
    x = x.contiguous()
    if x.is_cuda:
        return native().round_rows_bf16(x, int(seed) & Q._M32,
                                        int(tag_base) & Q._M32)
    N, F = x.shape
    b = x.view(torch.int32).to(torch.int64) & Q._M32
    tag = (torch.arange(N, dtype=torch.int64) + int(tag_base)) & Q._M32
    feat = torch.arange(F, dtype=torch.int64)
    h = Q._hash_u32((int(seed) & Q._M32)
                    ^ ((tag[:, None] * 0x9E3779B9) & Q._M32)
                    ^ ((feat[None, :] * 0x85EBCA6B) & Q._M32))
    special = (b & 0x7F800000) == 0x7F800000
    quiet = torch.where((b & 0x007FFFFF) != 0, 0x0040, 0)
    out = torch.where(special, (b >> 16) | quiet, (b + (h >> 16)) >> 16)
    # two's-complement wrap into int16, then reinterpret as bf16
    out = torch.where(out >= 0x8000, out - 0x10000, out).to(torch.int16)
    return out.view(torch.bfloat16)


def resolve_bwd_skip_zero(flag: Optional[bool], default: str) -> bool:
    """``None`` -> env ``ADAQP_BWD_SKIP_ZERO`` (``default`` when unset) is
    '1'; an explicit bool wins. (``GraphEngine.bwd_skip_zero`` is the flag;
    models/common.py resolves it at every output-layer backward.)"""
    if flag is None:
        return _os.environ.get('ADAQP_BWD_SKIP_ZERO', default) == '1'
    return bool(flag)


def resolve_bwd_skip_zero_bf16(flag: Optional[bool], default: str) -> bool:
    """:func:`resolve_bwd_skip_zero` for bf16 engines: ``None`` -> env
    ``ADAQP_BWD_SKIP_ZERO_BF16`` (``default`` when unset) is '1'; an explicit
    bool wins. (``GraphEngine.bwd_skip_zero_bf16`` is the flag.)"""
    if flag is None:
        return _os.environ.get('ADAQP_BWD_SKIP_ZERO_BF16', default) == '1'
    return bool(flag)


def row_live(x: Tensor) -> Tensor:
    """uint8 [N] for an fp32 or bf16 [N, F] tensor (bf16: even F): 1 where
    the row holds an element of non-zero magnitude, by bit pattern
    (``bits & 0x7fffffff != 0``, bf16 ``bits & 0x7fff != 0``), so denormals,
    NaN and Inf count and -0.0 does not. GPU: one pass of the native kernel
    (csrc/spmm_rowskip.hip, bf16 csrc/spmm_compact.hip); CPU: the same
    definition in torch integer ops. The ``live=`` operand of :func:`spmm`."""
    assert x.dtype in (torch.float32, torch.bfloat16) and x.dim() == 2
    x = x.contiguous()
    if x.dtype == torch.bfloat16:
        assert x.shape[1] % 2 == 0, 'row_live on bf16 needs an even F'
        if x.is_cuda:
            return native().row_live_bf16(x)
        return ((x.view(torch.int16) & 0x7FFF) != 0).any(dim=1).to(torch.uint8)
    if x.is_cuda:
        return native().row_live(x)
    return ((x.view(torch.int32) & 0x7FFFFFFF) != 0).any(dim=1).to(torch.uint8)


class QuantRemote:
    """The remote block of one quantized exchange, left in wire form: the
    received ``payload`` (uint8 [plan.total_bytes]) and ``params`` (bf16
    [2 * plan.total_nodes]) with the recv-side ``plan``. :func:`spmm` takes
    it in place of the dense ``x_remote`` and, for GPU fp32, gathers remote
    columns straight from the payload (csrc/spmm_quant.hip): same result
    bit for bit as with ``dequantize()``'s block, except that a row the
    plan does not cover reads as zero instead of being left unwritten.
    ``rows``: rows of the remote block (default: the plan's table).

    With bf16 local rows and ``spmm(..., quant_bf16=True)`` the bf16 gather
    (csrc/spmm_quant_bf16.hip) does the same against a bf16 block.

    The gather's loads reach up to QUANT_PAD bytes past the wire length,
    so on the GPU the payload has to start 4-byte aligned and have that
    many spare bytes behind it in its storage (``wire_buffer`` allocates
    such a tensor); one that does not is copied into one that does."""

    def __init__(self, payload: Tensor, params: Tensor, plan: SidePlan,
                 F: int, rows: Optional[int] = None):
        assert plan.F == F and payload.dtype == torch.uint8
        assert payload.numel() == plan.total_bytes
        assert params.numel() == 2 * plan.total_nodes
        if rows is None:
            rows = (plan.row_tab.shape[0] if plan.row_tab is not None else
                    max([int(r.max()) + 1 for r in plan.rows.values()
                         if r.numel()], default=0))
        self.params, self.plan, self.F, self.rows = params, plan, F, int(rows)
        if payload.is_cuda and plan.row_tab is not None:
            pad = int(native().QUANT_PAD)
            spare = (payload.untyped_storage().nbytes()
                     - payload.storage_offset() - payload.numel())
            if (not payload.is_contiguous() or payload.data_ptr() % 4
                    or spare < pad):
                buf = self.wire_buffer(payload.numel(), payload.device)
                payload = buf.copy_(payload)
        self.payload = payload
        self._desc: Optional[Tensor] = None

    @staticmethod
    def wire_buffer(nbytes: int, device) -> Tensor:
        """uint8 [nbytes] view of an allocation with the spare bytes the
        gather needs behind it."""
        pad = int(native().QUANT_PAD) if torch.device(device).type == 'cuda' else 0
        return torch.empty(nbytes + pad, dtype=torch.uint8,
                           device=device)[:nbytes]

    def fusable(self, x_local: Tensor) -> bool:
        """True if :func:`spmm` runs the quantized-gather kernel for this
        operand: GPU, fp32, a per-row table in the plan, and at least one
        local and one remote row. Everything else dequantizes."""
        return (x_local.is_cuda and x_local.dtype == torch.float32
                and self.plan.row_tab is not None
                and x_local.shape[0] > 0 and self.rows > 0)

    def fusable_bf16(self, x_local: Tensor) -> bool:
        """True if :func:`spmm` with ``quant_bf16`` on runs the bf16
        quantized-gather kernel for this operand: GPU, bf16, even F, a
        per-row table in the plan, and at least one local and one remote
        row. Everything else dequantizes."""
        return (x_local.is_cuda and x_local.dtype == torch.bfloat16
                and x_local.dim() == 2 and x_local.shape[1] % 2 == 0
                and self.plan.row_tab is not None
                and x_local.shape[0] > 0 and self.rows > 0)

    def descriptors(self) -> Tensor:
        """int32 [rows, 4] {payload byte offset, bits, inv, rmin} per
        remote row, built once on the current stream."""
        if self._desc is None:
            assert self.plan.row_tab.shape[0] == self.rows
            self._desc = native().quant_row_desc(self.plan.row_tab, self.params)
        return self._desc

    def dequantize(self, dtype=torch.float32) -> Tensor:
        out = torch.zeros(self.rows, self.F, dtype=dtype,
                          device=self.payload.device)
        return mixed_dequantize(self.payload, self.params, self.plan, out)

    def record_stream(self, stream) -> None:
        for t in (self.payload, self.params, self._desc):
            if t is not None and t.is_cuda:
                t.record_stream(stream)


def spmm(view: 'SpmmView', x_local: Tensor, x_remote,
         src_scale: Optional[Tensor], dst_scale: Optional[Tensor],
         out: Optional[Tensor] = None, addend: Optional[Tensor] = None,
         wave_index: Optional[bool] = None,
         packed: Union[PackedRows, 'PackedRowsBf16', None] = None,
         packed_depth: Optional[int] = None,
         out_dtype: Optional[torch.dtype] = None,
         live: Optional[Tensor] = None,
         order: Optional[int] = None,
         chunk: Optional[int] = None,
         compact: Optional[bool] = None,
         quant_bf16: Optional[bool] = None) -> Tensor:
    """Aggregation SpMM over an in-edge CSR view.

    Columns < len(x_local) read x_local; the rest read x_remote (the
    all-to-all output block) — no concat on the GPU path.
    src_scale: [n_local+n_remote] or None; dst_scale: [nrows] or None.
    ``out`` (GPU path): write into this [nrows, F] contiguous tensor —
    lets the decomposed path target row slices of ONE output so the
    central/marginal results need no torch.cat afterwards.
    ``addend``: optional [nrows, F] contiguous tensor of y's dtype; the
    result is ``spmm(...) + addend`` bit for bit, added in the kernel's
    epilogue instead of a separate pass.
    ``wave_index``: which SW == 64 kernel runs (None = WAVE_INDEX).
    ``packed``: ``pack_rows(x_local)`` for fp32 or
    ``pack_rows_bf16(x_local)`` for bf16; local columns are then gathered
    from the packed copy (remote columns and overflow rows from the dense
    tensors), same result bit for bit. Ignored on the CPU.
    ``packed_depth``: row fetches in flight per lane in that kernel
    (None = PACKED_DEPTH).
    ``x_remote`` may be a :class:`QuantRemote`. For GPU fp32
    (``QuantRemote.fusable``) the quantized-gather kernel runs and a
    ``packed`` operand is ignored for that call: the two gathers are not
    combined, and the quantized one wins. Otherwise (CPU, bf16) the block
    is dequantized first and the call proceeds as with a tensor: under
    bf16 it is the dense remote operand of a packed call.
    ``out_dtype=torch.float32`` with a bf16 ``x_local`` is the mixed call
    (csrc/spmm_mixed.hip): ``x_remote`` is bf16 (or None, or a QuantRemote,
    which is dequantized into a bf16 block unless ``quant_bf16`` is on),
    ``out`` and ``addend`` are fp32 and ``packed`` must be None. The rows
    are only gathered in bf16;
    the result equals ``spmm`` on the widened operands bit for bit.
    ``live``: ``row_live(x_local)`` (GPU, fp32 or bf16 with even F); local
    rows it marks as all zero are not fetched, same result bit for bit. A 0
    for a row that holds a non-zero is a misuse: that row is then read as
    zeros. Not combined with ``packed`` or ``out_dtype``; with a fusable
    ``QuantRemote`` the quantized-gather kernel runs and ``live`` is not used
    for that call. Ignored on the CPU.
    ``compact``: which row-skipping kernel an fp32 call with ``live`` runs
    (None = SPMM_COMPACT): False the edge-walking one
    (csrc/spmm_rowskip.hip), True the edge-compacting one
    (csrc/spmm_compact.hip), which finds a segment's live edges with one
    ballot per chunk and spends its row fetches on them alone. A bf16 call
    with ``live`` always runs the compacting kernel. Same result bit for bit.
    Without ``live``, and on the CPU, it is ignored.
    ``quant_bf16``: what happens to a :class:`QuantRemote` whose gathered
    rows are bf16 (None = QUANT_BF16, off unless ADAQP_FUSED_DEQUANT_BF16=1).
    On, and with a ``QuantRemote.fusable_bf16`` operand, a bf16 call and the
    mixed call gather remote columns from the wire
    (csrc/spmm_quant_bf16.hip) instead of dequantizing it: same result bit
    for bit. ``packed`` and ``live`` are dropped for such a call, as the fp32
    quantized gather drops them. It runs the static order.
    ``order`` / ``chunk``: how the GPU kernel hands out segments (None =
    SPMM_ORDER / SPMM_CHUNK): 0 the static order, 1 the ordered sweep in
    tickets of ``chunk`` segments. Same result bit for bit. The mixed,
    quantized, bf16 packed and wave-index kernels only have the static order.
    """
    assert live is None or (packed is None and out_dtype is None), \
        'live is not combined with packed or out_dtype'
    if out_dtype is not None:
        return _spmm_mixed(view, x_local, x_remote, src_scale, dst_scale,
                           out, addend, packed, out_dtype, quant_bf16)
    indptr, indices, num_rows = view.indptr, view.indices, view.nrows
    quant = None
    if isinstance(x_remote, QuantRemote):
        if (bool(QUANT_BF16 if quant_bf16 is None else quant_bf16)
                and x_remote.fusable_bf16(x_local)):
            return _spmm_quant_bf16(view, x_local, x_remote, src_scale,
                                    dst_scale, out, addend, torch.bfloat16)
        if x_remote.fusable(x_local):
            assert x_remote.F == x_local.shape[1]
            assert view.max_col < x_local.shape[0] + x_remote.rows, \
                'the view names a column past the remote rows described'
            quant, x_remote, packed, live = x_remote, None, None, None
        else:
            x_remote = x_remote.dequantize(x_local.dtype)
    if not x_local.is_cuda and view.col_blocked:
        raise RuntimeError('column-blocked SpmmView is GPU-only (the CPU '
                           'fallback consumes indptr, which the blocked '
                           'layout does not preserve)')
    if x_local.is_cuda:
        if out is None:
            out = torch.empty(num_rows, x_local.shape[1], dtype=x_local.dtype,
                              device=x_local.device)
        else:
            assert out.is_contiguous() and out.shape[0] == num_rows
        empty = torch.empty(0, device=x_local.device)
        order = int(SPMM_ORDER if order is None else order)
        chunk = int(SPMM_CHUNK if chunk is None else chunk)
        if addend is not None:
            assert (addend.is_contiguous() and addend.dtype == out.dtype
                    and addend.shape == out.shape)
        if packed is not None:
            assert packed.matches(x_local), \
                'packed operand was not made from x_local'
        if live is not None and x_local.shape[0] > 0:
            bf16 = x_local.dtype == torch.bfloat16
            assert bf16 or x_local.dtype == torch.float32, \
                'the row-skipping spmm is fp32 or bf16'
            assert (live.dtype == torch.uint8
                    and live.shape == (x_local.shape[0],)), \
                'live operand was not made from x_local'
            use_compact = bf16 or bool(SPMM_COMPACT if compact is None
                                       else compact)
            run = (native().spmm_csr_compact if use_compact
                   else native().spmm_csr_rowskip)
            run(
                indices, x_local,
                x_remote if x_remote is not None else empty, out,
                src_scale if src_scale is not None else empty,
                dst_scale if dst_scale is not None else empty,
                view.seg_row, view.seg_e0, view.seg_e1, view.seg_part,
                view.zero_rows, view.part_ptr, view.n_part,
                addend if addend is not None else empty, live,
                order, chunk)
            return out
        native().spmm_csr(indices, x_local,
                          x_remote if x_remote is not None else empty, out,
                          src_scale if src_scale is not None else empty,
                          dst_scale if dst_scale is not None else empty,
                          view.seg_row, view.seg_e0, view.seg_e1,
                          view.seg_part, view.zero_rows, view.part_ptr,
                          view.n_part,
                          addend if addend is not None else empty,
                          bool(WAVE_INDEX if wave_index is None
                               else wave_index),
                          packed.buf if packed is not None else empty,
                          int(PACKED_DEPTH if packed_depth is None
                              else packed_depth),
                          quant.payload if quant is not None else empty,
                          quant.descriptors() if quant is not None else empty,
                          order, chunk)
        return out
    x = (torch.cat([x_local, x_remote], dim=0)
         if x_remote is not None and x_remote.numel() else x_local)
    xs = x * src_scale[:x.shape[0], None] if src_scale is not None else x
    key = (indptr.data_ptr(), indices.data_ptr(), num_rows, x.shape[0])
    sp = _csr_cache.get(key)
    if sp is None:
        crow = indptr.to(torch.int64)
        col = indices.to(torch.int64)
        val = torch.ones(col.numel(), dtype=torch.float32)
        sp = torch.sparse_csr_tensor(crow, col, val, size=(num_rows, x.shape[0]))
        if len(_csr_cache) > 64:
            _csr_cache.clear()
        _csr_cache[key] = sp
    y = torch.sparse.mm(sp, xs.float()).to(x.dtype)
    if dst_scale is not None:
        y = y * dst_scale[:, None]
    if addend is not None:
        y = y + addend
    if out is not None:
        out.copy_(y)
        return out
    return y


def _spmm_quant_bf16(view: 'SpmmView', x_local: Tensor, quant: QuantRemote,
                     src_scale, dst_scale, out, addend, out_dtype) -> Tensor:
    """:func:`spmm` on bf16 rows with a ``fusable_bf16`` QuantRemote: remote
    columns come from the wire, ``out`` and ``addend`` are ``out_dtype``
    (bf16, or fp32 for the mixed call)."""
    num_rows, F = view.nrows, x_local.shape[1]
    assert quant.F == F
    assert view.max_col < x_local.shape[0] + quant.rows, \
        'the view names a column past the remote rows described'
    if out is None:
        out = torch.empty(num_rows, F, dtype=out_dtype, device=x_local.device)
    else:
        assert (out.is_contiguous() and out.shape == (num_rows, F)
                and out.dtype == out_dtype)
    assert addend is None or (addend.is_contiguous() and addend.dtype == out_dtype
                              and addend.shape == out.shape)
    empty = torch.empty(0, device=x_local.device)
    native().spmm_csr_quant_bf16(
        view.indices, x_local.contiguous(), quant.payload, quant.descriptors(),
        out, src_scale if src_scale is not None else empty,
        dst_scale if dst_scale is not None else empty,
        view.seg_row, view.seg_e0, view.seg_e1, view.seg_part, view.zero_rows,
        view.part_ptr, view.n_part, addend if addend is not None else empty)
    return out


def _spmm_mixed(view: 'SpmmView', x_local: Tensor, x_remote, src_scale,
                dst_scale, out, addend, packed, out_dtype,
                quant_bf16=None) -> Tensor:
    """:func:`spmm` with ``out_dtype``: bf16 rows in, fp32 out."""
    assert out_dtype == torch.float32 and x_local.dtype == torch.bfloat16, \
        'the mixed spmm gathers bf16 rows into an fp32 result'
    assert packed is None, 'the mixed spmm takes no packed operand'
    assert x_local.shape[1] % 2 == 0, 'the mixed spmm needs an even F'
    if isinstance(x_remote, QuantRemote):
        if (bool(QUANT_BF16 if quant_bf16 is None else quant_bf16)
                and x_remote.fusable_bf16(x_local)):
            return _spmm_quant_bf16(view, x_local, x_remote, src_scale,
                                    dst_scale, out, addend, torch.float32)
        x_remote = x_remote.dequantize(torch.bfloat16)
    if x_remote is not None and not x_remote.numel():
        x_remote = None
    assert x_remote is None or x_remote.dtype == torch.bfloat16
    for t in (out, addend):
        assert t is None or t.dtype == torch.float32
    if not x_local.is_cuda:
        return spmm(view, x_local.float(),
                    None if x_remote is None else x_remote.float(),
                    src_scale, dst_scale, out=out, addend=addend)
    num_rows, F = view.nrows, x_local.shape[1]
    assert view.max_col < x_local.shape[0] + (
        0 if x_remote is None else x_remote.shape[0]), \
        'the view names a column past the rows given'
    if out is None:
        out = torch.empty(num_rows, F, dtype=torch.float32,
                          device=x_local.device)
    else:
        assert out.is_contiguous() and out.shape == (num_rows, F)
    assert addend is None or (addend.is_contiguous()
                              and addend.shape == out.shape)
    empty = torch.empty(0, device=x_local.device)
    native().spmm_csr_bf16in(view.indices, x_local.contiguous(),
                             x_remote.contiguous() if x_remote is not None
                             else empty, out,
                             src_scale if src_scale is not None else empty,
                             dst_scale if dst_scale is not None else empty,
                             view.seg_row, view.seg_e0, view.seg_e1,
                             view.seg_part, view.zero_rows, view.part_ptr,
                             view.n_part,
                             addend if addend is not None else empty)
    return out


# --------------------------------------------------------------------------
# column sum (bias gradient)
# --------------------------------------------------------------------------

def colsum(g: Tensor) -> Tensor:
    """``g.sum(0)`` of a [N, F] matrix in g's dtype. GPU: one deterministic
    pass of the native kernel (fp32 accumulate, fixed order)."""
    if g.is_cuda:
        return native().colsum(g.contiguous())
    return g.sum(dim=0)
