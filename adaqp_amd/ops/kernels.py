"""Device dispatch for the hot ops.

GPU (MI355X): hand-written CDNA4 HIP kernels from ``adaqp_amd/csrc``
(built in-tree as ``adaqp_amd._C``). The GPU path REFUSES to fall back —
if the extension is missing on a CUDA device, that is a build error, not
a reason to silently run eager PyTorch.

CPU: torch reference implementations (bit-exact for quant pack/unpack —
same hash RNG) used by unit tests and the CPU/gloo plumbing config.
"""
from __future__ import annotations

from typing import Optional, Tuple

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


def spmm(view: 'SpmmView', x_local: Tensor, x_remote: Optional[Tensor],
         src_scale: Optional[Tensor], dst_scale: Optional[Tensor],
         out: Optional[Tensor] = None, addend: Optional[Tensor] = None,
         wave_index: Optional[bool] = None,
         packed: Optional[PackedRows] = None,
         packed_depth: Optional[int] = None) -> Tensor:
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
    ``packed``: ``pack_rows(x_local)``; local columns are then gathered
    from the packed copy (remote columns and overflow rows from the dense
    tensors), same result bit for bit. Ignored on the CPU.
    ``packed_depth``: row fetches in flight per lane in that kernel
    (None = PACKED_DEPTH).
    """
    indptr, indices, num_rows = view.indptr, view.indices, view.nrows
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
        if addend is not None:
            assert (addend.is_contiguous() and addend.dtype == out.dtype
                    and addend.shape == out.shape)
        if packed is not None:
            assert packed.matches(x_local), \
                'packed operand was not made from x_local'
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
                              else packed_depth))
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


# --------------------------------------------------------------------------
# column sum (bias gradient)
# --------------------------------------------------------------------------

def colsum(g: Tensor) -> Tensor:
    """``g.sum(0)`` of a [N, F] matrix in g's dtype. GPU: one deterministic
    pass of the native kernel (fp32 accumulate, fixed order)."""
    if g.is_cuda:
        return native().colsum(g.contiguous())
    return g.sum(dim=0)
