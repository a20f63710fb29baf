"""Distributed aggregation autograd ops.

Reference parity: ``AdaQP/model/ops.py`` (DistAggConv / DistAggSAGE,
full_graph_propagation / decomposed_graph_propagation) and the exchange
glue ``AdaQP/model/op_util.py:138-236``.

MI355X redesign of the overlap (reference: side CPU thread + 2 CUDA
events + 2 CPU events, ``ops.py:119-130``, ``op_util.py:101-130``):
RCCL collectives are stream-ordered device work, so the whole
quantize -> all_to_all -> dequantize pipeline is enqueued on a side HIP
stream while the central aggregation runs on the default stream; one
cuda event orders dequant-output -> marginal aggregation. No threads.

Backward uses the SAME exchange direction and the SAME CSR as forward
(bidirected graphs): the grad of my inner boundary nodes is sent out,
remote grads are received, and the in-edge aggregation with swapped
normalization performs the cross-partition reduction — exact transpose
(see ops.py:17-32 for the reference's equivalent on dgl.reverse graphs).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ..helpers import BitType, DistGNNType, PropagationMode
from ..comm.communicator import Communicator
from .kernels import (mixed_quantize, mixed_quantize_fused,
                      resolve_fused_quant, mixed_dequantize, spmm, QuantRemote,
                      resolve_fused_dequant, resolve_fused_dequant_bf16,
                      resolve_bwd_gather_bf16, round_rows_bf16)


# --------------------------------------------------------------------------
# boundary exchange
# --------------------------------------------------------------------------

def _exchange_start(engine, x_local: Tensor, key: str, quant: bool):
    """Device-side producer work only (gather or quantize kernels) — no
    transport. Split from :func:`_exchange_finish` so the decomposed path
    can enqueue the central aggregation BETWEEN the two: the transport may
    block the host (gloo staging), and anything enqueued after it would
    lose the overlap."""
    if quant:
        plan = engine.plans[key]
        seed = engine.next_seed()
        if x_local.is_cuda and resolve_fused_quant(
                getattr(engine, 'fused_quant', None)):
            # one launch for every bit width; on a tracing epoch the same
            # launch adds the variance proxy into traced[key], so the
            # index_select + engine.trace pair is not run
            acc = (engine.trace_accumulator(key)
                   if engine.is_tracing and engine.graph.num_send else None)
            with engine.timer.record(f'{key}_quant'):
                payload, params = mixed_quantize_fused(x_local, plan.send,
                                                       seed, trace=acc)
            return ('qt', payload, params, x_local.dtype)
        if engine.is_tracing:
            send = x_local.index_select(0, engine.graph.total_send_idx)
            engine.trace(key, send)
        with engine.timer.record(f'{key}_quant'):
            payload, params = mixed_quantize(x_local, plan.send, seed)
        return ('qt', payload, params, x_local.dtype)
    send = x_local.index_select(0, engine.graph.total_send_idx)
    if engine.is_tracing:
        engine.trace(key, send)
    return ('fp', send, None, x_local.dtype)


def _fused_dequant(engine, x_local: Tensor, key: str, quant: bool) -> bool:
    """True if this exchange hands the SpMM the wire buffer instead of a
    dequantized block: the engine's switch is on, the exchange is
    quantized, fp32, on the GPU, and the plan has its per-row table. A bf16
    exchange qualifies too when ``engine.fused_dequant_bf16`` is on as well
    (the SpMM then runs csrc/spmm_quant_bf16.hip)."""
    return (quant and x_local.is_cuda
            and (x_local.dtype == torch.float32
                 or (x_local.dtype == torch.bfloat16 and _quant_bf16(engine)))
            and resolve_fused_dequant(getattr(engine, 'fused_dequant', None))
            and engine.plans[key].recv.row_tab is not None)


def _quant_bf16(engine) -> bool:
    return resolve_fused_dequant_bf16(
        getattr(engine, 'fused_dequant_bf16', None))


def _exchange_finish(engine, staged, key: str, fused: bool = False,
                     remote_dtype: Optional[torch.dtype] = None):
    """Transport + consumer-side kernels (dequant/scatter). ``fused``
    (quantized exchanges only): return a :class:`QuantRemote` over the
    received wire buffer; the only consumer-side kernel is then the one
    that writes its row descriptors. ``remote_dtype`` (quantized, not
    fused): dtype of the dequantized block instead of the sender's."""
    comm = Communicator.ctx
    g = engine.graph
    kind, a, b, dtype = staged
    if kind == 'fp':
        with engine.timer.record(f'{key}_exchange'):
            recv, _ = comm.exchange_rows(a, g.send_splits, g.recv_splits)
        return recv
    plan = engine.plans[key]
    payload, params = a, b
    # fused: the collective gets a view of the exact wire length of a
    # buffer with the spare bytes the gather's window loads need
    recv_payload = (QuantRemote.wire_buffer(plan.recv.total_bytes,
                                            payload.device) if fused else
                    torch.empty(plan.recv.total_bytes, dtype=torch.uint8,
                                device=payload.device))
    recv_params = torch.empty(2 * plan.recv.total_nodes, dtype=torch.bfloat16,
                              device=payload.device)
    with engine.timer.record(f'{key}_exchange'):
        comm.all_to_all_v(recv_payload, payload,
                          plan.recv.byte_splits, plan.send.byte_splits)
        comm.all_to_all_v(recv_params, params,
                          plan.recv.param_splits, plan.send.param_splits)
    if fused:
        remote = QuantRemote(recv_payload, recv_params, plan.recv, plan.F,
                             rows=g.num_remote)
        with engine.timer.record(f'{key}_dequant'):
            if remote.rows:
                remote.descriptors()
        return remote
    out = torch.empty(g.num_remote, plan.F, dtype=remote_dtype or dtype,
                      device=payload.device)
    with engine.timer.record(f'{key}_dequant'):
        mixed_dequantize(recv_payload, recv_params, plan.recv, out)
    return out


def fp_exchange(engine, x_local: Tensor, key: str) -> Tensor:
    return _exchange_finish(engine,
                            _exchange_start(engine, x_local, key, False), key)


def qt_exchange(engine, x_local: Tensor, key: str) -> Tensor:
    return _exchange_finish(engine,
                            _exchange_start(engine, x_local, key, True), key)


def _exchange(engine, x_local: Tensor, key: str, is_train: bool) -> Tensor:
    if engine.bit_type == BitType.QUANT and is_train:
        return qt_exchange(engine, x_local, key)
    return fp_exchange(engine, x_local, key)


# --------------------------------------------------------------------------
# aggregation (SpMM with model-specific normalization)
# --------------------------------------------------------------------------

def _scales(engine, mode: PropagationMode) -> Tuple[Optional[Tensor], Optional[Tensor], bool]:
    """(src_scale[N], dst_scale[I], add_self) for the model/mode."""
    fwd = mode == PropagationMode.Forward
    if engine.model_type == DistGNNType.DistGCN:
        return ((engine.gcn_src_f, engine.gcn_dst_f, False) if fwd
                else (engine.gcn_src_b, engine.gcn_dst_b, False))
    if engine.agg_type == 'mean':
        return ((None, engine.sage_dst_f, False) if fwd
                else (engine.sage_src_b, None, False))
    if engine.agg_type == 'gcn':
        return ((None, engine.sage1_dst_f, True) if fwd
                else (engine.sage1_src_b, None, True))
    raise ValueError(f'unknown aggregator {engine.agg_type}')


def _agg(engine, view, x_local: Tensor, x_remote, src_scale, dst_scale,
         out=None, addend=None, packed=None, out_dtype=None,
         live=None) -> Tensor:
    """SpMM over one SpmmView. src_scale is the full [N] vector; dst_scale
    and the optional [num_inner, F] addend are sliced to the view's row
    range. ``packed``: ``pack_rows(x_local)`` (the gather's source rows, so
    the same handle serves every view). ``out_dtype``: the mixed call, bf16
    rows gathered into an fp32 result. ``live``: ``row_live(x_local)``, one
    array of the local rows for every view; all-zero local rows are not
    fetched. A QuantRemote ``x_remote`` goes to spmm with the engine's
    ``fused_dequant_bf16`` switch as ``quant_bf16`` (only bf16 rows read it;
    ``packed`` and ``live`` are then dropped for that view)."""
    ds = (dst_scale[view.base:view.base + view.nrows]
          if dst_scale is not None else None)
    ad = (addend[view.base:view.base + view.nrows]
          if addend is not None else None)
    if isinstance(x_remote, QuantRemote) and x_local.dtype == torch.bfloat16:
        return spmm(view, x_local, x_remote, src_scale, ds, out=out,
                    addend=ad, packed=packed, out_dtype=out_dtype, live=live,
                    quant_bf16=_quant_bf16(engine))
    if out_dtype is not None:
        assert packed is None
        return spmm(view, x_local, x_remote, src_scale, ds, out=out,
                    addend=ad, out_dtype=out_dtype)
    if packed is not None:
        assert live is None
        return spmm(view, x_local, x_remote, src_scale, ds, out=out,
                    addend=ad, packed=packed)
    if live is not None:
        return spmm(view, x_local, x_remote, src_scale, ds, out=out,
                    addend=ad, live=live)
    return spmm(view, x_local, x_remote, src_scale, ds, out=out, addend=ad)


def _addend_kw(addend, packed=None, live=None) -> dict:
    """_agg's ``addend``, ``packed`` and ``live`` keywords, each passed only
    when there is one, so the plain aggregation keeps the call signature it
    always had."""
    kw = {} if addend is None else {'addend': addend}
    if packed is not None:
        kw['packed'] = packed
    if live is not None:
        kw['live'] = live
    return kw


# --------------------------------------------------------------------------
# bf16 gather operand of the fp32 backward aggregation (opt-in)
#
# The backward SpMM of an fp32 engine gathers a dense GEMM output at 4F bytes
# per edge. With the switch on it gathers rows rounded to bf16 WITHOUT BIAS
# (round_rows_bf16: stochastic rounding, as the quantizer does for remote
# rows at 2/4/8 bits) and keeps accumulators, addend and result in fp32
# (csrc/spmm_mixed.hip). Only the SpMM operands change: the exchange reads
# the dense fp32 tensor, so wire format, plans, assigner and tracing are as
# without it, and the rounding seeds come from a counter of their own, so the
# quantization stream (engine.next_seed) is too.
# --------------------------------------------------------------------------

_GATHER_SALT = 0x62663136      # keeps the stream apart from the fused norm's


def bwd_gather_seed(engine, layer: int, counter: int) -> int:
    """Rounding seed of the ``counter``-th bf16-gather backward of
    ``engine``: the hash chain of models/norm.py over (base_seed, layer,
    counter, rank)."""
    from ..models.norm import derive_seed
    rank = Communicator.ctx.rank if Communicator.ctx is not None else 0
    return derive_seed(engine.base_seed ^ _GATHER_SALT, layer, counter, rank)


def next_bwd_gather_seed(engine, x: Tensor, layer: int) -> Optional[int]:
    """What a backward caller passes to ``propagate(gather_bf16=...)`` for
    the operand ``x``: ``None`` unless the switch is on, the engine computes
    in fp32 and ``x`` is an fp32 [N, F] tensor with even F; else the next
    seed (``engine.bwd_gather_calls`` counts them)."""
    if not (resolve_bwd_gather_bf16(getattr(engine, 'bwd_gather_bf16', None))
            and engine.compute_dtype == torch.float32
            and x.dtype == torch.float32 and x.dim() == 2
            and x.shape[1] > 0 and x.shape[1] % 2 == 0):
        return None
    seed = bwd_gather_seed(engine, layer, engine.bwd_gather_calls)
    engine.bwd_gather_calls += 1
    return seed


def _round_remote(remote, seed: int, num_local: int):
    """The remote operand of a bf16-gather SpMM: a full-precision block is
    rounded with the tags that follow the local rows'; a block dequantized
    into bf16, or a QuantRemote (which spmm dequantizes into one), is
    already that."""
    if isinstance(remote, Tensor) and remote.dtype == torch.float32:
        return round_rows_bf16(remote, seed, tag_base=num_local)
    return remote


def _self_term(engine, x_local: Tensor, mode: PropagationMode) -> Tensor:
    """SAGE 'gcn' aggregator self term (reference ops.py:44-47,57-64)."""
    I = engine.graph.num_inner
    scale = (engine.sage1_dst_f if mode == PropagationMode.Forward
             else engine.sage1_src_b[:I])
    return (x_local[:I] * scale[:, None]).to(x_local.dtype)


# --------------------------------------------------------------------------
# propagation paths
# --------------------------------------------------------------------------

def full_propagation(engine, x_local: Tensor, key: str, is_train: bool,
                     mode: PropagationMode, addend=None,
                     packed=None, gather_bf16: Optional[int] = None,
                     live=None) -> Tensor:
    quant = engine.bit_type == BitType.QUANT and is_train
    if _fused_dequant(engine, x_local, key, quant):
        remote = _exchange_finish(
            engine, _exchange_start(engine, x_local, key, True), key,
            fused=True)
    elif quant and gather_bf16 is not None:
        # dequantized straight into the bf16 block the SpMM gathers
        remote = _exchange_finish(
            engine, _exchange_start(engine, x_local, key, True), key,
            remote_dtype=torch.bfloat16)
    else:
        remote = _exchange(engine, x_local, key, is_train)
    src_scale, dst_scale, add_self = _scales(engine, mode)
    with engine.timer.record(f'{key}_full_aggregation'):
        if gather_bf16 is not None:
            y = _agg(engine, engine.full_view,
                     round_rows_bf16(x_local, gather_bf16),
                     _round_remote(remote, gather_bf16, x_local.shape[0]),
                     src_scale, dst_scale, addend=addend,
                     out_dtype=torch.float32)
        else:
            y = _agg(engine, engine.full_view, x_local, remote, src_scale,
                     dst_scale, **_addend_kw(addend, packed, live))
        if add_self:
            y = y + _self_term(engine, x_local, mode)
    return y


def decomposed_propagation(engine, x_local: Tensor, key: str, is_train: bool,
                           mode: PropagationMode, addend=None,
                           packed=None,
                           gather_bf16: Optional[int] = None,
                           live=None) -> Tensor:
    """Central aggregation (default stream) overlapped with
    quant->all_to_all->dequant (comm stream).

    Host-call order matters: producer kernels (quantize/gather) are
    enqueued on the comm stream, then the central SpMM is enqueued on the
    default stream, and only THEN the transport runs. With RCCL the
    transport is stream-ordered device work so any order would overlap;
    with a host-blocking transport (gloo staging — several ranks sharing
    one GPU, or CPU debug) the central SpMM must already be in the GPU
    queue when the host blocks, otherwise the overlap the decomposition
    exists for never happens (the reference needed a side thread for
    this, ``ops.py:156-193``; stream order + one event replaces it)."""
    src_scale, dst_scale, add_self = _scales(engine, mode)
    g = engine.graph
    on_gpu = x_local.is_cuda
    quant = engine.bit_type == BitType.QUANT and is_train
    # bf16 gather: both views read ONE rounded copy of the local rows (xg);
    # the exchange and the self term keep reading the fp32 x_local
    bf16 = gather_bf16 is not None
    agg_kw = ({'addend': addend, 'out_dtype': torch.float32} if bf16
              else _addend_kw(addend, packed, live))
    deq_kw = {'remote_dtype': torch.bfloat16} if bf16 and quant else {}
    xg = x_local

    if on_gpu:
        cur = torch.cuda.current_stream()
        engine.comm_stream.wait_stream(cur)          # x_local is ready
        x_local.record_stream(engine.comm_stream)
        with torch.cuda.stream(engine.comm_stream):
            staged = _exchange_start(engine, x_local, key, quant)
        # central and marginal SpMMs write disjoint row slices of ONE
        # output tensor (no torch.cat: the cat was a full [I,F]
        # read+write per propagation)
        C = g.num_central
        y = torch.empty(g.num_inner, x_local.shape[1], dtype=x_local.dtype,
                        device=x_local.device)
        # central rows only touch local columns -> enqueue NOW, before
        # the transport can block the host
        with engine.timer.record(f'{key}_central_aggregation'):
            if bf16:
                xg = round_rows_bf16(x_local, gather_bf16)
            _agg(engine, engine.central_view, xg, None, src_scale,
                 dst_scale, out=y[:C], **agg_kw)
        # fused dequant: `remote` is a QuantRemote (the wire buffer and its
        # row descriptors); the marginal SpMM gathers from it, and a packed
        # operand is ignored for that view (ops/kernels.py::spmm)
        fused_kw = ({'fused': True}
                    if _fused_dequant(engine, x_local, key, quant) else deq_kw)
        with torch.cuda.stream(engine.comm_stream):
            remote = _exchange_finish(engine, staged, key, **fused_kw)
            engine.remote_ready.record(engine.comm_stream)
        torch.cuda.current_stream().wait_event(engine.remote_ready)
        remote.record_stream(torch.cuda.current_stream())
        with engine.timer.record(f'{key}_marginal_aggregation'):
            if bf16:
                remote = _round_remote(remote, gather_bf16, x_local.shape[0])
            _agg(engine, engine.marginal_view, xg, remote, src_scale,
                 dst_scale, out=y[C:], **agg_kw)
    else:
        if deq_kw:
            remote = _exchange_finish(
                engine, _exchange_start(engine, x_local, key, True), key,
                **deq_kw)
        else:
            remote = _exchange(engine, x_local, key, is_train)
        if bf16:
            xg = round_rows_bf16(x_local, gather_bf16)
            remote = _round_remote(remote, gather_bf16, x_local.shape[0])
        with engine.timer.record(f'{key}_central_aggregation'):
            y_c = _agg(engine, engine.central_view, xg, None, src_scale,
                       dst_scale, **agg_kw)
        with engine.timer.record(f'{key}_marginal_aggregation'):
            y_m = _agg(engine, engine.marginal_view, xg, remote,
                       src_scale, dst_scale, **agg_kw)
        y = torch.cat([y_c, y_m], dim=0)
    if add_self:
        y = y + _self_term(engine, x_local, mode)
    return y


def propagate(engine, x_local: Tensor, layer: int, is_train: bool,
              mode: PropagationMode, addend=None, packed=None,
              gather_bf16: Optional[int] = None, live=None) -> Tensor:
    """``addend`` ([num_inner, F], the result's dtype): added to the
    aggregation in the SpMM epilogue, before any self term.
    ``packed``: ``pack_rows(x_local)``; the SpMMs gather local rows from
    it, the exchange still reads the dense ``x_local``.
    ``gather_bf16``: a seed from :func:`next_bwd_gather_seed` (the two
    backward callers only); the SpMMs gather rows rounded to bf16 with it
    into the fp32 result. Not combined with ``packed``.
    ``live``: ``row_live(x_local)`` (GPU fp32); the SpMMs do not fetch the
    local rows it marks as all zero, the exchange still reads the dense
    ``x_local``. Not combined with ``packed`` or ``gather_bf16``."""
    key = (f'forward{layer}' if mode == PropagationMode.Forward
           else f'backward{layer}')
    kw = {} if packed is None else {'packed': packed}
    if live is not None:
        assert packed is None and gather_bf16 is None
        kw['live'] = live
    if gather_bf16 is not None:
        assert packed is None and x_local.dtype == torch.float32
        kw['gather_bf16'] = gather_bf16
    if engine.use_parallel:
        return decomposed_propagation(engine, x_local, key, is_train, mode,
                                      addend=addend, **kw)
    return full_propagation(engine, x_local, key, is_train, mode,
                            addend=addend, **kw)


# --------------------------------------------------------------------------
# autograd Function (one class serves GCN and SAGE; the engine carries the
# model type — reference has DistAggConv/DistAggSAGE, ops.py:69-111)
# --------------------------------------------------------------------------

class DistAgg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_local: Tensor, engine, layer: int, is_train: bool) -> Tensor:
        ctx.engine = engine
        ctx.layer = layer
        ctx.in_dtype = x_local.dtype
        x_local = x_local.to(engine.compute_dtype).contiguous()
        return propagate(engine, x_local, layer, is_train, PropagationMode.Forward)

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        g = grad_out.to(ctx.engine.compute_dtype).contiguous()
        seed = next_bwd_gather_seed(ctx.engine, g, ctx.layer)
        kw = {} if seed is None else {'gather_bf16': seed}
        gx = propagate(ctx.engine, g, ctx.layer, True,
                       PropagationMode.Backward, **kw)
        return gx.to(ctx.in_dtype), None, None, None


def dist_aggregate(x_local: Tensor, engine, layer: int, is_train: bool) -> Tensor:
    return DistAgg.apply(x_local, engine, layer, is_train)
