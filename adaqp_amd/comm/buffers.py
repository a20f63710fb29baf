"""Mixed-bit boundary-exchange layout plans.

Reference parity: ``AdaQP/communicator/buffer.py`` (pinned-CPU + GPU
train/test buffers, per-bit index bookkeeping exchanged by
``all_gather_object``, rebuilt on every re-assignment) and the mixed
quantization glue ``AdaQP/model/op_util.py:189-236``.

MI355X redesign: everything stays on the GPU, so "buffers" reduce to a
LAYOUT PLAN — flat per-bit index/offset tensors that drive ONE fused
quant (or dequant) HIP kernel launch per bit-width and ONE
``all_to_all_single`` per payload. Wire format for each key
(``forward{l}``/``backward{l}``):

    payload uint8, peer-major; within a peer: bit groups in (2,4,8)
    order; within a group: the agreed global-id node order; each node
    occupies ceil(F*bits/8) bytes.
    params  bf16, 2 per node (scale, rmin), same node order.

Both sides derive the same layout from the per-node bit widths, which
the sender distributes with one int8 all-to-all (``exchange_bits``)
after every re-assignment — replacing the reference's
``all_gather_object`` of nested index dicts (``buffer.py:219-231``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
from torch import Tensor

from ..graph import LocalGraph
from .communicator import Communicator

BITS_SET = (2, 4, 8)


def bytes_per_node(F: int, bits: int) -> int:
    return (F * bits + 7) // 8


@dataclass
class SidePlan:
    """One direction (send or recv) of a key's wire layout."""
    F: int
    rows: Dict[int, Tensor]       # bit -> int64 row ids (local x rows / remote-block rows)
    pos: Dict[int, Tensor]        # bit -> int64 wire node positions
    off: Dict[int, Tensor]        # bit -> int64 wire byte offsets
    byte_splits: List[int]        # per peer payload bytes
    node_splits: List[int]        # per peer node counts
    total_bytes: int
    total_nodes: int
    # recv side: int32 [max row + 1, 4], row r = {wire byte offset (the
    # unsigned 32-bit value's bits), params slot, bits, 0} of remote-block
    # row r, all zero (bits 0) for a row no peer sends. None when it was not
    # asked for or total_bytes does not fit an unsigned 32-bit offset.
    row_tab: Optional[Tensor] = None
    # send side: send_rows int64 [S] = the peers' send rows concatenated, so
    # indexed by send slot (the position in graph.total_send_idx); send_tab
    # int32 [S, 4], row s = {source row in x_local, wire byte offset (the
    # unsigned 32-bit value's bits), params slot (= RNG tag), bits} of send
    # slot s: the one-launch quantizer's descriptor (csrc/quant_mixed.hip).
    # Both None when not asked for; send_tab also None when total_bytes does
    # not fit an unsigned 32-bit offset or a source row does not fit int32.
    send_rows: Optional[Tensor] = None
    send_tab: Optional[Tensor] = None
    send_max_row: int = -1        # largest source row (-1: none), host side

    @property
    def param_splits(self) -> List[int]:
        return [2 * n for n in self.node_splits]

    def to(self, device) -> 'SidePlan':
        self.rows = {b: t.to(device) for b, t in self.rows.items()}
        self.pos = {b: t.to(device) for b, t in self.pos.items()}
        self.off = {b: t.to(device) for b, t in self.off.items()}
        if self.row_tab is not None:
            self.row_tab = self.row_tab.to(device)
        if self.send_rows is not None:
            self.send_rows = self.send_rows.to(device)
        if self.send_tab is not None:
            self.send_tab = self.send_tab.to(device)
        return self


@dataclass
class KeyPlan:
    """Quantized-exchange plan for one (layer, direction) key."""
    F: int
    send: SidePlan
    recv: SidePlan

    def to(self, device) -> 'KeyPlan':
        self.send.to(device)
        self.recv.to(device)
        return self


def _row_table(rows: Dict[int, Tensor], pos: Dict[int, Tensor],
               off: Dict[int, Tensor], total_bytes: int) -> Optional[Tensor]:
    """The per-row view of a layout (SidePlan.row_tab): the same
    rows/pos/off, indexed by row instead of grouped by bit width."""
    if total_bytes >= 2 ** 32:
        return None
    n = max([int(r.max()) + 1 for r in rows.values() if r.numel()], default=0)
    tab = torch.zeros(n, 4, dtype=torch.int64)
    for b in BITS_SET:
        tab[rows[b], 0] = off[b]
        tab[rows[b], 1] = pos[b]
        tab[rows[b], 2] = b
    tab[:, 0] -= (tab[:, 0] >= 2 ** 31).to(torch.int64) * 2 ** 32
    return tab.to(torch.int32)


def _send_table(slot: Dict[int, Tensor], rows: Dict[int, Tensor],
                pos: Dict[int, Tensor], off: Dict[int, Tensor],
                total_nodes: int, total_bytes: int,
                max_row: int) -> Optional[Tensor]:
    """The per-send-slot view of a send layout (SidePlan.send_tab): the same
    rows/pos/off, indexed by send slot instead of grouped by bit width."""
    if total_bytes >= 2 ** 32 or max_row >= 2 ** 31:
        return None
    tab = torch.zeros(total_nodes, 4, dtype=torch.int64)
    for b in BITS_SET:
        tab[slot[b], 0] = rows[b]
        tab[slot[b], 1] = off[b]
        tab[slot[b], 2] = pos[b]
        tab[slot[b], 3] = b
    tab[:, 1] -= (tab[:, 1] >= 2 ** 31).to(torch.int64) * 2 ** 32
    return tab.to(torch.int32)


def _layout(bits_per_peer: List[Optional[Tensor]],
            rows_per_peer: List[Optional[Tensor]], F: int,
            row_tab: bool = True, send_tab: bool = False) -> SidePlan:
    """Build one side's layout from per-peer bit vectors (agreed order).
    ``row_tab``: also build the per-row table (the recv side's rows are
    remote-block rows, each at most once; a send side has no use for it).
    ``send_tab``: also build the send side's per-slot table and row list
    (a source row may be sent to several peers, so it is indexed by send
    slot, not by row)."""
    rows = {b: [] for b in BITS_SET}
    pos = {b: [] for b in BITS_SET}
    off = {b: [] for b in BITS_SET}
    slot = {b: [] for b in BITS_SET}
    slot_rows: List[Tensor] = []
    byte_splits, node_splits = [], []
    p_cursor = 0
    b_cursor = 0
    for bits_vec, rows_vec in zip(bits_per_peer, rows_per_peer):
        n = 0 if bits_vec is None else int(bits_vec.numel())
        if n == 0:
            byte_splits.append(0)
            node_splits.append(0)
            continue
        peer_bytes = 0
        slot_rows.append(rows_vec.to(torch.int64))
        for b in BITS_SET:
            sel = torch.nonzero(bits_vec == b, as_tuple=True)[0]
            k = int(sel.numel())
            if k == 0:
                continue
            bpn = bytes_per_node(F, b)
            rows[b].append(rows_vec[sel])
            slot[b].append(sel + sum(node_splits))
            pos[b].append(torch.arange(k, dtype=torch.int64) + p_cursor)
            off[b].append(torch.arange(k, dtype=torch.int64) * bpn + b_cursor)
            p_cursor += k
            b_cursor += k * bpn
            peer_bytes += k * bpn
        if p_cursor - sum(node_splits) != n:
            bad = set(torch.unique(bits_vec).tolist()) - set(BITS_SET)
            raise ValueError(f'invalid bit widths in assignment: {bad}')
        byte_splits.append(peer_bytes)
        node_splits.append(n)
    cat = lambda d: {b: (torch.cat(v) if v else torch.empty(0, dtype=torch.int64))
                     for b, v in d.items()}
    rows, pos, off = cat(rows), cat(pos), cat(off)
    tab = _row_table(rows, pos, off, b_cursor) if row_tab else None
    plan = SidePlan(F, rows, pos, off, byte_splits, node_splits,
                    b_cursor, p_cursor, tab)
    if send_tab:
        plan.send_rows = (torch.cat(slot_rows) if slot_rows
                          else torch.empty(0, dtype=torch.int64))
        assert plan.send_rows.numel() == p_cursor
        plan.send_max_row = (int(plan.send_rows.max()) if p_cursor else -1)
        assert p_cursor == 0 or int(plan.send_rows.min()) >= 0
        plan.send_tab = _send_table(cat(slot), rows, pos, off, p_cursor,
                                    b_cursor, plan.send_max_row)
    return plan


def exchange_bits(comm: Communicator, graph: LocalGraph,
                  send_bits: Dict[int, Tensor]) -> List[Optional[Tensor]]:
    """Distribute my per-node bit widths to consumers; returns per-peer bit
    vectors for my remote block (CPU int8 gloo all-to-all)."""
    send_parts = []
    for p in range(graph.world_size):
        if graph.send_splits[p]:
            send_parts.append(send_bits[p].to(torch.uint8).cpu())
    send = torch.cat(send_parts) if send_parts else torch.empty(0, dtype=torch.uint8)
    recv = torch.empty(sum(graph.recv_splits), dtype=torch.uint8)
    torch.distributed.all_to_all_single(
        recv, send, list(graph.recv_splits), list(graph.send_splits))
    out: List[Optional[Tensor]] = []
    o = 0
    for p in range(graph.world_size):
        n = graph.recv_splits[p]
        out.append(recv[o:o + n].to(torch.int64) if n else None)
        o += n
    return out


def build_key_plan(comm: Communicator, graph: LocalGraph, F: int,
                   send_bits: Dict[int, Tensor],
                   device=None) -> KeyPlan:
    """send_bits: peer -> int64 bit widths over send_idx[peer] order."""
    send_bits_l = [send_bits.get(p) if p != graph.rank and graph.send_splits[p]
                   else None for p in range(graph.world_size)]
    send_rows_l = [graph.send_idx[p].cpu() if graph.send_splits[p] else None
                   for p in range(graph.world_size)]
    recv_bits_l = exchange_bits(comm, graph, send_bits)
    base = 0
    recv_rows_l: List[Optional[Tensor]] = []
    for p in range(graph.world_size):
        n = graph.recv_splits[p]
        recv_rows_l.append(torch.arange(base, base + n, dtype=torch.int64) if n else None)
        base += n
    plan = KeyPlan(F, _layout(send_bits_l, send_rows_l, F, row_tab=False,
                              send_tab=True),
                   _layout(recv_bits_l, recv_rows_l, F))
    # send slot s is position s of total_send_idx: the traced accumulator
    # (GraphEngine.traced) is indexed that way
    assert torch.equal(plan.send.send_rows,
                       graph.total_send_idx.cpu().to(torch.int64)), \
        'send plan rows are not graph.total_send_idx'
    if device is not None:
        plan.to(device)
    return plan


def uniform_bits(graph: LocalGraph, bits: int) -> Dict[int, Tensor]:
    return {p: torch.full((graph.send_splits[p],), bits, dtype=torch.int64)
            for p in range(graph.world_size) if graph.send_splits[p]}
