"""Float64 oracles for the distributed aggregation layer (no GPU code).

``kernel_oracles.py`` pins each HIP kernel; this module pins what
``adaqp_amd/ops/dist_agg.py`` composes from them: the exchange routing, the
engine's scale vectors, the central/marginal split, the self term and the
dtype casts of ``DistAgg``. The reference is the dense operator over the
WHOLE graph, with degrees recomputed here from the edge list, so nothing
of the engine's own bookkeeping enters it.

Tolerance model (same as ``kernel_oracles``): count the fp32 roundings
(``U32`` = 2^-24 relative each) against S, the operator applied to |T|,
and add half a bf16 ulp wherever a value is stored as bf16. No bound is
sized from an output under test.

One worker (``run_rank``) runs every case on one rank, on the CPU or the
GPU; ``test_agg_oracles.py`` spawns it over gloo on the CPU and
``test_dist_agg_gpu.py`` on one MI355X shared by three ranks.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from adaqp_amd.helpers import DistGNNType, PropagationMode, RunMode
from kernel_oracles import (U32, _first, bf16_half_ulp, pack_delta,
                            segs_per_row, spmm_reference)

FWD, BWD = PropagationMode.Forward, PropagationMode.Backward

# An entry of an engine scale vector is an fp32 pow()/reciprocal of an
# exactly representable degree, evaluated by the device's math library:
# within 2 fp32 ulps of the true power, i.e. 4 half-ulp units.
SCALE_U32 = 4

MODELS = (('gcn', 'mean'), ('sage', 'mean'), ('sage', 'gcn'))
MODES = ('Vanilla', 'AdaQP-p', 'AdaQP-q', 'AdaQP')
BITS = (2, 4, 8)
WORLD = 3
LAYER = 1                      # no backward0 plan exists (engine.exchange_keys)
SEED_COUNTER = 40              # engine._rng_counter before every replayed call


def model_name(kind: str, agg: str) -> str:
    return 'GCN' if kind == 'gcn' else f'SAGE-{agg}'


# --------------------------------------------------------------------------
# the dense global operator
# --------------------------------------------------------------------------

_dense_cache: dict = {}


def _dense(g):
    """(A, din, dout) in float64; A[dst, src] = 1; degrees clamped to 1."""
    hit = _dense_cache.get(id(g))
    if hit is None:
        n = g.num_nodes
        A = torch.zeros(n, n, dtype=torch.float64)
        A[g.dst, g.src] = 1.0
        din = torch.bincount(g.dst, minlength=n).clamp(min=1).double()
        dout = torch.bincount(g.src, minlength=n).clamp(min=1).double()
        hit = _dense_cache[id(g)] = (g, A, din, dout)
    return hit[1:]


def _scale_vectors(kind: str, agg: str, direction, din: Tensor, dout: Tensor):
    """(src, dst, self) float64 vectors or None, by degree: the operator is
    dst * (A~ @ (src * T)) + self * T with A~ = A forward, A^T backward."""
    fwd = direction == FWD
    if kind == 'gcn':
        return ((dout.pow(-0.5), din.pow(-0.5), None) if fwd
                else (din.pow(-0.5), dout.pow(-0.5), None))
    if agg == 'mean':
        return (None, 1.0 / din, None) if fwd else (1.0 / din, None, None)
    if agg == 'gcn':
        s = 1.0 / (din + 1.0)
        return (None, s, s) if fwd else (s, None, s)
    raise ValueError((kind, agg))


def _operator_parts(g, kind, agg, direction, T: Tensor):
    """(agg_ref, self_ref | None, S_agg, S_self) over all nodes, float64."""
    A, din, dout = _dense(g)
    T = T.cpu().double()
    src, dst, slf = _scale_vectors(kind, agg, direction, din, dout)
    M = A if direction == FWD else A.t()

    def apply(t):
        y = M @ (t * src[:, None] if src is not None else t)
        return y * dst[:, None] if dst is not None else y
    ref, S = apply(T), apply(T.abs())
    if slf is None:
        return ref, None, S, torch.zeros_like(S)
    return ref, T * slf[:, None], S, T.abs() * slf[:, None]


def global_operator(g, kind: str, agg: str, direction, T: Tensor):
    """(ref, S) in float64 over the whole GlobalGraph.

    forward   GCN        Din^-1/2 A Dout^-1/2 T
              SAGE mean  Din^-1 A T
              SAGE gcn   (A T + T) / (Din + 1)
    backward  the exact transposes:
              GCN        Dout^-1/2 A^T Din^-1/2 T
              SAGE mean  A^T Din^-1 T
              SAGE gcn   A^T (T / (Din + 1)) + T / (Din + 1)
    S is the same expression on |T| (every factor is non-negative)."""
    ref, slf, S, S_self = _operator_parts(g, kind, agg, direction, T)
    return (ref if slf is None else ref + slf), S + S_self


# --------------------------------------------------------------------------
# counted tolerance and the two aggregate checkers
# --------------------------------------------------------------------------

def _counted_tolerance(ref_agg, ref_self, S_agg, S_self, deg, segs, n_scales,
                       dtype):
    """Bound on |result - (ref_agg + ref_self)| per element.

    fp32 roundings, each at most U32 relative to S = S_agg + S_self:
      deg        one fma per edge of the row
      segs       the fixed-order combine of a split row's partial sums
                 (counted as 1 for an unsplit row, as check_spmm does)
      2          acc0 + acc1, and the product with the dst scale
      4 each     (SCALE_U32) for every engine scale vector in the
                 expression: its entries are fp32 pow() results within two
                 ulps of the exact power, so the src vector perturbs every
                 summand, and the dst vector the sum, by 4 * U32 relative.
                 GCN uses two vectors, SAGE one. The SAGE-gcn self term
                 reads the same vector as the aggregate, so its error is
                 the same 4 * U32, relative to S_self — already inside
                 4 * U32 * S.
      2          with a self term: its product and the final add.
    So c = 2 + 4 * n_scales (+ 2 with a self term): 10 for GCN, 6 for
    SAGE mean, 8 for SAGE gcn.

    bf16 results add half a bf16 ulp for every store to bf16: the
    aggregate, and with a self term two more — the self term itself and
    the sum of the two."""
    has_self = ref_self is not None
    c = 2 + SCALE_U32 * n_scales + (2 if has_self else 0)
    S = S_agg + S_self
    ref = ref_agg + ref_self if has_self else ref_agg
    tol = (deg + segs + c).double()[:, None] * U32 * S
    if dtype == torch.bfloat16:
        h = bf16_half_ulp(ref_agg.abs() + tol)
        if has_self:
            h = h + bf16_half_ulp(ref_self.abs() + tol)
            h = h + bf16_half_ulp(ref.abs() + tol + h)
        tol = tol + h
    else:
        assert dtype == torch.float32, dtype
    return ref, tol


def _n_scales(kind: str) -> int:
    return 2 if kind == 'gcn' else 1


def _raise_first(what: str, got: Tensor, ref: Tensor, tol: Tensor, deg, segs):
    o = got.cpu().double()
    assert o.shape == ref.shape, (what, o.shape, ref.shape)
    bad = ~((o - ref).abs() <= tol)
    if bad.any():
        r, f = _first(bad)
        raise AssertionError(
            f'{what}: y[{r}, {f}] = {float(o[r, f])!r}, oracle '
            f'{float(ref[r, f])!r} (tol {float(tol[r, f]):.3e}, deg '
            f'{int(deg[r])}, segs {int(segs[r])}, {got.dtype}); '
            f'{int(bad.sum())} bad of {o.numel()} in '
            f'{int(bad.any(dim=1).sum())} rows')
    return float(((o - ref).abs() / tol.clamp(min=1e-300)).max())


def check_propagated(g, lg, kind: str, agg: str, direction, T: Tensor,
                     got: Tensor, segs: Tensor, what: str = '') -> float:
    """got [I, F]: one rank's propagation of the global T (the rank held
    T[local_to_global[:I]], its peers the rest) against the dense global
    operator. Tolerance: _counted_tolerance. Returns max |err| / tol."""
    I = lg.num_inner
    idx = lg.local_to_global.cpu()[:I]
    ref_agg, ref_self, S_agg, S_self = _operator_parts(g, kind, agg, direction, T)
    indptr = lg.indptr.cpu()
    deg = indptr[1:] - indptr[:-1]
    ref, tol = _counted_tolerance(
        ref_agg[idx], None if ref_self is None else ref_self[idx],
        S_agg[idx], S_self[idx], deg, segs.cpu(), _n_scales(kind), got.dtype)
    return _raise_first(what or 'propagated', got, ref, tol, deg, segs)


def check_aggregate_with_remote(g, lg, kind: str, agg: str, direction,
                                x_local: Tensor, remote: Tensor, got: Tensor,
                                segs: Tensor, what: str = '') -> float:
    """Quantised modes: the rank-local CSR applied to cat(x_local, remote
    exactly as received), scales from the GLOBAL degrees looked up through
    local_to_global, plus the self term. The kernels are deterministic for
    a seed, so a replayed propagate must land inside the same counted
    tolerance as the full-precision check."""
    _, din, dout = _dense(g)
    l2g = lg.local_to_global.cpu()
    I = lg.num_inner
    src, dst, slf = _scale_vectors(kind, agg, direction, din[l2g], dout[l2g])
    x_all = torch.cat([x_local.cpu().double(), remote.cpu().double()], dim=0)
    ref_agg, S_agg, deg = spmm_reference(
        lg.indptr, lg.indices, x_all, src, None if dst is None else dst[:I])
    ref_self = S_self = None
    if slf is not None:
        ref_self = x_all[:I] * slf[:I, None]
        S_self = ref_self.abs()
    ref, tol = _counted_tolerance(
        ref_agg, ref_self, S_agg,
        S_self if S_self is not None else torch.zeros_like(S_agg),
        deg, segs.cpu(), _n_scales(kind), got.dtype)
    return _raise_first(what or 'aggregate', got, ref, tol, deg, segs)


# --------------------------------------------------------------------------
# dequantised remote block
# --------------------------------------------------------------------------

def check_dequantized(true_rows: Tensor, bits: Tensor, got: Tensor,
                      what: str = '') -> float:
    """got [R, F] (fp32 or bf16): the received block; true_rows [R, F]: the
    rows the peers really hold; bits int64 [R] per row.

    Per row: mn/mx of the true row, range = mx - mn, L = 2^bits - 1,
    scale = bf16(L / range), rmin = bf16(mn). The sender stores
    q = clamp(floor((x - rmin) * scale + u), 0, L), u in [0, 1); the
    receiver returns q / scale + rmin. In exact arithmetic:
      - unclamped: q - (x - rmin) * scale lies in (-1, 1), so the error
        is below one step, 1 / scale;
      - low clamp (x < rmin, q = 0): the error is rmin - x <= rmin - mn,
        the bf16 rounding of mn, at most bf16_half_ulp(mn);
      - high clamp (q = L): x - rmin <= range + bf16_half_ulp(mn) and
        L / scale >= range * (1 - 2^-8), since half a bf16 ulp of the
        scale is at most 2^-8 of it: the error is at most
        bf16_half_ulp(mn) + 2^-8 * range.
    The sum of the three covers every element. fp32 evaluation adds
    pack_delta(bits) / scale (a level may flip within pack_delta of a
    boundary, see kernel_oracles.pack_delta) and three roundings on the
    receiver (1 / scale, the product, the sum) relative to at most
    L / scale + |rmin|. A bf16 output adds half a bf16 ulp of the value.
    A constant row (range 0) is sent as scale 0 and comes back as rmin."""
    x = true_rows.cpu().double()
    o = got.cpu().double()
    assert o.shape == x.shape, (what, o.shape, x.shape)
    L = (2.0 ** bits.cpu().double()) - 1
    mn = x.min(dim=1).values
    rng = x.max(dim=1).values - mn
    live = rng > 0
    scale = torch.where(live, L / rng.clamp(min=1e-300), torch.ones_like(rng))
    scale = scale.float().bfloat16().double()
    step = torch.where(live, 1.0 / scale, torch.zeros_like(scale))
    rmin_mag = mn.abs() + bf16_half_ulp(mn)
    delta = torch.tensor([pack_delta(int(b)) for b in bits.tolist()],
                         dtype=torch.float64)
    tol = step + bf16_half_ulp(mn) + 2.0 ** -8 * rng \
        + delta * step + 3 * U32 * (L * step + rmin_mag)
    tol = tol[:, None].expand_as(x)
    if got.dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(x.abs() + tol)
    else:
        assert got.dtype == torch.float32, got.dtype
    bad = ~((o - x).abs() <= tol)
    if bad.any():
        r, f = _first(bad)
        raise AssertionError(
            f'{what or "dequantized"}: remote[{r}, {f}] = {float(o[r, f])!r}, '
            f'true {float(x[r, f])!r} (bound {float(tol[r, f]):.3e}, bits '
            f'{int(bits[r])}, row min {float(mn[r])!r}, range '
            f'{float(rng[r])!r}, {got.dtype}); {int(bad.sum())} bad of '
            f'{o.numel()} in {int(bad.any(dim=1).sum())} rows')
    return float(((o - x).abs() / tol).max())


# --------------------------------------------------------------------------
# shared inputs
# --------------------------------------------------------------------------

N_NODES = 1200


def fwd_bits(gid: Tensor) -> Tensor:
    return torch.tensor(BITS)[gid % 3]


def bwd_bits(gid: Tensor) -> Tensor:
    return torch.tensor(BITS)[(gid // 3) % 3]


_case_cache: dict = {}


def build_case():
    """(g, [LocalGraph] * 3), all on the CPU — do not modify. Every rank
    has >= 100 central and >= 50 marginal rows, receives from both peers
    and has a marginal row split into more than one SpMM segment."""
    if 'g' not in _case_cache:
        from adaqp_amd.graph import random_partitioned_graph, partition_all
        from adaqp_amd.ops.kernels import SEG_EDGES
        g = random_partitioned_graph(N_NODES, 20000, 8, 3, WORLD, seed=21,
                                     cut_frac=0.02, alpha=3.0)
        for name in ('src', 'dst'):        # generated on the GPU when present
            setattr(g, name, getattr(g, name).cpu())
        lgs = partition_all(g, WORLD)
        for lg in lgs:
            assert lg.num_central >= 100 and lg.num_marginal >= 50, \
                (lg.rank, lg.num_central, lg.num_marginal)
            for p in range(WORLD):
                if p != lg.rank:
                    assert lg.recv_splits[p] > 0 and lg.send_splits[p] > 0, \
                        (lg.rank, p, lg.recv_splits, lg.send_splits)
            cnt = (lg.indptr[1:] - lg.indptr[:-1])[lg.num_central:]
            assert int((cnt > SEG_EDGES).sum()) >= 1, \
                f'rank {lg.rank}: no split row in the marginal view'
        _case_cache['g'] = (g, lgs)
    return _case_cache['g']


def case_tensors(F: int, dtype) -> Tuple[Tensor, Tensor]:
    """Global X and G [1200, F] in ``dtype``, identical on every rank:
    unit normal plus a per-row offset in 4..10 (X) / 3..13 (G), so rows are
    well separated and no row minimum is near 0. bf16 cases round here,
    and the oracle reads the rounded values."""
    key = (F, dtype)
    if key not in _case_cache:
        gen = torch.Generator().manual_seed(5000 + F)
        i = torch.arange(N_NODES)
        X = torch.randn(N_NODES, F, generator=gen) + (4 + i % 7).float()[:, None]
        G = torch.randn(N_NODES, F, generator=gen) + (3 + i % 11).float()[:, None]
        _case_cache[key] = (X.to(dtype), G.to(dtype))
    return _case_cache[key]


DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def case_list(dtypes=('fp32',)) -> List[str]:
    """Case ids '<model>/<mode>/<dtype>-F<F>'. bf16 runs F = 24 and F = 22
    (2 mod 4: the SpMM's two-element-per-lane path)."""
    out = []
    for kind, agg in MODELS:
        for mode in MODES:
            for dt in dtypes:
                for F in ((24,) if dt == 'fp32' else (24, 22)):
                    out.append(f'{model_name(kind, agg)}/{mode}/{dt}-F{F}')
    return out


# --------------------------------------------------------------------------
# faults for the sensitivity tests: name -> (case id, check that must fail)
# --------------------------------------------------------------------------

FAULTS: Dict[str, Tuple[str, str]] = {
    'sage_mean_bwd_dst_scale': ('SAGE-mean/Vanilla/fp32-F24', 'propagate-bwd'),
    'marginal_dst_no_base': ('GCN/AdaQP-p/fp32-F24', 'propagate-fwd'),
    'peer_blocks_swapped': ('GCN/Vanilla/fp32-F24', 'fp_exchange-fwd'),
    'sage_gcn_bwd_no_self': ('SAGE-gcn/Vanilla/fp32-F24', 'propagate-bwd'),
    'neighbour_qparams': ('GCN/AdaQP-q/fp32-F24', 'dequantized-fwd'),
}


class _Patch:
    """Install one named fault into adaqp_amd.ops.dist_agg; undo on exit."""

    def __init__(self, name: Optional[str]):
        self.name = name
        self.saved = {}

    def _set(self, attr, fn):
        import adaqp_amd.ops.dist_agg as da
        self.saved[attr] = getattr(da, attr)
        setattr(da, attr, fn)

    def __enter__(self):
        import adaqp_amd.ops.dist_agg as da
        name = self.name
        if name is None:
            return self
        if name == 'sage_mean_bwd_dst_scale':
            orig = da._scales

            def scales(engine, mode):
                if (engine.model_type == DistGNNType.DistSAGE
                        and engine.agg_type == 'mean' and mode == BWD):
                    return None, engine.sage_dst_f, False
                return orig(engine, mode)
            self._set('_scales', scales)
        elif name == 'marginal_dst_no_base':
            def agg(engine, view, x_local, x_remote, src, dst, out=None):
                ds = dst[:view.nrows] if dst is not None else None
                return da.spmm(view, x_local, x_remote, src, ds, out=out)
            self._set('_agg', agg)
        elif name == 'peer_blocks_swapped':
            orig = da._exchange_finish

            def finish(engine, staged, key):
                r = orig(engine, staged, key)
                n = [s for s in engine.graph.recv_splits if s]
                assert len(n) == 2
                return torch.cat([r[n[0]:], r[:n[0]]], dim=0)
            self._set('_exchange_finish', finish)
        elif name == 'sage_gcn_bwd_no_self':
            orig = da._self_term

            def self_term(engine, x_local, mode):
                t = orig(engine, x_local, mode)
                return torch.zeros_like(t) if mode == BWD else t
            self._set('_self_term', self_term)
        elif name == 'neighbour_qparams':
            orig = da.mixed_dequantize

            def dequant(payload, params, plan, out):
                # the first 8-bit node whose wire neighbour has an rmin more
                # than one unit away takes that neighbour's (scale, rmin)
                pos = plan.pos[8].cpu()
                rmin = params.cpu().float()[1::2]
                d = (rmin[pos[:-1]] - rmin[pos[1:]]).abs()
                ok = (pos[1:] == pos[:-1] + 1) & (d > 1.0)
                j = int(torch.nonzero(ok)[0])
                p = int(pos[j])
                params = params.clone()
                params[2 * p:2 * p + 2] = params[2 * p + 2:2 * p + 4]
                return orig(payload, params, plan, out)
            self._set('mixed_dequantize', dequant)
        else:
            raise ValueError(name)
        return self

    def __exit__(self, *exc):
        import adaqp_amd.ops.dist_agg as da
        for attr, fn in self.saved.items():
            setattr(da, attr, fn)
        return False


# --------------------------------------------------------------------------
# the worker: every case on one rank
# --------------------------------------------------------------------------

def _engine(lg, mode: str, kind: str, agg: str, F: int, dtype, device):
    from adaqp_amd.runtime import GraphEngine
    mt = DistGNNType.DistGCN if kind == 'gcn' else DistGNNType.DistSAGE
    engine = GraphEngine(lg, RunMode(mode), mt, msg_dims=[F, F],
                         agg_type=agg, device=device)
    engine.compute_dtype = dtype
    if engine.bit_type.name == 'QUANT':
        gid = lg.local_to_global.cpu()
        assign = {}
        for key in engine.exchange_keys():
            fn = fwd_bits if key.startswith('forward') else bwd_bits
            assign[key] = {p: fn(gid[idx.cpu()])
                           for p, idx in lg.send_idx.items() if idx.numel()}
        engine.set_assignment(assign)
    return engine


def _view_segs(engine) -> Tensor:
    """Segments per row as the engine's path sees them; asserts that the
    full view and the central/marginal views split rows alike, which is
    what makes the two paths sum in the same order."""
    full = segs_per_row(engine.full_view)
    split = torch.cat([segs_per_row(engine.central_view),
                       segs_per_row(engine.marginal_view)])
    assert torch.equal(full, split), 'full and split views segment rows differently'
    assert int((split[engine.graph.num_central:] > 1).sum()) >= 1
    return full


def _run_fp(engine, lg, x, gl, x32):
    """All engine calls of a full-precision case (no checks: a failed
    check must not desynchronise the ranks' collectives)."""
    from adaqp_amd.ops.dist_agg import fp_exchange, propagate, dist_aggregate
    o = {}
    with torch.no_grad():
        o['ex_f'] = fp_exchange(engine, x, f'forward{LAYER}')
        o['ex_b'] = fp_exchange(engine, gl, f'backward{LAYER}')
        o['y_f'] = propagate(engine, x, LAYER, True, FWD)
        o['y_b'] = propagate(engine, gl, LAYER, True, BWD)
        o['y_f2'] = propagate(engine, x, LAYER, True, FWD)
        o['y_b2'] = propagate(engine, gl, LAYER, True, BWD)
    xin = x.clone().requires_grad_(True)
    y = dist_aggregate(xin, engine, LAYER, True)
    y.backward(gl.to(y.dtype))
    o['ag_y'], o['ag_g'] = y.detach(), xin.grad
    if x32 is not None:        # fp32 tensors into a bf16 engine
        xin = x32.clone().requires_grad_(True)
        y = dist_aggregate(xin, engine, LAYER, True)
        y.backward(gl.to(y.dtype))
        o['ag32_y'], o['ag32_g'] = y.detach(), xin.grad
    return {k: v.cpu() for k, v in o.items()}


def _run_qt(engine, lg, x, gl):
    from adaqp_amd.ops.dist_agg import qt_exchange, propagate
    o = {}
    with torch.no_grad():
        for tag, t, mode in (('f', x, FWD), ('b', gl, BWD)):
            key = ('forward' if mode == FWD else 'backward') + str(LAYER)
            engine._rng_counter = SEED_COUNTER
            o['rm_' + tag] = qt_exchange(engine, t, key)
            for rep in ('', '2'):
                engine._rng_counter = SEED_COUNTER
                o[f'y_{tag}{rep}'] = propagate(engine, t, LAYER, True, mode)
    return {k: v.cpu() for k, v in o.items()}


def run_rank(rank: int, device, dtypes=('fp32',), faults=()) -> list:
    """Run every case of ``case_list(dtypes)`` on this rank, then every
    fault in ``faults`` on its own case. Needs a live Communicator of world
    size 3. Returns [(fault | None, case id, check, None | failure text,
    max error / bound where the check has one)]; each check is caught on
    its own so one failure does not mask the rest."""
    g, lgs = build_case()
    import copy
    lg = copy.deepcopy(lgs[rank])
    l2g = lg.local_to_global.cpu()
    I = lg.num_inner
    records = []
    vanilla: dict = {}

    def one_case(cid: str, fault: Optional[str]):
        name, mode, rest = cid.split('/')
        kind, agg = next(m for m in MODELS if model_name(*m) == name)
        dt, F = rest.split('-F')
        dtype, F = DTYPES[dt], int(F)
        X, G = case_tensors(F, dtype)
        x = X[l2g[:I]].to(device)
        gl = G[l2g[:I]].to(device)
        x32 = x.float() if dtype == torch.bfloat16 else None
        engine = _engine(lg, mode, kind, agg, F, dtype, device)
        quant = engine.bit_type.name == 'QUANT'
        with _Patch(fault):
            o = _run_qt(engine, lg, x, gl) if quant else _run_fp(engine, lg, x, gl, x32)
        if device.type == 'cuda':
            torch.cuda.synchronize()

        def check(label, fn):
            try:
                r = fn()
                records.append((fault, cid, label, None,
                                r if isinstance(r, float) else None))
            except AssertionError as e:
                records.append((fault, cid, label, f'rank {rank}: {e}', None))

        segs = None

        def get_segs():
            nonlocal segs
            if segs is None:
                segs = _view_segs(engine)
            return segs
        check('segments', get_segs)
        if segs is None:
            segs = segs_per_row(engine.full_view)

        def eq(a, b, msg):
            def f():
                assert a.dtype == b.dtype and torch.equal(a, b), msg
            return f

        for tag, T, mode_, d in (('fwd', X, FWD, 'f'), ('bwd', G, BWD, 'b')):
            yk = o['y_' + d]
            if quant:
                bits = (fwd_bits if d == 'f' else bwd_bits)(l2g[I:])
                check(f'dequantized-{tag}', lambda: check_dequantized(
                    T[l2g[I:]], bits, o['rm_' + d], f'{cid} {tag}'))
                check(f'aggregate-{tag}', lambda: check_aggregate_with_remote(
                    g, lg, kind, agg, mode_, T[l2g[:I]], o['rm_' + d], yk,
                    segs, f'{cid} {tag}'))
                check(f'dtype-{tag}', lambda: _assert_dtype(
                    (o['rm_' + d], yk), dtype))
            else:
                check(f'fp_exchange-{tag}', eq(
                    o['ex_' + d], T[l2g[I:]],
                    f'{cid}: fp_exchange {tag} is not T[local_to_global[I:]]'))
                check(f'propagate-{tag}', lambda: check_propagated(
                    g, lg, kind, agg, mode_, T, yk, segs, f'{cid} {tag}'))
            # same call twice: a missing stream wait shows as a difference
            check(f'replay-{tag}', eq(yk, o[f'y_{d}2'],
                                      f'{cid}: {tag} differs between two calls'))
        if not quant:
            check('dist_aggregate-fwd', lambda: check_propagated(
                g, lg, kind, agg, FWD, X, o['ag_y'], segs, f'{cid} autograd fwd'))
            check('dist_aggregate-grad', lambda: check_propagated(
                g, lg, kind, agg, BWD, G, o['ag_g'], segs, f'{cid} autograd grad'))
            check('dist_aggregate-dtype', lambda: _assert_dtype(
                (o['ag_y'], o['ag_g']), dtype))
            if x32 is not None:
                check('dist_aggregate-fp32in-fwd', lambda: check_propagated(
                    g, lg, kind, agg, FWD, X, o['ag32_y'], segs,
                    f'{cid} fp32-in fwd'))
                check('dist_aggregate-fp32in-grad', lambda: check_propagated(
                    g, lg, kind, agg, BWD, G, o['ag32_g'].bfloat16(), segs,
                    f'{cid} fp32-in grad'))
                check('dist_aggregate-fp32in-dtype', lambda: (
                    _assert_dtype((o['ag32_y'],), dtype),
                    _assert_dtype((o['ag32_g'],), torch.float32)))
            if fault is None and mode == 'Vanilla':
                vanilla[(name, rest)] = (o['y_f'], o['y_b'])
            if fault is None and mode == 'AdaQP-p':
                vf, vb = vanilla[(name, rest)]
                check('parity-fwd', eq(o['y_f'], vf,
                                       f'{cid}: forward differs from Vanilla'))
                check('parity-bwd', eq(o['y_b'], vb,
                                       f'{cid}: backward differs from Vanilla'))

    for cid in case_list(dtypes):
        one_case(cid, None)
    for fault in faults:
        one_case(FAULTS[fault][0], fault)
    return records


def _assert_dtype(tensors, dtype):
    for t in tensors:
        assert t.dtype == dtype, (t.dtype, dtype)


def worker_main(rank: int, port: int, device_name: str, dtypes, faults, q):
    """Process entry: one rank of world size 3 over gloo."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(WORLD), LOCAL_RANK='0')
    from adaqp_amd.comm import Communicator
    comm = Communicator(backend='gloo', timeout_s=120)
    try:
        device = torch.device(device_name)
        if device.type == 'cuda':
            from adaqp_amd.ops.kernels import native
            native()
            torch.cuda.set_device(device)
            comm.device = device
        q.put((rank, run_rank(rank, device, dtypes, faults)))
    finally:
        Communicator.shutdown()


def spawn_workers(port: int, device_name: str, dtypes, faults=(),
                  join_s: float = 240.0) -> Dict[int, list]:
    """Start the three ranks once; {rank: records}. A rank that is still
    alive after ``join_s`` or exits non-zero fails the caller, no retry."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=worker_main,
                         args=(r, port, device_name, tuple(dtypes),
                               tuple(faults), q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    # drain before joining: a child blocks in put() until its records are read
    out: Dict[int, list] = {}
    import time
    deadline = time.monotonic() + join_s
    while len(out) < WORLD and time.monotonic() < deadline:
        if not q.empty():
            rank, recs = q.get()
            out[rank] = recs
        elif not any(p.is_alive() for p in procs):
            break
        else:
            time.sleep(0.05)
    hung = False
    for p in procs:
        p.join(max(deadline - time.monotonic(), 1.0))
        if p.is_alive():
            hung = True
    if hung:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
        raise AssertionError('aggregation worker hung')
    while not q.empty():
        rank, recs = q.get()
        out[rank] = recs
    codes = [p.exitcode for p in procs]
    assert codes == [0] * WORLD, f'worker exit codes {codes}'
    assert sorted(out) == list(range(WORLD)), sorted(out)
    return out


def failures(results: Dict[int, list], cid: str, fault: Optional[str] = None):
    """[(rank, check, text)] of the failed checks of one case, and the
    number of checks that ran for it."""
    bad, n = [], 0
    for rank, recs in results.items():
        for f, c, label, text, _ in recs:
            if f == fault and c == cid:
                n += 1
                if text is not None:
                    bad.append((rank, label, text))
    return bad, n
