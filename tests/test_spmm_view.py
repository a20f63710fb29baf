"""SpmmView segmentation invariants (the GPU kernel's work-item layout)."""
import torch

from adaqp_amd.ops.kernels import SpmmView, _auto_seg
SEG_EDGES = _auto_seg(0, 1)  # low-degree auto default (test graphs avg deg ~15)
from adaqp_amd.runtime.timer import Timer
from adaqp_amd.runtime.recorder import Recorder


def _random_csr(rows, max_deg, seed, hub=None):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, max_deg, (rows,), generator=g)
    if hub is not None:
        deg[0] = hub
    indptr = torch.zeros(rows + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.randint(0, rows, (int(indptr[-1]),), generator=g)
    return indptr, indices


def test_partial_slots_partition_split_rows():
    """Every segment of a split row owns exactly one partial-sum slot, a
    row's slots are the contiguous range part_ptr names for it, in segment
    order, and unsplit segments own none — in both work-item layouts."""
    rows = 120
    indptr, indices = _random_csr(rows, 30, 5, hub=4 * SEG_EDGES + 9)
    for cb in (0, 16):
        v = SpmmView(indptr, indices, 0, rows, col_block=cb)
        assert v.n_part >= 5 and int(v.part_ptr[0]) == 0
        assert int(v.part_ptr[-1]) == v.n_part
        assert v.part_ptr.numel() == v.zero_rows.numel() + 1
        assert ((v.seg_part >= 0) == v.seg_multi.bool()).all()
        used = v.seg_part[v.seg_part >= 0]
        assert sorted(used.tolist()) == list(range(v.n_part))
        for j, r in enumerate(v.zero_rows.tolist()):
            mine = v.seg_part[(v.seg_row == r) & (v.seg_part >= 0)].tolist()
            assert mine == list(range(int(v.part_ptr[j]),
                                      int(v.part_ptr[j + 1])))


def test_segments_cover_all_edges_exactly():
    for seed in range(3):
        rows = 200
        indptr, indices = _random_csr(rows, 30, seed, hub=5 * SEG_EDGES + 3)
        v = SpmmView(indptr, indices, 0, rows)
        # every edge covered exactly once, in order, within its row
        covered = torch.zeros(int(indptr[-1]), dtype=torch.int32)
        for i in range(v.seg_row.numel()):
            r = int(v.seg_row[i])
            e0, e1 = int(v.seg_e0[i]), int(v.seg_e1[i])
            assert indptr[r] <= e0 <= e1 <= indptr[r + 1]
            assert e1 - e0 <= SEG_EDGES
            covered[e0:e1] += 1
        assert (covered == 1).all()
        # multi flag consistent with zero_rows
        multi_rows = set(v.zero_rows.tolist())
        for i in range(v.seg_row.numel()):
            assert bool(v.seg_multi[i]) == (int(v.seg_row[i]) in multi_rows)
        # rows with 0 edges still get one (empty) segment -> output written
        zero_deg = (indptr[1:] == indptr[:-1]).sum()
        assert v.seg_row.numel() >= rows
        assert v.seg_row.numel() == rows + sum(
            max((int(indptr[r + 1] - indptr[r]) + SEG_EDGES - 1) // SEG_EDGES, 1) - 1
            for r in range(rows))


def test_timer_rollup():
    t = Timer(enabled=True, cuda=False)
    with t.record('forward0_exchange'):
        pass
    with t.record('forward0_quant'):
        pass
    with t.record('forward0_central_aggregation'):
        pass
    with t.record('grad_reduce'):
        pass
    row = t.epoch_rollup()
    assert len(row) == 6
    assert all(v >= 0 for v in row)
    assert t.records == {}          # cleared per epoch


def test_recorder_best(tmp_path):
    r = Recorder()
    r.add({'train': 0.5, 'val': 0.6, 'test': 0.55})
    r.add({'train': 0.7, 'val': 0.8, 'test': 0.75})
    r.add({'train': 0.9, 'val': 0.7, 'test': 0.95})
    b = r.best()
    assert b['epoch'] == 1
    assert abs(b['val'] - 0.8) < 1e-6 and abs(b['test'] - 0.75) < 1e-6
    r.save(str(tmp_path), 'x')
    assert (tmp_path / 'x_metrics.txt').exists()
    assert (tmp_path / 'x_val_curve.pt').exists()


def test_blocked_view_covers_all_edges():
    """col_block mode permutes edges; coverage must stay exact and the
    CPU reference result (via edge expansion) must be preserved."""
    for seed in range(2):
        rows = 150
        indptr, indices = _random_csr(rows, 40, seed, hub=2 * SEG_EDGES + 5)
        v = SpmmView(indptr, indices, 0, rows, col_block=16)
        # same multiset of (row, col) pairs
        orig = []
        for r in range(rows):
            for e in range(int(indptr[r]), int(indptr[r + 1])):
                orig.append((r, int(indices[e])))
        perm = []
        for i in range(v.seg_row.numel()):
            r = int(v.seg_row[i])
            for e in range(int(v.seg_e0[i]), int(v.seg_e1[i])):
                perm.append((r, int(v.indices[e])))
        assert sorted(orig) == sorted(perm)
        # single-segment rows store plainly; all others zeroed+atomic
        from collections import Counter
        per_row = Counter(int(r) for r in v.seg_row)
        zr = set(v.zero_rows.tolist())
        for r in range(rows):
            if per_row.get(r, 0) == 1:
                assert r not in zr
            else:
                assert r in zr
