"""The driver contract: bench.py must run under torch.distributed.run
with N>1 (one rank per device — CPU here) and print one valid JSON line
with the required fields."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(nproc, extra):
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           f'--nproc-per-node={nproc}', '--master-addr', '127.0.0.1',
           '--master-port', '29520', 'bench.py', '--cpu',
           '--gpus', str(nproc), '--steps', '2', '--warmup', '1',
           '--scale', '0.002'] + extra
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_json_contract_2rank(tmp_path):
    d = json.loads(json.dumps(_run_bench(
        2, ['--part-dir', str(tmp_path / 'parts'), '--full'])))
    assert d['n_gpus'] == 2
    assert d['steps'] == 2 and d['warmup'] == 1
    assert d['higher_is_better'] is False
    assert d['scaling'] == 'strong'
    assert d['unit'] == 's/epoch'
    assert d['value'] > 0 and abs(d['ms_per_step'] - d['value'] * 1000) < 1e-6
    assert d['dtype'] == 'fp32'
    assert 'synthetic' in d['data']
    assert 'ogbn-products' in d['metric']
    assert 0.0 <= d['config']['test_acc'] <= 1.0


def test_bench_json_contract_1rank_defaults(tmp_path):
    cmd = [sys.executable, 'bench.py', '--cpu', '--steps', '2', '--warmup', '1',
           '--scale', '0.002', '--part-dir', str(tmp_path / 'parts')]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][0])
    assert d['n_gpus'] == 1
    # a plain run skips the evaluation pass; --full fills test_acc
    assert d['config']['test_acc'] is None


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed epoch's results as float .npy
    files, identical from run to run (same seeded inputs; the CPU path has
    no atomics), within the 64 MB budget."""
    import numpy as np
    dumps = []
    for tag in ('a', 'b'):
        out_dir = tmp_path / tag
        cmd = [sys.executable, 'bench.py', '--cpu', '--steps', '2',
               '--warmup', '1', '--scale', '0.002',
               '--part-dir', str(tmp_path / 'parts'),
               '--dump-outputs', str(out_dir)]
        out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([l for l in out.stdout.splitlines()
                        if l.startswith('{')][0])
        assert d['steps'] == 2 and d['ms_per_step'] > 0
        dumps.append({p.name: np.load(p) for p in out_dir.glob('*.npy')})
    a, b = dumps
    assert {'loss.npy', 'logits.npy'} <= set(a) and set(a) == set(b)
    assert any(k.startswith('grad_') for k in a)
    assert any(k.startswith('param_') for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.isfinite(v).all(), k
        assert np.array_equal(v, b[k]), k
    assert a['logits.npy'].shape[1] == 47      # ogbn-products classes


def test_bench_dump_outputs_2rank_shares_budget(tmp_path):
    """With N>1 ranks each rank writes its loss and its share of the
    logits sample; the weights and reduced gradients, equal on all ranks,
    are written once."""
    import numpy as np
    out_dir = tmp_path / 'dump'
    _run_bench(2, ['--part-dir', str(tmp_path / 'parts'),
                   '--dump-outputs', str(out_dir)])
    files = {p.name: np.load(p) for p in out_dir.glob('*.npy')}
    for r in (0, 1):
        assert files[f'loss_rank{r}.npy'].shape == (1,)
        assert 0 < files[f'logits_rank{r}.npy'].shape[0] \
            <= 65536 // 2             # bench.DUMP_LOGIT_ROWS / ranks
    assert not any('rank' in k for k in files
                   if k.startswith(('param_', 'grad_')))
    assert any(k.startswith('param_') for k in files)
    assert all(np.isfinite(v).all() for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64 * 2 ** 20


def test_bench_adaptive_scheme_2rank(tmp_path):
    d = _run_bench(2, ['--part-dir', str(tmp_path / 'parts'),
                       '--assign-scheme', 'adaptive'])
    assert d['config']['mode'] == 'AdaQP'
