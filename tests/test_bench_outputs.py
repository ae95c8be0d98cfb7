"""bench.py's ``--dump-outputs`` and ``--full``.  CPU: the dump's sampling and
size cap.  GPU: a small plain run writes exactly what the same steps of the
resident sim give in this process, and carries none of the secondary lines;
``--full`` brings them back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, 'bench.py')
HEADLINE_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY_KEYS = ('cpu_baseline', 'speedup_vs_cpu', 'variants', 'dropin_detect', 'asas_update')
SMALL = ['--gpus', '1', '--n', '3000', '--settle', '2', '--warmup', '2', '--steps', '3']


def import_bench():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import bench
    return bench


def test_dump_sample_is_fixed_sorted_and_exact():
    bench = import_bench()
    a = np.arange(1000, dtype=np.int32)
    s = bench.dump_sample(a, 100)
    assert s.dtype == np.float64 and s.shape == (100,)
    assert np.all(np.diff(s) > 0)                              # ascending indices, no repeats
    assert np.array_equal(s, bench.dump_sample(a.copy(), 100))   # the same choice every time
    b = np.linspace(0.0, 1.0, 1000)
    assert np.array_equal(bench.dump_sample(b, 100), b[s.astype(np.int64)])   # by length alone
    assert np.array_equal(bench.dump_sample(a, 1000), a)       # short enough: whole
    assert bench.dump_sample(np.ones(3, np.float32), 8).dtype == np.float32
    assert bench.dump_sample(np.array([True, False]), 8).dtype == np.float64
    assert bench.dump_sample(np.ones((2, 3)), 8).shape == (6,)


def test_dump_outputs_keeps_to_its_size_cap(tmp_path, monkeypatch):
    bench = import_bench()
    assert bench.DUMP_MAX_BYTES <= 64 * 1000 * 1000
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4000)
    arrays = dict(big=np.arange(5000.0), small=np.arange(7, dtype=np.uint8), ints=np.arange(900, dtype=np.int32))
    done = bench.dump_outputs(str(tmp_path / 'out'), arrays)
    got = {k: np.load(str(tmp_path / 'out' / (k + '.npy'))) for k in arrays}
    assert sum(v.nbytes for v in got.values()) <= 4000
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got['small'], arrays['small'])
    assert done == dict(big=[166, 5000], small=[7, 7], ints=[166, 900])
    assert set(got['big']) <= set(arrays['big'])


def run_bench(args):
    e = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE')}
    r = subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_sims_last_step(tmp_path):
    from bluesky_amd import _lib, resident, synth
    out = str(tmp_path / 'dump')
    d = run_bench(SMALL + ['--dump-outputs', out])
    assert all(k in d for k in HEADLINE_KEYS)
    assert d['steps'] == 3 and d['ms_per_step'] > 0 and d['full'] is False
    assert d['value'] == pytest.approx(3000.0 * 3000.0 / (d['ms_per_step'] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY_KEYS if k in d]
    # the same 2 + 2 + 3 steps here, on a context of their own
    t = synth.workload('box100k', n=3000, seed=7)
    c = _lib.Context(0)
    try:
        sim = resident.ResidentSim(resident.initial_state(t), resident.params(cd_every=1), ctx=c)
        sim.step(7)
        state, st = sim.read(), sim.stats()
        pairs = c.fetch_pairs(st['n_conf'], st['n_los'])
    finally:
        c.close()
    exp = {'state_' + k: v for k, v in state.items()}
    exp.update(('pairs_' + k, v) for k, v in pairs.items() if v is not None)
    assert st['n_conf'] > 0                                    # the pair arrays are not empty
    assert sorted(os.listdir(out)) == sorted(k + '.npy' for k in exp)
    assert sorted(d['dumped_outputs']['elements']) == sorted(exp)
    for k, v in exp.items():
        got = np.load(os.path.join(out, k + '.npy'))
        assert got.dtype == np.float64, k
        assert got.tobytes() == np.asarray(v, dtype=np.float64).tobytes(), k
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_full_run_carries_the_secondary_lines():
    d = run_bench(SMALL + ['--full', '--workload', 'box10k', '--cpu-rows', '64'])
    assert all(k in d for k in HEADLINE_KEYS) and d['full'] is True
    assert d['cpu_baseline']['value'] > 0 and d['speedup_vs_cpu'] > 0
    assert {'reference_cadence', 'candidate_reuse', 'geo_matrix'} <= set(d['variants'])
    assert d['dropin_detect']['n'] == 3000
