"""bench.py driver-contract guards. Without a GPU: the module imports
cleanly, the argument surface matches the driver's launch line, the output
dump is a fixed float32 sample, and a GPU-less invocation fails loudly (no
silent CPU benchmark). With one: a tiny plain run end to end."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_args_defaults():
    sys.path.insert(0, REPO)
    import bench
    old = sys.argv
    try:
        sys.argv = ['bench.py']
        a = bench.parse_args()
    finally:
        sys.argv = old
    # the driver runs `python bench.py --gpus N --steps K --warmup W`
    assert a.gpus == 1 and a.steps >= 1 and a.warmup >= 1
    assert tuple(a.chunk_size) == (512, 512, 512)       # config-2 workload
    assert tuple(a.patch_size) == (20, 256, 256)
    assert tuple(a.overlap) == (4, 64, 64)
    assert a.batch_size == 12
    assert a.dtype == 'float32'


def test_driver_flags_accepted():
    sys.path.insert(0, REPO)
    import bench
    old = sys.argv
    try:
        sys.argv = ['bench.py', '--gpus', '8', '--steps', '3',
                    '--warmup', '1']
        a = bench.parse_args()
    finally:
        sys.argv = old
    assert (a.gpus, a.steps, a.warmup) == (8, 3, 1)


def test_full_and_dump_flags():
    sys.path.insert(0, REPO)
    import bench
    old = sys.argv
    try:
        sys.argv = ['bench.py', '--gpus', '1', '--steps', '2',
                    '--warmup', '1']
        a = bench.parse_args()
        # a plain run measures nothing but the headline figure
        assert a.full is False and a.dump_outputs is None
        sys.argv += ['--full', '--dump-outputs', 'somewhere']
        a = bench.parse_args()
        assert a.full is True and a.dump_outputs == 'somewhere'
        sys.argv = ['bench.py', '--steps', '0']
        with pytest.raises(SystemExit):
            bench.parse_args()
    finally:
        sys.argv = old


class _Out:
    def __init__(self, array):
        self.array = array


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """--dump-outputs writes float32 arrays: the whole output when it fits
    the cap, otherwise the smallest-stride subsample that does, plus the
    voxels at fixed seeded indices — identical from call to call."""
    sys.path.insert(0, REPO)
    import bench
    import numpy as np
    t = torch.arange(3 * 7 * 9 * 11, dtype=torch.float32) \
        .reshape(3, 7, 9, 11).to(torch.bfloat16)
    ref = t.to(torch.float32).numpy()

    info = bench.dump_outputs(str(tmp_path / 'a'), _Out(t))
    assert info['stride'] == 1 and info['shape'] == [3, 7, 9, 11]
    full = np.load(tmp_path / 'a' / 'output_strided.npy')
    assert full.dtype == np.float32
    np.testing.assert_array_equal(full, ref)
    sample = np.load(tmp_path / 'a' / 'output_sample.npy')
    assert sample.dtype == np.float32 and sample.shape == (ref.size,)
    idx = np.sort(np.random.RandomState(0).randint(0, ref.size,
                                                   size=ref.size))
    np.testing.assert_array_equal(sample, ref.ravel()[idx])

    # a cap smaller than the array forces a stride; the sample shrinks too
    cap = ref[:, ::2, ::2, ::2].nbytes
    monkeypatch.setattr(bench, 'DUMP_STRIDED_BYTES', cap)
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_VOXELS', 100)
    info = bench.dump_outputs(str(tmp_path / 'b'), _Out(t))
    assert info['stride'] == 2
    sub = np.load(tmp_path / 'b' / 'output_strided.npy')
    np.testing.assert_array_equal(sub, ref[:, ::2, ::2, ::2])
    assert sub.nbytes <= cap < ref.nbytes
    s1 = np.load(tmp_path / 'b' / 'output_sample.npy')
    bench.dump_outputs(str(tmp_path / 'c'), _Out(t))
    s2 = np.load(tmp_path / 'c' / 'output_sample.npy')
    assert s1.shape == (100,)
    np.testing.assert_array_equal(s1, s2)


@pytest.mark.gpu
def test_plain_run_dumps_last_step_output(tmp_path, golden):
    """One tiny plain run of the real script (identity engine): the result
    line carries the headline fields, the --full-only fields are null, and
    the dumped output is the masked identity inference of the deterministic
    input, i.e. input/255 in every channel at the 1e-5 identity pin."""
    import json
    import numpy as np
    _, arrays = golden
    out_dir = tmp_path / 'dump'
    r = subprocess.run(
        [sys.executable, 'bench.py', '--gpus', '1', '--steps', '2',
         '--warmup', '1', '--engine', 'identity',
         '--chunk-size', '20', '68', '72', '--patch-size', '10', '32', '32',
         '--overlap', '2', '8', '8', '--batch-size', '3',
         '--dump-outputs', str(out_dir)],
        capture_output=True, text=True, cwd=REPO,
        env=dict(os.environ, PYTHONPATH=REPO), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['metric'] == 'output_voxels_per_sec'
    assert res['unit'] == 'voxels/s' and res['higher_is_better'] is True
    assert res['dtype'] == 'f32' and res['steps'] == 2
    assert res['ms_per_step'] > 0
    assert res['value'] == pytest.approx(
        20 * 68 * 72 / (res['ms_per_step'] / 1e3), rel=1e-9)
    assert res['full'] is False
    assert res['roofline'] is None and res['cpu_baseline'] is None
    got = np.load(out_dir / 'output_strided.npy')
    assert got.dtype == np.float32 and got.shape == (3, 20, 68, 72)
    want = arrays['sin_20x68x72_u8'].astype(np.float32) / 255.0
    np.testing.assert_allclose(got, np.broadcast_to(want, got.shape),
                               rtol=0, atol=1e-5)
    sample = np.load(out_dir / 'output_sample.npy')
    idx = np.sort(np.random.RandomState(0).randint(0, got.size,
                                                   size=got.size))
    np.testing.assert_array_equal(sample, got.ravel()[idx])


@pytest.mark.skipif(torch.cuda.is_available(), reason='GPU present')
def test_no_silent_cpu_fallback():
    r = subprocess.run([sys.executable, 'bench.py', '--steps', '1'],
                       capture_output=True, text=True, cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO), timeout=300)
    assert r.returncode != 0
    assert 'requires a GPU' in (r.stderr + r.stdout)
