"""bench.py's host side without a device: the options of a plain run and the files --dump-outputs writes."""
import os
import sys

import numpy as np
import pytest

import bench    # the repository root is on sys.path (conftest.py)


def parse(argv, monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    return bench.parse()


def test_a_plain_run_is_not_a_full_one(monkeypatch):
    a = parse(['--gpus', '1', '--steps', '7', '--warmup', '3'], monkeypatch)
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs == ''
    a = parse(['--steps', '2', '--full', '--dump-outputs', 'out'], monkeypatch)
    assert a.full and a.dump_outputs == 'out'
    with pytest.raises(SystemExit):
        parse(['--steps', '0'], monkeypatch)


def test_dump_writes_the_factors_whole_when_they_fit(tmp_path):
    rng = np.random.RandomState(0)
    W, T = rng.rand(1000, 5), rng.rand(5, 300)
    bench.dump_outputs(str(tmp_path), W, T)
    assert sorted(os.listdir(str(tmp_path))) == ['T.npy', 'W.npy']
    assert np.array_equal(np.load(str(tmp_path / 'W.npy')), W) and np.array_equal(np.load(str(tmp_path / 'T.npy')), T)


def test_dump_samples_rows_of_a_large_W_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 200000)
    rng = np.random.RandomState(1)
    W, T = rng.rand(5000, 8), rng.rand(8, 100)
    for sub in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / sub), W, T)
    names = sorted(os.listdir(str(tmp_path / 'a')))
    assert names == ['T.npy', 'W_sample.npy', 'W_sample_rows.npy']
    got = {n: np.load(str(tmp_path / 'a' / n)) for n in names}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BYTES
    rows = got['W_sample_rows.npy'].astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0) and rows[-1] < W.shape[0]
    assert np.array_equal(got['W_sample.npy'], W[rows]) and np.array_equal(got['T.npy'], T)
    for n in names:
        assert np.array_equal(np.load(str(tmp_path / 'b' / n)), got[n])
