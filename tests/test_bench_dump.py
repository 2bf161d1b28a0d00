"""bench.py --dump-outputs on the CPU (host tensors in place of the step's device buffers): the
files hold the last step's float64 audio and its int16 conversion as float32, whole when they
fit the budget, else the same seeded sample of rows on every run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _measured(world, B, T):
    import torch

    import bench
    from areafunctionsynthesis_amd import sharding
    m = bench.Measured()
    m.T = T
    m.out_dev = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (B, T)))
    m.pcm = sharding.PcmGather(lambda x, o: o.copy_((x * 32767).to(torch.int16)), (B, T), world, 0, bench._NoGather())
    for root in m.pcm.roots:
        if root is not None:
            root.zero_()
    for _ in range(3):  # (the last step's slot is the one dumped)
        m.pcm.submit(m.out_dev)
    return m


@pytest.mark.parametrize("world", (1, 2))
def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch, world):
    import bench
    B, T = 50, 1000
    m = _measured(world, B, T)
    audio = m.out_dev.numpy()
    bench.dump_outputs(str(tmp_path / "whole"), m)
    a, p = np.load(tmp_path / "whole" / "audio.npy"), np.load(tmp_path / "whole" / "pcm.npy")
    assert a.dtype == np.float64 and p.dtype == np.float32
    assert np.array_equal(a, audio) and p.shape == (world * B, T)
    if world == 1:
        assert np.array_equal(p, (audio * 32767).astype(np.int16))
    # above the budget: 7 rows of each, the same ones on every run, rows of the output itself
    monkeypatch.setattr(bench, "DUMP_BYTES", 12 * T * 7)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), m)
    a1, a2 = np.load(tmp_path / "s1" / "audio.npy"), np.load(tmp_path / "s2" / "audio.npy")
    p1 = np.load(tmp_path / "s1" / "pcm.npy")
    assert a1.shape == (7, T) and p1.shape == (7, T) and a1.nbytes + p1.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(a1, a2) and np.array_equal(p1, np.load(tmp_path / "s2" / "pcm.npy"))
    rows = [int(np.flatnonzero((audio == r).all(axis=1))[0]) for r in a1]
    assert rows == sorted(set(rows))
    # utterances longer than the budget: the first samples of one row
    monkeypatch.setattr(bench, "DUMP_BYTES", 12 * 300)
    bench.dump_outputs(str(tmp_path / "cut"), m)
    assert np.load(tmp_path / "cut" / "audio.npy").shape == (1, 300)
