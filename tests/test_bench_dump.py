"""bench.py --dump-outputs (CPU): the files a dump writes, their dtype, the size cap and that the
sample of a capped dump is a fixed one. The tensors here live on the CPU; the GPU run of the
option is tests/test_gpu_bench_plain.py."""
import os

import numpy as np
import pytest
import torch

import bench


def _tensors(shapes, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dtype) for s in shapes]


def test_dump_whole_when_small(tmp_path):
    shapes = [(5, 7), (3,), (2, 3, 4)]
    outs, res = _tensors(shapes, 1), _tensors(shapes, 2, torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "d"), outs, res)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(
        [f"out_{i:04d}.npy" for i in range(3)] + [f"residual_{i:04d}.npy" for i in range(3)])
    for i in range(3):
        o = np.load(tmp_path / "d" / f"out_{i:04d}.npy")
        r = np.load(tmp_path / "d" / f"residual_{i:04d}.npy")
        assert o.dtype == np.float32 and r.dtype == np.float32
        assert np.array_equal(o, outs[i].reshape(-1).numpy())
        assert np.array_equal(r, res[i].reshape(-1).float().numpy())


def test_dump_capped_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 1000)  # 1000 float32 of outputs, 1000 of residuals
    shapes = [(100, 30), (7,), (50, 40)]
    outs, res = _tensors(shapes, 3), _tensors(shapes, 4)
    bench.dump_outputs(str(tmp_path / "a"), outs, res)
    bench.dump_outputs(str(tmp_path / "b"), outs, res)
    total = 0
    for name in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.size >= 1
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 8 * 1000 + 4 * 2 * len(shapes)  # the cap, plus the one element a tiny tensor keeps
    # every sampled value is an element of its tensor, outputs and residuals at the same indices
    o, r = np.load(tmp_path / "a" / "out_0000.npy"), np.load(tmp_path / "a" / "residual_0000.npy")
    flat_o, flat_r = outs[0].reshape(-1).numpy(), res[0].reshape(-1).numpy()
    idx = [int(np.flatnonzero(flat_o == v)[0]) for v in o]
    assert np.array_equal(flat_r[idx], r)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_parse_rejects_counts_it_cannot_time(argv, monkeypatch, capsys):
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.parse()
    assert e.value.code == 2 and "--steps must be at least 1" in capsys.readouterr().err
