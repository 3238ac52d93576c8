"""bench.py --dump-outputs: the files a run writes (no GPU: dump_outputs reads
the env's tensors wherever they live, so a stand-in with CPU tensors serves)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402


class _Env:
    """The attributes of CarlaBEVVectorEnv that dump_outputs reads."""

    def __init__(self, n, S, seed):
        g = torch.Generator().manual_seed(seed)
        self.num_envs, self.S = n, S
        self._frames = torch.randint(0, 9, (n, S, S), dtype=torch.uint8, generator=g)
        self.reward = torch.rand(n, dtype=torch.float64, generator=g)
        self.term = torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g)
        self.trunc = torch.zeros(n, dtype=torch.uint8)
        self.cause = torch.randint(0, 5, (n,), dtype=torch.int32, generator=g)
        self.info = torch.rand((n, 16), dtype=torch.float32, generator=g)

    def frames(self):
        return self._frames


@pytest.mark.parametrize("n,S", [(5, 128), (700, 128), (150, 256)])  # all envs; a 512-env sample; a 128-env sample
def test_dump_outputs_files(tmp_path, n, S):
    env = _Env(n, S, seed=n)
    shapes = bench.dump_outputs(env, str(tmp_path / "a"))
    bench.dump_outputs(env, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"{k}.npy" for k in shapes)
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), name
        assert list(a.shape) == shapes[name[:-4]]
        assert np.array_equal(a, b), name  # the same sample of envs every time
        total += a.nbytes
    assert total <= 64 << 20
    k = min(n, bench.DUMP_FRAME_BYTES // (4 * S * S))
    ids = np.load(tmp_path / "a" / "frames_env_ids.npy").astype(np.int64)
    assert ids.shape == (k,) and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < n
    f = env.frames().numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "frames.npy"), f[ids].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "frames_sum.npy"), f.reshape(n, -1).sum(axis=1, dtype=np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "reward.npy"), env.reward.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "terminated.npy"), env.term.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "cause.npy"), env.cause.numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "comfort.npy"), env.info.numpy())
