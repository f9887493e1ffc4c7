"""GymVectorAdapter.render_batch over an engine WITHOUT render_frames (the oracle-backed engine of
tests/test_gym_vector.py): the frames of the selected sub-envs, stacked from single render_frame calls.  No GPU."""
import numpy as np
import pytest

from test_gym_vector import OracleEngine

from procgen2_amd.gym_vector import GymVectorAdapter


@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_render_batch_stacks_the_single_frames(output):
    env = GymVectorAdapter(OracleEngine("maze", 3), output=output, render_mode="rgb_array", render_size=(96, 80))
    assert not hasattr(env.engine, "render_frames")
    env.reset()
    frames = env.render_batch()
    if output == "torch":
        import torch
        assert isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8
        frames = frames.numpy()
    assert frames.shape == (3, 80, 96, 3) and frames.dtype == np.uint8
    assert np.array_equal(frames, np.stack([env.render(index=k) for k in range(3)]))
    some = env.render_batch([2, 0, 2])
    some = some.numpy() if output == "torch" else some
    assert np.array_equal(some, frames[[2, 0, 2]])
    assert tuple(env.render_batch([]).shape) == (0, 80, 96, 3)
    env.close()


def test_render_batch_is_none_without_rgb_array_mode():
    env = GymVectorAdapter(OracleEngine("maze", 2), output="numpy")
    env.reset()
    assert env.render_batch() is None
    env.close()
