"""CPU: the host side of batched sampling chains - shard-to-group splitting, the generate CLI's chains_per_gpu, the
arguments generate_samples refuses, the per-row stream table of the sampler, and the exact-fp32-only refusal of
SimpleUnet3D.set_batch_invariant."""
import pytest
import torch

import holo_diffusion_amd as hda
from holo_diffusion_amd import _lib
from holo_diffusion_amd.generate import chain_groups, generate_samples, parse_cli, shard_indices


def test_chain_groups_split_a_shard_in_order():
    assert chain_groups(range(5), 2) == [[0, 1], [2, 3], [4]]
    assert chain_groups(range(4), 4) == [[0, 1, 2, 3]]
    assert chain_groups(range(3), 8) == [[0, 1, 2]]
    assert chain_groups(range(3), 1) == [[0], [1], [2]]
    assert chain_groups([], 2) == []
    # a rank's round-robin shard keeps its sample ids: rank 1 of 2 over 7 samples
    assert chain_groups(shard_indices(7, 1, 2), 2) == [[1, 3], [5]]
    for bad in (0, -1):
        with pytest.raises(ValueError):
            chain_groups(range(3), bad)


def test_cli_parses_chains_per_gpu():
    assert parse_cli(["exp_dir=/x"])["chains_per_gpu"] == 1
    assert parse_cli(["exp_dir=/x", "chains_per_gpu=4"])["chains_per_gpu"] == 4
    for bad in ("0", "-2", "two", "1.5", "true"):
        with pytest.raises(SystemExit):
            parse_cli(["exp_dir=/x", f"chains_per_gpu={bad}"])


def test_generate_samples_refuses_progressive_with_batched_chains():
    with pytest.raises(ValueError, match="progressive"):
        generate_samples(object(), num_samples=2, chains_per_gpu=2, progressive_sampling_steps_per_render=1)
    with pytest.raises(ValueError, match=">= 1"):
        generate_samples(object(), num_samples=2, chains_per_gpu=0)


def test_row_stream_table():
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=1, device_noise_stream=3)
    assert diff._row_streams(4, torch.device("cpu")) is None  # a plain int: today's kernels
    diff.device_noise_stream = [5, 0, 0xFFFFFFFF]
    t = diff._row_streams(3, torch.device("cpu"))
    assert t.dtype == torch.int32 and t.view(-1).tolist() == [5, 0, -1]  # (uint32 bits)
    assert diff._row_streams(3, torch.device("cpu")) is t  # uploaded once
    with pytest.raises(ValueError, match="3 streams for a batch of 2"):
        diff._row_streams(2, torch.device("cpu"))
    diff.device_noise_stream = [1, 1 << 32]
    with pytest.raises(ValueError, match="2\\^32"):
        diff._row_streams(2, torch.device("cpu"))


def _net(dtype):
    return hda.SimpleUnet3D(image_size=8, in_channels=8, out_channels=8, model_channels=32, channel_mult=(1, 2),
                            attention_resolutions=(2,), compute_dtype=dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f32_bf16x3"])
def test_batch_invariant_is_refused_outside_exact_fp32(dtype):
    net = _net(dtype)
    with pytest.raises(_lib.HoloError, match="exact-fp32"):
        net.set_batch_invariant(True)
    assert not net.batch_invariant
    net.set_batch_invariant(False)  # (turning it off is always allowed)


def test_batch_invariant_flag_defaults_off():
    net = _net("f32")
    assert not net.batch_invariant
    assert net.set_batch_invariant(True) is net and net.batch_invariant  # (no native handle yet: applied at first use)
    net.set_batch_invariant(False)
    assert not net.batch_invariant
