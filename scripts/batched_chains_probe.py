"""Batched sampling chains at 64^3 x 32 (the north-star net): grid-steps/s of the sampler's perf chain - channels-last UNet
forward + the in-kernel Philox step - at B = 1, 2 and 4 chains per call, with batch-invariant plans (the mode
generate_samples(chains_per_gpu=B) runs in) and with free plans, and the UNet workspace of each.  With
--ops, the per-op table (holo_unet_time_ops) of the invariant and the free plan at the largest B.

    python scripts/batched_chains_probe.py [--batches 1 2 4] [--warmup 5] [--steps 30] [--ops] > out.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd.structure import unet_param_shapes  # noqa: E402
from holo_diffusion_amd.weights import synth_state_dict  # noqa: E402

NORTH = dict(image_size=64, in_channels=32, out_channels=32, model_channels=64, num_res_blocks=2,
             channel_mult=(1, 1, 2, 4, 8), attention_resolutions=(4, 8), num_heads=2)


def make_net(device):
    net = hda.SimpleUnet3D(**NORTH)
    shapes = unet_param_shapes(NORTH["image_size"], NORTH["in_channels"], NORTH["out_channels"], NORTH["model_channels"],
                               NORTH["num_res_blocks"], NORTH["channel_mult"], NORTH["attention_resolutions"])
    net.load_state_dict({"_net." + k: v for k, v in synth_state_dict(shapes, 1234).items()})
    return net.to(device)


def time_chain(net, B, warm, timed, device):
    """Seconds per step of B chains: forward_channels_last + holo_ddpm_step_philox_rows (streams 0..B-1)."""
    diff = hda.ImplicitronGaussianDiffusion(device_noise_seed=7, device_noise_stream=list(range(B)))
    R, C = NORTH["image_size"], NORTH["in_channels"]
    x = torch.randn(B, R, R, R, C, device=device)
    ts = torch.arange(999, 999 - (warm + timed), -1, device=device, dtype=torch.int64)[:, None].repeat(1, B).contiguous()
    with torch.no_grad():
        for k in range(warm + timed):
            if k == warm:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            out = net.forward_channels_last(x, ts[k])
            x, _, _ = diff._step_device_noise(x, ts[k], out, 999 - k, True, want_pred=False, channels_last=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert torch.isfinite(x).all()
    return dt / timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--ops", action="store_true", help="per-op table at the largest batch, invariant and free plans")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batched_chains_probe needs the GPU"
    device = torch.device("cuda", 0)
    net = make_net(device)
    print(f"# {' '.join(sys.argv)}")
    print(f"# north-star net 64^3 x 32, perf chain (channels-last forward + in-kernel Philox step), "
          f"{args.warmup} warm-up + {args.steps} timed steps per row; device {torch.cuda.get_device_name(0)}")
    print(f"{'plans':<10} {'B':>2} {'ms/call':>9} {'grid-steps/s':>13} {'x B=1':>7} {'workspace MiB':>14}")
    base = {}
    for mode in ("invariant", "free"):
        net.set_batch_invariant(mode == "invariant")
        for B in args.batches:
            s = time_chain(net, B, args.warmup, args.steps, device)
            rate = B / s
            base.setdefault(mode, rate if B == 1 else None)
            rel = rate / base[mode] if base.get(mode) else float("nan")
            ws = net.workspace_bytes(B, device) / 2 ** 20
            print(f"{mode:<10} {B:>2} {1e3 * s:>9.3f} {rate:>13.1f} {rel:>7.3f} {ws:>14.1f}")
            sys.stdout.flush()
            torch.cuda.empty_cache()
    if args.ops:
        B = max(args.batches)
        for mode in ("invariant", "free"):
            net.set_batch_invariant(mode == "invariant")
            ops = net.time_ops(B, 5, device)
            print(f"\n# per-op table, B = {B}, {mode} plans (ms per forward, hipEvents; conv rows: kernel, tile depth, split-K)")
            total = 0.0
            for o in ops:
                total += o["ms"]
                extra = f" {o['kernel']} tz{o['tile_depth']} split{o['nsplit']}" if o["op"] == "conv" else ""
                print(f"{o['op']:<12} {o['cin']:>4}->{o['cout']:<4} @{o['out_dim']:>2}^3 {o['ms']:8.4f}{extra}")
            print(f"# total {total:.3f} ms")
    net.set_batch_invariant(False)


if __name__ == "__main__":
    main()
