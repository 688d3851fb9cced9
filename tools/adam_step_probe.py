"""What the parameter update of a training step costs on the north-star denoiser (64^3 x 32, 165 M parameters), two ways,
alternating in one process on synthetic gradients:

  (a) torch.optim.Adam(foreach=True).step(), then what the next forward_train pays for it: SimpleUnet3D._ensure_handle
      (one holo_unet_set_param per parameter + a host synchronise) and _ensure_dgrad_weights (one holo_unet_set_dgrad_weight
      per convolution weight + a second synchronise)
  (b) HoloAdam.step: the multi-tensor kernel + the stream-ordered re-packs of holo_unet_adam_step
  (c) for the split of (b): the multi-tensor kernel alone, on clones of the same tensors bound as plain tensors

Each repetition is timed with the host clock around work that ends in a device synchronise.  Not a test, not the benchmark.
  python tools/adam_step_probe.py [timed repetitions, default 12]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import holo_diffusion_amd as hda  # noqa: E402
from holo_diffusion_amd.structure import unet_param_shapes  # noqa: E402
from holo_diffusion_amd.weights import synth_state_dict  # noqa: E402

WARMUP = 3
reps = max(10, int(sys.argv[1]) if len(sys.argv) > 1 else 12)
dev = torch.device("cuda", 0)
w = bench.NORTH
net = hda.SimpleUnet3D(image_size=w["resol"], in_channels=32, out_channels=32, model_channels=64, channel_mult=w["channel_mult"],
                       attention_resolutions=w["attention_resolutions"])
net.load_state_dict({"_net." + k: v for k, v in synth_state_dict(unet_param_shapes(64, 32, 32, 64, 2, w["channel_mult"],
                                                                                   w["attention_resolutions"]), 1234).items()})
net.to(dev).requires_grad_(True)
named = dict(net._net.named_parameters())
gen = torch.Generator(device=dev).manual_seed(7)
grads = {k: torch.randn(p.shape, device=dev, generator=gen) * 1e-3 for k, p in named.items()}
for k, p in named.items():
    p.grad = grads[k]
topt = torch.optim.Adam(list(named.values()), lr=4e-5, foreach=True)
hopt = hda.HoloAdam(lr=4e-5).add_unet(net)
plain = {k: p.detach().clone() for k, p in named.items()}
kopt = hda.HoloAdam(lr=4e-5).add_tensors(plain, "unet")
net._ensure_handle(dev)
net._ensure_dgrad_weights(dev)
torch.cuda.synchronize()


def torch_path():
    topt.step()
    net._ensure_handle(dev)
    net._ensure_dgrad_weights(dev)


def native_path():
    hopt.step(grads)


def kernels_only():
    kopt.step(grads)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


ms = {"torch_adam_plus_rebind": [], "holo_adam": [], "holo_adam_kernels_only": []}
for i in range(WARMUP + reps):
    a, b, c = timed(torch_path), timed(native_path), timed(kernels_only)
    if i >= WARMUP:
        ms["torch_adam_plus_rebind"].append(a)
        ms["holo_adam"].append(b)
        ms["holo_adam_kernels_only"].append(c)
out = {"parameters": sum(p.numel() for p in named.values()), "tensors": len(named), "repetitions": reps, "rebinds": net.rebinds}
for k, v in ms.items():
    out[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
print(json.dumps(out))
