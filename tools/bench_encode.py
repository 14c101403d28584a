#!/usr/bin/env python
"""Times mkd_encode (first-stage encoder: image -> scaled latent, posterior sample) for a batch of images."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from makeupdiffuse_amd.engine import MkdEngine, NetConfig, VaeConfig
eng = MkdEngine(NetConfig()); eng.configure_vae_encoder(VaeConfig())
g = torch.Generator(device='cuda'); g.manual_seed(0)
for name, shape in eng.expected_params().items():
    if name.startswith(MkdEngine.VAE_ENCODER_PREFIXES):
        t = torch.randn(shape, generator=g, device='cuda')
        if len(shape) > 1:
            t = t / (t[0].numel() ** 0.5)
        elif 'norm' in name and name.endswith('weight'):
            t = torch.ones(shape, device='cuda')
        eng.load_weight(name, t)
eng.finalize_vae_encoder()
for B, H in ((8, 256), (8, 512), (1, 256)):
    x = torch.rand(B, 3, H, H, device='cuda') * 2 - 1
    noise = torch.randn(B, 4, H // 8, H // 8, device='cuda')
    for _ in range(2): eng.encode(x, noise=noise)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(5): eng.encode(x, noise=noise)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
    print(f'encode B={B} image {H}x{H}: {dt * 1e3:.2f} ms  ({eng.encode_flops() / dt * 1e-12:.0f} TFLOP/s, '
          f'{eng.encode_flops() / 1e12:.2f} TFLOP)', flush=True)
