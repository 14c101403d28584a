"""Helpers for the -m gpu parity tests: call libmkd through its C ABI with torch-owned device memory."""
import ctypes as C

import torch

from makeupdiffuse_amd import lib as mlib

DEV = 'cuda:0'


def L():
    return mlib.load()


def P(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def bf(t):
    return t.to(DEV).to(torch.bfloat16).contiguous()


def rel_l2(a, b):
    a = a.float().cpu(); b = b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def assert_close_bf16(out, ref, rel=4e-3, what=''):
    """SURVEY.md §8c per-kernel tolerance: rel-L2 <= 4e-3, max-abs <= 2^-6 * |ref|_inf (bf16 in, fp32 acc)."""
    out = out.float().cpu(); ref = ref.float().cpu()
    assert torch.isfinite(out).all(), f'{what}: non-finite output'
    r = rel_l2(out, ref)
    mx = (out - ref).abs().max().item()
    lim = ref.abs().max().item() * 2 ** -6
    assert r <= rel, f'{what}: rel-L2 {r:.3e} > {rel:.1e}'
    assert mx <= lim, f'{what}: max-abs {mx:.3e} > {lim:.3e}'


def dot_bound(n, abs_sum):
    """A-priori bound on an fp32 dot product of n terms (any summation order, FMA or not): |err| <= (n + 16) 2^-24 sum |a_i b_i|
    per element; abs_sum is that sum (a tensor, float64).  The 16 covers a bias, a scale and the rounding of the inputs' products;
    a missed tap, lane or channel is off by a term of the sum itself, orders of magnitude more."""
    return (n + 16) * 2.0 ** -24 * abs_sum.double()


def assert_within(out, ref, bound, what=''):
    """Per element |out - ref| <= bound (tensors of one shape, compared in float64); reports the worst ratio."""
    out = out.double().cpu(); ref = ref.double().cpu(); bound = bound.double().cpu()
    assert torch.isfinite(out).all(), f'{what}: non-finite output'
    ratio = ((out - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f'[bound] {what}: worst |err| / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{what}: |err| is {ratio:.2f} x its bound at the worst element'


def sync():
    torch.cuda.synchronize()
