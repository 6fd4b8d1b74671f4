"""Helpers shared by tests/test_gpu_distq_edges.py and tests/test_gpu_rainbow_edges.py."""
import torch

SENTINEL = 7.0          # grad_out is pre-filled: a column the engine must zero cannot pass by luck


def dev_obs(obs):
    """uint8 NCHW host observations -> the engines' NHWC device tensor."""
    return torch.as_tensor(obs).permute(0, 2, 3, 1).contiguous().cuda()


def within(got, ref, bar, what):
    """Every element of `got` within `bar` of the float64 `ref` (prints the largest |got - ref| / bar first)."""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    assert torch.isfinite(got).all(), what
    ratio = (got - ref).abs() / bar.clamp_min(1e-300)
    bad = (got - ref).abs() > bar
    print(f"    {what}: largest |got - ref64| / bar = {float(torch.where(bar > 0, ratio, torch.zeros_like(ratio)).max()):.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), float(((got - ref).abs() - bar).max()))
