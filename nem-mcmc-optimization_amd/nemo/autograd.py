"""The order score as a differentiable torch function of the mapped weights.

``order_score(engine, pos, w01, cap=0)`` returns ll (B,) for device tensors
``pos`` (B, S) int32 and ``w01`` (B, S, S) float64 and back-propagates
d ll / d w01 (``nemo_score_grad_dev``, csrc/nemo_grad.hip): one enqueue on
torch's current stream over the tensors' own device pointers, with no host
copy and no synchronisation.  The gradient is exactly 0 at every entry that is
not a permissible pair (and ``w01`` is not read there).
"""
from __future__ import annotations

import torch

from .engine import Engine


def _check(name, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"order_score: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"order_score: {name} must be {dtype}, got {t.dtype}")
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError(f"order_score: {name} must be on the engine's device cuda:{device}, got {t.device}")
    if tuple(t.shape) != shape:
        raise ValueError(f"order_score: {name} must be {shape}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"order_score: {name} must be contiguous (strides {t.stride()})")


class _OrderScore(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w01, pos, engine, cap):
        b = pos.shape[0]
        ll = torch.empty(b, dtype=torch.float64, device=w01.device)
        grad = torch.empty_like(w01)
        engine.reserve(b)   # outside the enqueue: grows scratch only when the batch does
        if b:
            with torch.cuda.device(w01.device):
                engine.score_grad_dev(b, pos.data_ptr(), w01.data_ptr(), ll.data_ptr(), grad.data_ptr(), cap=cap,
                                      stream=torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(grad)
        return ll

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad_out[:, None, None] * grad, None, None, None


def order_score(engine: Engine, pos: torch.Tensor, w01: torch.Tensor, cap: int = 0) -> torch.Tensor:
    """ll (B,) of the orders ``pos`` (B, S) int32 at the mapped weights
    ``w01`` (B, S, S) float64, both contiguous on the engine's device;
    differentiable in ``w01``."""
    if pos.dim() != 2:
        raise ValueError(f"order_score: pos must be (B, S), got {tuple(pos.shape)}")
    b = pos.shape[0]
    _check("pos", pos, torch.int32, (b, engine.S), engine.device)
    _check("w01", w01, torch.float64, (b, engine.S, engine.S), engine.device)
    return _OrderScore.apply(w01, pos, engine, int(cap))


__all__ = ["order_score"]
