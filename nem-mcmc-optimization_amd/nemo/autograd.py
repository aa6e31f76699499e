"""The order score as a differentiable torch function of the mapped weights.

``order_score(engine, pos, w01, cap=0)`` returns ll (B,) for device tensors
``pos`` (B, S) int32 and ``w01`` (B, S, S) float64 and back-propagates
d ll / d w01 (``nemo_score_grad_dev``, csrc/nemo_grad.hip): one enqueue on
torch's current stream over the tensors' own device pointers, with no host
copy and no synchronisation.  The gradient is exactly 0 at every entry that is
not a permissible pair (and ``w01`` is not read there).

``order_score_rates(engine, pos, w01, A, B, cap=0)`` is the same score at
per-gene error rates ``A``, ``B`` (B, S) float64 -- A_k = log(alpha_k / (1 -
beta_k)), B_k = log(beta_k / (1 - alpha_k)) -- on an engine staged from a
knockdown matrix, differentiable in ``w01``, ``A`` and ``B``
(``nemo_score_rates_dev``): again one enqueue, no host copy, no synchronisation.
"""
from __future__ import annotations

import torch

from .engine import Engine


def _check(name, t, dtype, shape, device, fn="order_score"):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{fn}: {name} must be {dtype}, got {t.dtype}")
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError(f"{fn}: {name} must be on the engine's device cuda:{device}, got {t.device}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{fn}: {name} must be {shape}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be contiguous (strides {t.stride()})")


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


class _OrderScoreRates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w01, A, B, pos, engine, cap):
        b = pos.shape[0]
        ll = torch.empty(b, dtype=torch.float64, device=w01.device)
        grad = torch.empty_like(w01)
        rates = torch.stack((A, B), dim=1)   # (B, 2, S): the A row, then the B row
        drates = torch.empty_like(rates)
        engine.reserve(b)
        if b:
            with torch.cuda.device(w01.device):
                engine.score_rates_dev(b, pos.data_ptr(), w01.data_ptr(), rates.data_ptr(), ll.data_ptr(),
                                       drates.data_ptr(), grad.data_ptr(), cap=cap,
                                       stream=torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(grad, drates)
        return ll

    @staticmethod
    def backward(ctx, grad_out):
        grad, drates = ctx.saved_tensors
        go = grad_out[:, None]
        return go[:, :, None] * grad, go * drates[:, 0], go * drates[:, 1], None, None, None


def order_score_rates(engine: Engine, pos: torch.Tensor, w01: torch.Tensor, A: torch.Tensor, B: torch.Tensor,
                      cap: int = 0) -> torch.Tensor:
    """ll (B,) of the orders ``pos`` (B, S) int32 at the mapped weights ``w01``
    (B, S, S) and the per-gene rates ``A``, ``B`` (B, S), all float64 and
    contiguous on the engine's device (broadcast a scalar with
    ``expand().contiguous()``); differentiable in ``w01``, ``A`` and ``B``.
    The rates are not validated here: non-finite rates give non-finite
    outputs."""
    fn = "order_score_rates"
    if pos.dim() != 2:
        raise ValueError(f"{fn}: pos must be (B, S), got {tuple(pos.shape)}")
    b = pos.shape[0]
    _check("pos", pos, torch.int32, (b, engine.S), engine.device, fn)
    _check("w01", w01, torch.float64, (b, engine.S, engine.S), engine.device, fn)
    _check("A", A, torch.float64, (b, engine.S), engine.device, fn)
    _check("B", B, torch.float64, (b, engine.S), engine.device, fn)
    return _OrderScoreRates.apply(w01, A, B, pos, engine, int(cap))


__all__ = ["order_score", "order_score_rates"]
