"""The error rates as parameters of the model.

The reference fixes alpha (false positive) and beta (false negative) when a
NEM is built; the closing comment of its nem.py ("shared probability between
clusters for the error rates, use that as a latent variable") names what it
never built.  The engine scores a batch of evaluations, each at its own
per-gene rates, with the derivatives in them (``Engine.score_rates``,
``nemo.autograd.order_score_rates``); this module holds what turns that into a
fit:

* ``log_ratios(alpha, beta)``: A = log(alpha / (1 - beta)), B = log(beta /
  (1 - alpha)), the form the engine takes (nem.py:17-18);
* ``absolute_ll(ll, D, alpha, beta)``: the order score ll is a ratio against
  a baseline -- every effect attached to nothing and every observation a
  "correct" one -- that itself depends on the rates, so across rates one
  compares L = ll + sum_k [ n_k log(1 - beta_k) + (E - n_k) log(1 - alpha_k) ],
  n_k = sum_e D[k][e] (up to the constant -E log(S + 1) of the uniform prior
  over attachments, with which L is the log of the mixture likelihood);
* ``fit_error_rates``: L-BFGS on -L over the rates, and optionally the
  weights, of a fixed order.
"""
from __future__ import annotations

import numpy as np


def _is_torch(*xs):
    try:
        import torch
    except ImportError:   # numpy callers need no torch
        return False
    return any(isinstance(x, torch.Tensor) for x in xs)


def log_ratios(alpha, beta):
    """(A, B) = (log(alpha / (1 - beta)), log(beta / (1 - alpha))), in numpy or in torch."""
    if _is_torch(alpha, beta):
        import torch
        return torch.log(alpha / (1.0 - beta)), torch.log(beta / (1.0 - alpha))
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    return np.log(alpha / (1.0 - beta)), np.log(beta / (1.0 - alpha))


def absolute_ll(ll, D, alpha, beta):
    """L = ll + sum_k [ n_k log(1 - beta_k) + (E - n_k) log(1 - alpha_k) ] for
    the knockdown matrix D (S, E) and rates that are scalars or (S,) -- or
    (..., S) against ll (...,).  numpy in, numpy out; when ll or a rate is a
    torch tensor the result is one (differentiable in all three)."""
    d = np.asarray(D)
    e = d.shape[1]
    n = d.sum(axis=1).astype(np.float64)
    if _is_torch(ll, alpha, beta):
        import torch
        ref = next(x for x in (ll, alpha, beta) if isinstance(x, torch.Tensor))
        nt = torch.as_tensor(n, dtype=torch.float64, device=ref.device)
        al = torch.as_tensor(alpha, dtype=torch.float64, device=ref.device)
        be = torch.as_tensor(beta, dtype=torch.float64, device=ref.device)
        base = nt * torch.log1p(-be) + (e - nt) * torch.log1p(-al)
        return ll + base.sum(dim=-1)
    al, be = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    base = n * np.log1p(-be) + (e - n) * np.log1p(-al)
    return ll + base.sum(axis=-1)


def fit_error_rates(D, order, weights=None, errors0=(0.2, 0.2), per_gene=False, fit_weights=False,
                    bounds=(1e-12, 0.5), max_iter=50, rel_diff=1e-8, device=0):
    """Maximise L (``absolute_ll``) over the error rates of a fixed order on the GPU.

    ``D`` (S, E) 0/1, S <= 64; ``order``: the S-genes first to last; ``weights``
    (S, S) mapped weights, [i][j] that of parent j of child i (default 0.5),
    read at the permissible pairs alone.  Each rate is lo + (hi - lo)
    sigmoid(u) within ``bounds``, started from ``errors0``; ``per_gene`` gives
    every S-gene its own pair.  ``fit_weights`` adds the logits of the
    permissible pairs, started from ``weights``.  ``torch.optim.LBFGS`` with a
    strong-Wolfe line search runs on -L through ``order_score_rates``, with
    ``JointMethod``'s bookkeeping: every closure's L is listed and the best
    one kept.

    -> (alpha, beta, weights, L, L_list): the rates as floats, or (S,) arrays
    with ``per_gene``; the (S, S) weights of the best evaluation.

    What a fit can and cannot tell (a CPU experiment on synthetic 16 x 130
    data, fp64 numpy): with the generating graph's order and closure as fixed
    weights, scalar rates started from (0.2, 0.2) reach an L above that of the
    generating rates in about ten iterations, near them.  With a wrong order
    and arbitrary fixed weights the fit runs to beta = 0.5 ("nothing is
    observable"): the best explanation of data the graph does not explain.
    With ``per_gene=True`` it overfits, driving rates to the bounds.  Neither
    is an error of the routine."""
    import torch

    from .autograd import order_score_rates
    from .engine import Engine
    d = np.ascontiguousarray(np.asarray(D), dtype=np.uint8)
    s = d.shape[0]
    order = np.asarray(order, dtype=np.int64)
    if sorted(order.tolist()) != list(range(s)):
        raise ValueError(f"order must be a permutation of 0..{s - 1}")
    lo, hi = float(bounds[0]), float(bounds[1])
    if not 0.0 < lo < hi < 1.0:
        raise ValueError(f"bounds {bounds} must satisfy 0 < lo < hi < 1")
    a0, b0 = (float(v) for v in errors0)
    if not (lo <= a0 <= hi and lo <= b0 <= hi):
        raise ValueError(f"errors0 {errors0} outside the bounds {bounds}")
    pos_h = np.empty(s, dtype=np.int32)
    pos_h[order] = np.arange(s)
    mask_h = pos_h[:, None] > pos_h[None, :]
    w_h = np.full((s, s), 0.5) if weights is None else np.asarray(weights, dtype=np.float64)
    if w_h.shape != (s, s):
        raise ValueError(f"weights must be ({s}, {s}), got {w_h.shape}")
    w_h = np.where(mask_h, w_h, 0.0)

    eng = Engine.from_knockdown(d, *log_ratios(a0, b0), device=device)
    try:
        dev = torch.device("cuda", device)
        pos = torch.from_numpy(pos_h[None]).to(dev)
        mask = torch.from_numpy(mask_h[None]).to(dev)
        w_fix = torch.from_numpy(w_h[None]).to(dev)
        shape = (s,) if per_gene else ()

        def logit(r):
            t = min(max((r - lo) / (hi - lo), 1e-12), 1.0 - 1e-12)
            return float(np.log(t / (1.0 - t)))

        ua = torch.full(shape, logit(a0), dtype=torch.float64, device=dev, requires_grad=True)
        ub = torch.full(shape, logit(b0), dtype=torch.float64, device=dev, requires_grad=True)
        params = [ua, ub]
        x = None
        if fit_weights:
            wc = np.clip(w_h, 1e-12, 1.0 - 1e-12)
            x = torch.from_numpy(np.where(mask_h, np.log(wc / (1.0 - wc)), 0.0)[None]).to(dev).requires_grad_(True)
            params.append(x)
        opt = torch.optim.LBFGS(params, max_iter=int(max_iter), tolerance_change=float(rel_diff),
                                line_search_fn="strong_wolfe")
        l_list, best = [], {"L": -float("inf")}

        def closure():
            opt.zero_grad()
            alpha = lo + (hi - lo) * torch.sigmoid(ua)
            beta = lo + (hi - lo) * torch.sigmoid(ub)
            a, b = log_ratios(alpha, beta)
            w = w_fix if x is None else torch.where(mask, torch.sigmoid(x), torch.zeros_like(x))
            ll = order_score_rates(eng, pos, w, a.expand(1, s).contiguous(), b.expand(1, s).contiguous())[0]
            big_l = absolute_ll(ll, d, alpha, beta)
            (-big_l).backward()
            v = float(big_l.detach())
            l_list.append(v)
            if v > best["L"]:
                best.update(L=v, alpha=alpha.detach().cpu().numpy(), beta=beta.detach().cpu().numpy(),
                            w=w.detach()[0].cpu().numpy())
            return -big_l

        opt.step(closure)
    finally:
        eng.close()
    if "w" not in best:
        raise FloatingPointError("fit_error_rates: no evaluation gave a finite L")
    al, be = best["alpha"], best["beta"]
    if not per_gene:
        al, be = float(al), float(be)
    return al, be, best["w"], best["L"], l_list


__all__ = ["absolute_ll", "fit_error_rates", "log_ratios"]
