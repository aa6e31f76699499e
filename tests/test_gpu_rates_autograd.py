"""nemo.autograd.order_score_rates (a torch.autograd.Function over
nemo_score_rates_dev) and nemo.rates.fit_error_rates (GPU)."""
import numpy as np
import pytest

import rates_ref as rr
from nemo.engine import Engine

pytestmark = pytest.mark.gpu


def _setup():
    """(engine, D, perms, pos (3, S), w01 in (0.05, 0.95), A, B (3, S)) of an S = 5, E = 17 model."""
    s, e = 5, 17
    d = rr.small_d(s, e)
    eng = Engine.from_knockdown(d, -1.0, -2.0)
    rng = np.random.default_rng(23)
    perms = [rng.permutation(s) for _ in range(3)]
    pos = np.empty((3, s), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(s)
    al, be = rng.uniform(0.02, 0.4, (3, s)), rng.uniform(0.02, 0.4, (3, s))
    a, b = rr.log_ratios(al, be)
    return eng, d, perms, pos, rng.uniform(0.05, 0.95, (3, s, s)), np.ascontiguousarray(a), np.ascontiguousarray(b)


def test_gradcheck():
    import torch

    from nemo.autograd import order_score_rates
    eng, _, _, pos, w01, a, b = _setup()
    try:
        dpos = torch.from_numpy(pos).cuda()
        w = torch.from_numpy(w01).cuda().requires_grad_(True)
        ta = torch.from_numpy(a).cuda().requires_grad_(True)
        tb = torch.from_numpy(b).cuda().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x, y, z: order_score_rates(eng, dpos, x, y, z), (w, ta, tb))
        assert torch.autograd.gradcheck(lambda x, y, z: order_score_rates(eng, dpos, x, y, z, 2), (w, ta, tb))
    finally:
        eng.close()


def test_per_evaluation_scaling_and_the_host_entry_bits():
    import torch

    from nemo.autograd import order_score_rates
    eng, d, perms, pos, w01, a, b = _setup()
    try:
        dpos = torch.from_numpy(pos).cuda()
        w = torch.from_numpy(w01).cuda().requires_grad_(True)
        ta = torch.from_numpy(a).cuda().requires_grad_(True)
        tb = torch.from_numpy(b).cuda().requires_grad_(True)
        ll = order_score_rates(eng, dpos, w, ta, tb)
        scale = np.array([1.0, -2.5, 0.125])
        (ll * torch.from_numpy(scale).cuda()).sum().backward()
        ll_h, da_h, db_h, g_h = eng.score_rates(pos, w01, a, b)
        assert np.array_equal(ll.detach().cpu().numpy(), ll_h)
        # a power of two or one product per entry: the scaling is exact or one rounding
        for got, want in ((w.grad, scale[:, None, None] * g_h), (ta.grad, scale[:, None] * da_h),
                          (tb.grad, scale[:, None] * db_h)):
            assert np.array_equal(got.cpu().numpy(), want)
        for k in range(3):
            ref = rr.rates_reference(d, a[k], b[k], perms[k], w01[k])
            assert (np.abs(da_h[k].astype(np.longdouble) - ref.da).astype(np.float64) <= ref.tol_a).all()
            assert (np.abs(db_h[k].astype(np.longdouble) - ref.db).astype(np.float64) <= ref.tol_b).all()
    finally:
        eng.close()


def test_wrong_dtype_device_shape_or_stride_raises():
    import torch

    from nemo.autograd import order_score_rates
    eng, _, _, pos, w01, a, b = _setup()
    try:
        dpos, w = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda()
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        with pytest.raises(TypeError, match="float64"):
            order_score_rates(eng, dpos, w.float(), ta, tb)
        with pytest.raises(TypeError, match="float64"):
            order_score_rates(eng, dpos, w, ta.float(), tb)
        with pytest.raises(TypeError, match="int32"):
            order_score_rates(eng, dpos.long(), w, ta, tb)
        with pytest.raises(TypeError, match="Tensor"):
            order_score_rates(eng, dpos, w, a, tb)
        with pytest.raises(ValueError, match="device"):
            order_score_rates(eng, dpos, w, ta, tb.cpu())
        with pytest.raises(ValueError, match="device"):
            order_score_rates(eng, dpos.cpu(), w, ta, tb)
        with pytest.raises(ValueError, match="contiguous"):
            order_score_rates(eng, dpos, w.transpose(1, 2), ta, tb)
        with pytest.raises(ValueError, match="contiguous"):
            order_score_rates(eng, dpos, w, ta[0].expand(3, 5), tb)
        with pytest.raises(ValueError, match="must be"):
            order_score_rates(eng, dpos, w, ta[0], tb)
        with pytest.raises(ValueError, match="must be"):
            order_score_rates(eng, dpos, w[:2], ta, tb)
    finally:
        eng.close()


def test_fit_error_rates_against_the_cpu_fit():
    """Scalar rates of the generating graph's order and closure, from (0.2, 0.2): the GPU fit's L is no
    worse than the start, than the generating rates, and than scipy's fit of the fp64 restatement less
    100 rel_diff |L| (two optimisers with different stopping rules at rel_diff = 1e-8).  The recovered
    rates are a statistical matter and not asserted."""
    from nemo.rates import fit_error_rates
    d, order, w = rr.fit_case()
    l_cpu, al_cpu, be_cpu, _, l_start, l_truth = rr.cpu_fit()
    al, be, w_out, l_fit, l_list = fit_error_rates(d, order, weights=w, errors0=rr.FIT_START, rel_diff=rr.REL_DIFF)
    print(f"RATES fit: L_start {l_list[0]:.4f} (cpu {l_start:.4f}) L_truth {l_truth:.4f} L_fit {l_fit:.6f} "
          f"(cpu {l_cpu:.6f}, gap {l_fit - l_cpu:.3e}) alpha {al:.4f} beta {be:.4f} (cpu {al_cpu:.4f} {be_cpu:.4f}) "
          f"in {len(l_list)} evaluations")
    assert isinstance(al, float) and isinstance(be, float)
    assert l_fit == max(l_list) and len(l_list) > 1
    assert abs(l_list[0] - l_start) <= 1e-9 * abs(l_start)
    assert l_fit >= l_list[0]
    assert l_fit >= l_truth
    assert l_fit >= l_cpu - 100.0 * rr.REL_DIFF * abs(l_cpu)
    mask = w_out != 0.0
    assert np.array_equal(w_out[mask], w[mask]) and w_out.shape == w.shape


def test_fit_per_gene_and_with_weights_runs_and_improves():
    from nemo.rates import fit_error_rates
    d, order, w = rr.fit_case()
    al, be, w_out, l_fit, l_list = fit_error_rates(d, order, weights=np.clip(w, 0.1, 0.9), per_gene=True,
                                                   fit_weights=True, max_iter=15)
    assert al.shape == (16,) and be.shape == (16,) and w_out.shape == (16, 16)
    assert l_fit == max(l_list) >= l_list[0] and np.isfinite(l_list).all()
    pos = np.empty(16, dtype=np.int64)
    pos[order] = np.arange(16)
    assert (w_out[pos[:, None] <= pos[None, :]] == 0.0).all()
