"""nemo.autograd.order_score (a torch.autograd.Function over
nemo_score_grad_dev) and nemo.methods.JointMethod (GPU)."""
import numpy as np
import pytest

import fixed_point_models as fm
import score_grad_ref as gr
import stream_models as sm
from nemo.engine import Engine
from nemo.methods import JointMethod

pytestmark = pytest.mark.gpu


def _setup(kind):
    """(engine, pos (3, S) int32, w01 (3, S, S) in (0.05, 0.95)) of a small factored / generic model."""
    if kind == "factored":
        m = gr.get_model("small-S4-E20")
        u, t = m.U, m.T
    else:
        rng = np.random.default_rng(3)
        t, u = rng.uniform(-2.0, 2.0, (5, 5, 33)), rng.uniform(-2.0, 2.0, (6, 33))
    s = t.shape[0]
    eng = Engine(u, t)
    assert eng.factored == (kind == "factored")
    rng = np.random.default_rng(17)
    perms = [rng.permutation(s) for _ in range(3)]
    pos = np.empty((3, s), dtype=np.int32)
    for k, p in enumerate(perms):
        pos[k, p] = np.arange(s)
    return eng, u, t, perms, pos, rng.uniform(0.05, 0.95, (3, s, s))


@pytest.mark.parametrize("kind", ["factored", "generic"])
def test_gradcheck(kind):
    import torch

    from nemo.autograd import order_score
    eng, _, _, _, pos, w01 = _setup(kind)
    try:
        dpos = torch.from_numpy(pos).cuda()
        w = torch.from_numpy(w01).cuda().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: order_score(eng, dpos, x), (w,))
        assert torch.autograd.gradcheck(lambda x: order_score(eng, dpos, x, 2), (w,))
    finally:
        eng.close()


def test_chain_rule_through_sigmoid_and_per_evaluation_scaling():
    import torch

    from nemo.autograd import order_score
    eng, u, t, perms, pos, w01 = _setup("factored")
    try:
        dpos = torch.from_numpy(pos).cuda()
        x = torch.from_numpy(np.log(w01 / (1.0 - w01))).cuda().requires_grad_(True)
        sig = torch.sigmoid(x)
        ll = order_score(eng, dpos, sig)
        scale = torch.tensor([1.0, -2.5, 0.125], dtype=torch.float64, device="cuda")
        (ll * scale).sum().backward()
        s01 = sig.detach().cpu().numpy()
        ll_h, g_h = eng.score_grad(pos, s01)
        assert np.array_equal(ll.detach().cpu().numpy(), ll_h)
        want = scale.cpu().numpy()[:, None, None] * g_h * (s01 * (1.0 - s01))
        got = x.grad.cpu().numpy()
        for k in range(3):
            ref = gr.grad_reference(u, t, perms[k], s01[k])
            tol = abs(float(scale[k])) * ref.tol * 0.25 + 1e-300   # sigma' <= 1/4; the kernel's bits carry no error
            assert (np.abs(got[k] - want[k]) <= tol).all(), k
            ok = gr.permissible(perms[k])
            assert (got[k][~ok] == 0.0).all()
            # and the engine's gradient itself is the reference's
            assert (np.abs(g_h[k].astype(np.longdouble) - ref.g).astype(np.float64) <= ref.tol).all(), k
    finally:
        eng.close()


def test_wrong_dtype_device_or_stride_raises():
    import torch

    from nemo.autograd import order_score
    eng, _, _, _, pos, w01 = _setup("factored")
    try:
        dpos, w = torch.from_numpy(pos).cuda(), torch.from_numpy(w01).cuda()
        with pytest.raises(TypeError, match="float64"):
            order_score(eng, dpos, w.float())
        with pytest.raises(TypeError, match="int32"):
            order_score(eng, dpos.long(), w)
        with pytest.raises(ValueError, match="device"):
            order_score(eng, dpos, w.cpu())
        with pytest.raises(ValueError, match="device"):
            order_score(eng, dpos.cpu(), w)
        with pytest.raises(ValueError, match="contiguous"):
            order_score(eng, dpos, w.transpose(1, 2))
        with pytest.raises(ValueError, match="contiguous"):
            order_score(eng, torch.from_numpy(np.tile(pos, (1, 2))).cuda()[:, ::2], w)
        with pytest.raises(ValueError, match="must be"):
            order_score(eng, dpos, w[:2])
    finally:
        eng.close()


def test_joint_method_on_net2(net2):
    m, _ = net2
    order = np.random.default_rng(0).permutation(m.num_s)
    tables = m.get_score_tables(m.observed_knockdown_mat)
    jm = JointMethod(order, m.num_s, m.num_e, m.U, tables)
    dag, real_ll = jm.optimize(max_iter=30)
    assert len(jm.ll_list) > 1 and jm.best_ll == max(jm.ll_list)
    assert jm.best_ll > jm.ll_list[0]
    # best_ll is the order score of the kept weights
    eng = jm.engine
    pos = jm._pos[None, :]
    perm = np.asarray(order)
    full = fm.reference(m.U, np.asarray(tables, dtype=np.float64), perm, jm.best_weights, full=True)
    tol = sm.tol_ll(full[1], sm.tol_cell(m.num_s - 1, float(np.abs(full[2]).max())))
    assert abs(jm.best_ll - float(eng.score(pos, jm.best_weights[None])[0])) <= tol
    assert abs(jm.best_ll - full[0]) <= tol
    # the return: Method.optimize's shapes and types, and the rounded weights' own score
    assert isinstance(real_ll, float) and dag.shape == (m.num_s, m.num_s) and dag.dtype == (1 * (np.zeros(1) > 0.5)).dtype
    assert set(np.unique(dag)) <= {0, 1}
    assert real_ll == float(eng.score(pos, dag.T.astype(np.float64)[None])[0])
    assert (dag.T[jm.mask == 0] == 0).all()
