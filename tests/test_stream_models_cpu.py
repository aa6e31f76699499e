"""The case list of tests/stream_models.py covers what the streaming and
grouped score kernels' launchers decide (CPU only).

The GPU tests (test_gpu_stream.py) run the kernels on that list; this file
keeps the list from thinning out unnoticed: every RENORM is selected for each
dtype on each side of its threshold, every residue of the 8-way and 4-way
unrolled loops appears as a list length, the range tables carry products past
both ends of the fp64 exponent range in a cell that decides its column, and
the reference is finite on every input (so no evaluation is ever skipped or
masked)."""
import numpy as np
import pytest

import fixed_point_models as fm
import stream_models as sm


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_reference_full_agrees_with_the_short_form():
    """``full=True`` and a kept exp(T) return the cells behind the same ll and cs."""
    name = "f64-own-S9-E64-a70"
    u, t = sm.tables(name)
    perms, _, w01 = sm.evals(9)
    for k in (0, 3, 10):
        ll, cs, xmin = fm.reference(u, t, perms[k], w01[k], 3)
        fl, fcs, cells, ow = fm.reference(u, t, perms[k], w01[k], 3, full=True, et=np.exp(t.astype(np.longdouble)))
        assert fl == ll and np.array_equal(fcs.astype(np.float64), cs)
        assert float((cells[:9] - cells[9]).min()) == xmin
        assert np.allclose((ow.sum(axis=0)).astype(np.float64), 1.0, rtol=0, atol=1e-15)


def test_every_renorm_is_selected_on_each_side_of_its_threshold():
    seen = {}
    for c in sm.CASES:
        _, t = sm.tables(c.name)
        amax = sm.table_absmax(t)
        assert amax == (15.0 if c.is_range else c.a) or c.is_range and 14.9 < amax <= 15.0, c.name
        assert c.renorm == sm.renorm(c.dtype, c.s, amax), c.name
        # what the staging accepts: the product range, or a wide fp64 table with exact_generic
        wide = amax > sm.PRODUCT_RANGE[c.dtype]
        assert not wide or (c.generic and c.dtype == "f64" and amax <= sm.WIDE_MAX), c.name
        assert (sm.group_renorm(c.dtype, c.s, amax) is None) == wide
        seen.setdefault((c.dtype, c.renorm), []).append(amax * (c.s - 1))
    assert set(seen) == {("f64", 0), ("f64", 1), ("f64", 2), ("f32", 0), ("f32", 1)}
    # the thresholds' two sides, at the amplitudes the list promises
    assert 560.0 in seen[("f64", 0)] and 640.0 in seen[("f64", 1)]
    assert 76.0 in seen[("f32", 0)] and 95.0 in seen[("f32", 1)]
    by = {(c.dtype, c.s, c.a): c for c in sm.CASES}
    assert by[("f64", 9, 170.0)].renorm == 1 and by[("f64", 9, 171.0)].renorm == 2 and by[("f64", 9, 705.0)].renorm == 2
    assert by[("f32", 18, 20.0)].renorm == 1
    # both kinds, both routes to the streaming kernel (exact_generic is an fp64 option's
    # route: a narrow table through it too), every dtype at kMaxS
    for dtype in ("f64", "f32"):
        for kind in sm.KINDS:
            assert any(c.dtype == dtype and c.kind == kind and c.generic for c in sm.CASES) or dtype == "f32"
            assert any(c.dtype == dtype and c.kind == kind and not c.generic for c in sm.CASES)
        assert any(c.dtype == dtype and c.s == sm.MAX_S for c in sm.CASES)
    assert any(c.generic and c.renorm == 0 for c in sm.CASES)


def test_shapes_cover_the_unrolled_loops_and_the_tiles():
    ss = {c.s for c in sm.CASES}
    assert {2, 18, 64, 65, 130, 256} <= ss
    es = {c.e for c in sm.CASES}
    assert {1, 63, 64, 65, 130, 4100} <= es
    assert any(c.s == 256 and c.e == 70 for c in sm.CASES)
    assert (4100 + sm.TILE - 1) // sm.TILE == 65     # finalize_kernel's strided sum takes a second term
    # S = 18, identity order: list lengths 0..17 -- empty, tails 1..7, exactly 8 and 16, 8 + 1;
    # every residue of the group kernel's 4-way loop with and without a full block before it
    perms, pos, _ = sm.evals(18)
    ident = next(k for k, p in enumerate(perms) if np.array_equal(p, np.arange(18)))
    assert sorted(sm.list_lengths(perms[ident])) == list(range(18))
    for c in sm.CASES:
        if c.s == 18:
            assert {0, 1, 3, 16, 17, 23} == set(c.caps)
    lens = set()
    for c in sm.CASES:
        perms, _, _ = sm.evals(c.s, c.nevals)
        for cap in c.caps:
            for p in perms:
                lens |= set(int(v) for v in sm.list_lengths(p, cap))
    assert {v % 8 for v in lens} == set(range(8)) and {v // 8 for v in lens} >= {0, 1, 2, 7, 31}
    assert {0, 1, 3, 8, 9, 16, 17, 63, 64, 129, 255} <= lens
    # the work count ntiles * 37 is no multiple of 8 for some E (the XCD remap's remainder)
    assert any((((c.e + 63) // 64) * 37) % 8 for c in sm.CASES)
    # the group kernel's dynamic LDS at kMaxS: GW (S - 1) CB doubles, the largest request below 64 KB
    assert 4 * 255 * 8 * 8 == 65280 == 2 * 255 * 16 * 8 and 65280 < 65536


def test_evaluations_hold_every_order_weight_and_edge_value():
    for s, n in ((18, 12), (130, 6), (256, 5)):
        perms, pos, w01 = sm.evals(s, n)
        assert len(perms) == n == pos.shape[0] == w01.shape[0]
        for p, q in zip(perms, pos):
            assert np.array_equal(q[p], np.arange(s))
        ident, rev = np.arange(s), np.arange(s)[::-1]
        assert any(np.array_equal(p, ident) for p in perms) and any(np.array_equal(p, rev) for p in perms)
        assert any(not np.array_equal(p, ident) and not np.array_equal(p, rev) for p in perms)
        assert any((w == 1.0).all() for w in w01)
        edge = [w for w in w01 if np.isin(w, sm.EDGE_WEIGHTS).all() and not np.isin(w, (0.0, 1.0)).all()]
        assert len(edge) == 3
        assert all(set(np.unique(w)) == set(sm.EDGE_WEIGHTS) for w in edge)
    perms, _, w01 = sm.evals(18)
    assert any((w == 0.0).all() for w in w01)
    # a group of four holds the identity and its reverse: disjoint parent sets, a union list of
    # all S - 1 parents in which each member's missing half is the padding weight 0
    assert np.array_equal(perms[2], np.arange(18)) and np.array_equal(perms[3], np.arange(18)[::-1])


@pytest.mark.parametrize("kind", sm.KINDS)
def test_range_tables_reach_past_both_ends_of_the_exponent_range(kind):
    name = f"f64-{kind}-S64-E130-range"
    c = sm.BY_NAME[name]
    u, t = sm.tables(name)
    assert np.all(t[:, :, sm.RANGE_POS] >= 10.0) and np.all(t[:, :, sm.RANGE_POS] <= 15.0)
    assert np.all(t[:, :, sm.RANGE_NEG] <= -10.0) and np.all(t[:, :, sm.RANGE_NEG] >= -15.0)
    assert np.abs(t).max() <= 15.0
    perms, _, w01 = sm.evals(64)
    k = 2
    assert np.array_equal(perms[k], np.arange(64)) and (w01[k] == 1.0).all()
    r = sm.refs(name, 0)
    deep = 63    # the identity order's last child: 63 parents
    logprod = (r.cells[k][deep] - u[deep].astype(np.longdouble)).astype(np.float64)
    assert (logprod > 710.0).any() and (logprod[sm.RANGE_POS] > 710.0).all()
    gap = (r.cells[k].max(axis=0) - r.cells[k][deep]).astype(np.float64)
    decisive = (logprod < -745.0) & (gap <= 30.0)
    assert decisive.any() and decisive[sm.RANGE_NEG].all()
    # ... and in some column that cell is the maximum itself: dropping it moves ll
    assert (gap[sm.RANGE_NEG] == 0.0).any()
    assert c.renorm == 1 and sm.group_renorm("f64", 64, 15.0) == 1


@pytest.mark.parametrize("name", sm.case_ids())
def test_reference_is_finite_on_every_input(name):
    c = sm.BY_NAME[name]
    for cap in c.caps:
        r = sm.refs(name, cap)
        assert r.ll.shape == (c.nevals,)
        assert np.isfinite(r.ll).all() and np.isfinite(r.cs).all() and np.isfinite(r.cells).all()
        assert np.isfinite(r.ow).all() and (r.ow >= 0).all() and (r.ow <= 1).all()
        # float64 holds them too: what the kernels' outputs are compared with
        assert np.isfinite(r.cells.astype(np.float64)).all() and np.isfinite(r.cs.astype(np.float64)).all()


def test_ladder_list():
    ids = sm.ladder_ids()
    assert len(ids) == 2 * len(fm.LADDER) + len(fm.TABLES)
    cs = {fm.predict(fm.get_model(n).U, fm.get_model(n).T).c for n in ids if n.startswith("nem")}
    assert cs == {-1, 1, 2, 3, 4, 5, 6, 7}
    for n in ids[:2] + ids[-2:]:
        r = sm.ladder_refs(n, 0)
        assert np.isfinite(r.cells).all() and np.isfinite(r.cs).all()
