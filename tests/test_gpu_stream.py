"""The streaming and grouped score kernels against a long-double reference
(GPU): score_kernel<TT, RENORM>, score_group_kernel<TT, CB, GW, RENORM>,
prep_kernel, prep_group_kernel, finalize_kernel and lse_kernel
(csrc/nemo_kernels.hip).

The inputs are tests/stream_models.py's: real-valued tables on each side of
every dispatch threshold (each RENORM of each dtype), one-signed "range"
tables whose deep products leave the fp64 exponent range, S from 2 to kMaxS
with every residue of the unrolled loops as a list length, E from 1 to 65
tiles, every cap class, and weights 0, 1, saturated and an "edge mix" of
{0, 2^-60, 0.5, 1 - 1e-6, 1 - 1e-9, 1 - 2^-53, 1}.  The reference is
fixed_point_models.reference in np.longdouble; no evaluation is skipped or
masked (tests/test_stream_models_cpu.py keeps the reference finite).

Tolerances.  They come from the number formats, not from what the kernels
return.  eps = 2^-53, u = 2^-24, n = the length of a child's parent list (for
cs and the order weights: the longest list of the evaluation), M = max |cell|
of the evaluation.

* fp64 cells and cs: 32 eps max(M, 1) + 4 n eps.  The first term is the few
  roundings a cell takes at its own magnitude (k ln 2 of the renormalised
  exponent, its sum with log(prod), the sum with U, the log-sum-exp's m +
  log(l)) -- the bound test_wide_table_fast_scores_equal_oracle uses.  The
  second: each factor costs the product at most 2 ulp (one FMA, one multiply),
  relative errors of the product and so absolute errors of its log.
* fp64 ll: E times the cs tolerance plus fixed_point_models.noise(cs), the
  left-fold summation bound over the E columns.
* fp64 order weights: ow = exp(cell - cs), so an error d of the exponent is a
  relative error d of ow: the cell tolerance times ow, plus 4 eps.
* fp32 tables, score_kernel: each factor has s, 1 - s (rounded once from
  fp64) and e^T rounded once to fp32, one fmaf and one multiply, 4 u relative
  per factor, and U is rounded once: 4 n u + |U|max u to first order; the
  tolerance is twice that, 8 n u + 2 |U|max u, plus the fp64 term.  (The
  kernel forms the factor in fp64 and rounds it once, which is inside this
  count; the tolerance does not rely on it.)
* fp32 tables, score_group_kernel: its products are fp64, only e^T and U are
  rounded to fp32: n u + |U|max u, doubled, plus the fp64 term.
* lse_kernel: the fp64 cell tolerance with n = rows (one exp and one add per
  row, relative errors of l and so absolute errors of its log).

Every case prints its worst error and tolerance per output (pytest -s):
MEASUREMENTS.md's table of observed errors comes from those lines.

The cross-section.  Every case of stream_models.CASES runs under each of its
caps with a batch of 37 (its evaluations repeated in turn: ntiles * 37 is no
multiple of 8 for odd tile counts), under option xcd_remap 1 and 0, and with
each output combination (ll only; cs; cells only; order weights only; cells
and order weights): one call is compared with the reference, every other call
must return its bits.  Batches of 5 and 1, the reversed batch and
nemo_score_dev on device pointers must return the batch's bits too.  The
group kernel runs the same cases and caps for G = 4, 8 and 16 at batches 1,
G - 1, G, G + 1 and 37."""
import numpy as np
import pytest

import fixed_point_models as fm
import stream_models as sm
from nemo import _lib
from nemo.engine import Engine, _LseEngine

pytestmark = pytest.mark.gpu

GROUPS = (4, 8, 16)


def _engine(c):
    u, t = sm.tables(c.name)
    eng = Engine(u, t, dtype=c.dtype, exact_generic=c.generic)
    eng.set_option("exact", 0)
    if c.e == 1:   # one column: every row is constant, so the table factors; score_path 1 streams it
        assert eng.factored
        eng.set_option("score_path", 1)
    assert (not eng.factored or c.e == 1) and eng.get_option("exact") == 0
    return eng


def _ladder_engine(m):
    if m.nem is not None:
        eng = Engine.from_knockdown(m.nem.observed_knockdown_mat, m.nem.A, m.nem.B)
    else:
        eng = Engine(m.U, m.T)
    eng.set_option("exact", 0)
    eng.set_option("score_path", 1)   # the streaming kernel on a factorable table
    return eng


class Worst:
    """Worst error / tolerance per output of one test, printed and asserted at its end."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, {}, []

    def add(self, what, err, tol, where):
        err, tol = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(err))
        assert not np.isnan(err).any(), (self.tag, what, where)
        k = int(np.argmax(err / tol))
        e, t = float(err.flat[k]), float(tol.flat[k])
        if e / t >= self.rows.get(what, (-1.0,))[0]:
            self.rows[what] = (e / t, e, t, where)
        if e > t:
            self.bad.append((what, where, e, t))

    def done(self):
        for what, (ratio, e, t, where) in sorted(self.rows.items()):
            print(f"STREAM {self.tag} out={what} err={e:.3e} tol={t:.3e} ratio={ratio:.3f} at={where}")
        assert not self.bad, ("(output, where, |got - ref|, tolerance)", self.bad[:8], len(self.bad))


def _check_full(worst, got, r, k, row, perm, cap, dtype, umax, where):
    """One evaluation's ll, cs, cells and order weights (row ``row`` of a full call) against reference k."""
    ld = np.longdouble
    cells, cs, ow = r.cells[k], r.cs[k], r.ow[k]
    e = cs.size
    big = float(np.abs(cells).max())
    lens = np.append(sm.list_lengths(perm, cap), 0)
    trow = np.array([sm.tol_cell(int(n), big, dtype, umax) for n in lens])[:, None]
    tcs = sm.tol_cell(int(r.nmax[k]), big, dtype, umax)
    assert np.isfinite(got["cells"][row]).all() and np.isfinite(got["cs"][row]).all(), where
    worst.add("cells", np.abs(got["cells"][row].astype(ld) - cells), np.broadcast_to(trow, cells.shape), where)
    worst.add("cs", np.abs(got["cs"][row].astype(ld) - cs), tcs, where)
    worst.add("ow", np.abs(got["ow"][row].astype(ld) - ow), tcs * ow.astype(np.float64) + 4.0 * sm.EPS, where)
    worst.add("ll", [abs(float(ld(got["ll"][row]) - cs.sum()))], sm.tol_ll(cs, tcs), where)


def _same(a, b, what):
    for key in ("ll", "cs", "cells", "ow"):
        if a.get(key) is not None and b.get(key) is not None:
            assert np.array_equal(a[key], b[key]), (what, key)


def _rows(d, idx):
    return {k: (None if v is None else v[idx]) for k, v in d.items()}


def _score_dev_full(eng, pos, w, cap):
    """nemo_score_dev on device pointers, every output."""
    import torch
    b, s, e = pos.shape[0], eng.S, eng.E
    eng.reserve(b)
    dpos, dw = torch.from_numpy(pos).cuda(), torch.from_numpy(w).cuda()
    nan = float("nan")
    dll = torch.full((b,), nan, dtype=torch.float64, device="cuda")
    dcs = torch.full((b, e), nan, dtype=torch.float64, device="cuda")
    dcells = torch.full((b, s + 1, e), nan, dtype=torch.float64, device="cuda")
    dow = torch.full((b, s + 1, e), nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().nemo_score_dev(eng.handle, b, dpos.data_ptr(), dw.data_ptr(), int(cap), dll.data_ptr(),
                                         dcs.data_ptr(), dcells.data_ptr(), dow.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return {"ll": dll.cpu().numpy(), "cs": dcs.cpu().numpy(), "cells": dcells.cpu().numpy(), "ow": dow.cpu().numpy()}


def _group_ll(eng, pos, w, cap, group):
    """nemo_score_group_dev: ll of a batch (NaN where the kernel wrote nothing)."""
    import torch
    b = pos.shape[0]
    eng.reserve(b)
    dpos = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    dll = torch.full((b,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.score_dev(b, dpos.data_ptr(), dw.data_ptr(), dll.data_ptr(), cap=cap,
                  stream=torch.cuda.current_stream().cuda_stream, group=group)
    torch.cuda.synchronize()
    return dll.cpu().numpy()


def _stream_case(worst, eng, perms, pos, w01, refs_of, caps, dtype, umax, dev=True):
    n = len(perms)
    idx = sm.tile_batch(n, 37)
    p, w = np.ascontiguousarray(pos[idx]), np.ascontiguousarray(w01[idx])
    for cap in caps:
        r = refs_of(cap)
        eng.set_option("xcd_remap", 1)
        full = eng.score(p, w, cap=cap, want_cs=True, want_cells=True, want_ow=True)
        for k in range(n):
            _check_full(worst, full, r, k, k, perms[k], cap, dtype, umax, f"cap={cap} eval={k}")
        # a repeated evaluation returns its first copy's bits
        _same(_rows(full, np.arange(n, 37)), _rows(full, idx[n:]), ("repeat", cap))
        # every output combination parks the cells on another path: the same bits
        combos = {"ll": {}, "cs": {"want_cs": True}, "cells": {"want_cells": True}, "ow": {"want_ow": True},
                  "cells+ow": {"want_cells": True, "want_ow": True}}
        for remap in (1, 0):
            eng.set_option("xcd_remap", remap)
            for label, kw in combos.items():
                got = eng.score(p, w, cap=cap, **kw)
                got = {"ll": got} if not kw else got
                _same(got, full, (label, cap, remap))
            _same(eng.score(p, w, cap=cap, want_cs=True, want_cells=True, want_ow=True), full, ("full", cap, remap))
        eng.set_option("xcd_remap", 1)
        # batches of 5 and 1, the reversed batch, device pointers
        kw = {"want_cs": True, "want_cells": True, "want_ow": True}
        _same(eng.score(p[:5], w[:5], cap=cap, **kw), _rows(full, slice(0, 5)), ("batch 5", cap))
        for one in (0, n - 1, 36):
            _same(eng.score(p[one:one + 1], w[one:one + 1], cap=cap, **kw), _rows(full, slice(one, one + 1)),
                  ("batch 1", cap, one))
            assert eng.score(p[one:one + 1], w[one:one + 1], cap=cap)[0] == full["ll"][one], ("ll of one", cap, one)
        rev = slice(None, None, -1)
        _same(eng.score(np.ascontiguousarray(p[rev]), np.ascontiguousarray(w[rev]), cap=cap, **kw), _rows(full, rev),
              ("reversed", cap))
        if dev:
            _same(_score_dev_full(eng, p, w, cap), full, ("nemo_score_dev", cap))


@pytest.mark.parametrize("name", sm.case_ids())
def test_score_kernel_against_reference(name):
    c = sm.BY_NAME[name]
    u, _ = sm.tables(name)
    perms, pos, w01 = sm.evals(c.s, c.nevals)
    eng = _engine(c)
    worst = Worst(f"score_kernel<{c.dtype},{c.renorm}> {name}")
    try:
        assert eng.score_kernel(0)[0] == -1 and eng.score_kernel(3, ll_only=False)[0] == -1   # the streaming kernel
        _stream_case(worst, eng, perms, pos, w01, lambda cap: sm.refs(name, cap), c.caps, c.dtype,
                     float(np.abs(u).max()))
    finally:
        eng.close()
    worst.done()


def _group_case(worst, eng, perms, pos, w01, refs_of, caps, dtype, umax, batches=None):
    n = len(perms)
    for cap in caps:
        r = refs_of(cap)
        big = [float(np.abs(r.cells[k]).max()) for k in range(n)]
        tol = [sm.tol_ll(r.cs[k], sm.tol_cell(int(r.nmax[k]), big[k], dtype, umax, group=True)) for k in range(n)]
        want = np.array([float(v) for v in r.cs.sum(axis=1)])
        for g in GROUPS:
            first = {}
            for b in batches or (1, g - 1, g, g + 1, 37):
                # start each batch at another evaluation: every evaluation meets every slot of a group
                idx = (sm.tile_batch(n, b) + b) % n
                ll = _group_ll(eng, pos[idx], w01[idx], cap, g)
                assert np.isfinite(ll).all(), (cap, g, b, ll)
                worst.add(f"ll G={g}", np.abs(ll - want[idx]), np.array(tol)[idx], f"cap={cap} batch={b}")
                # an evaluation's ll does not depend on its batch, its group's other members or its slot
                for k, v in zip(idx, ll):
                    assert first.setdefault(int(k), v) == v, (cap, g, b, int(k))


def _group_cases():
    return [c.name for c in sm.CASES if c.renorm != 2]


@pytest.mark.parametrize("name", _group_cases())
def test_group_kernel_against_reference(name):
    c = sm.BY_NAME[name]
    u, t = sm.tables(name)
    perms, pos, w01 = sm.evals(c.s, c.nevals)
    eng = _engine(c)
    worst = Worst(f"score_group_kernel<{c.dtype},RENORM {sm.group_renorm(c.dtype, c.s, sm.table_absmax(t))}> {name}")
    try:
        _group_case(worst, eng, perms, pos, w01, lambda cap: sm.refs(name, cap), c.caps, c.dtype,
                    float(np.abs(u).max()))
    finally:
        eng.close()
    worst.done()


@pytest.mark.parametrize("name", sm.ladder_ids())
def test_ladder_under_streaming_and_group_kernels(name):
    """fixed_point_models' error-rate ladder and table-built models under score_path 1 and through
    the group entry: the kernel other tests lean on, pinned to the reference at low error rates
    and saturated weights."""
    m = fm.get_model(name)
    perms, pos, w01 = fm.inputs(m.S)
    eng = _ladder_engine(m)
    umax = float(np.abs(m.U).max())
    worst = Worst(f"ladder {name}")
    try:
        assert eng.score_kernel(0)[0] == -1
        _stream_case(worst, eng, perms, pos, w01, lambda cap: sm.ladder_refs(name, cap), (0, 3), "f64", umax, dev=False)
        _group_case(worst, eng, perms, pos, w01, lambda cap: sm.ladder_refs(name, cap), (0, 3), "f64", umax,
                    batches=(len(perms),))
    finally:
        eng.close()
    worst.done()


def test_group_results_do_not_depend_on_the_slot():
    """Rotating or reversing a batch moves every evaluation to another slot of another group
    (other members, another union list): its ll keeps its bits."""
    c = sm.BY_NAME["f64-own-S18-E130-a3"]
    _, pos, w01 = sm.evals(c.s)
    eng = _engine(c)
    try:
        idx = sm.tile_batch(12, 37)
        for cap in (0, 3):
            for g in GROUPS:
                base = _group_ll(eng, pos[idx], w01[idx], cap, g)
                for perm in (np.roll(np.arange(37), 1), np.roll(np.arange(37), g // 2 + 1), np.arange(37)[::-1]):
                    got = _group_ll(eng, pos[idx][perm], w01[idx][perm], cap, g)
                    assert np.array_equal(got, base[perm]), (cap, g)
    finally:
        eng.close()


def test_group_scratch_regrowth_matches_a_fresh_engine():
    """G = 16, then 4, then 8 on one engine with growing batches (each call past the scratch the
    last one left): the results of a fresh engine, bit for bit."""
    c = sm.BY_NAME["f64-own-S18-E130-a3"]
    _, pos, w01 = sm.evals(c.s)
    eng = _engine(c)
    try:
        for g, b in ((16, 5), (4, 12), (8, 37), (16, 130), (4, 64)):
            idx = sm.tile_batch(12, b)
            got = _group_ll(eng, pos[idx], w01[idx], 0, g)
            fresh = _engine(c)
            try:
                assert np.array_equal(got, _group_ll(fresh, pos[idx], w01[idx], 0, g)), (g, b)
            finally:
                fresh.close()
    finally:
        eng.close()


def test_group_entry_arguments():
    c = sm.BY_NAME["f64-own-S18-E130-a3"]
    _, pos, w01 = sm.evals(c.s)
    eng = _engine(c)
    try:
        for g in (0, 2, 3, 5, 32, -4):
            with pytest.raises(_lib.NemoError) as ei:
                _group_ll(eng, pos, w01, 0, g)
            assert ei.value.code == _lib.NEMO_ERR_ARG and "group" in str(ei.value), g
        # group 1 is nemo_score_dev: the host call's bits
        assert np.array_equal(_group_ll(eng, pos, w01, 3, 1), eng.score(pos, w01, cap=3))
    finally:
        eng.close()
    wide = sm.BY_NAME["f64-own-S9-E63-a171-generic"]
    _, pos, w01 = sm.evals(wide.s)
    eng = _engine(wide)
    try:
        for g in GROUPS:
            with pytest.raises(_lib.NemoError) as ei:
                _group_ll(eng, pos, w01, 0, g)
            assert ei.value.code == _lib.NEMO_ERR_ARG and "product range" in str(ei.value), g
    finally:
        eng.close()


# --------------------------------------------------------------------------
# lse_kernel
# --------------------------------------------------------------------------
def _lse_cells(rows, e, seed):
    """Columns spread over +-1500: a base per column, entries near it (the sum counts) or far
    below and above it (the running maximum is rescaled); every third column all but one -inf."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1500.0, 1500.0, e)
    spread = np.where(rng.random((rows, e)) < 0.5, rng.uniform(-3.0, 3.0, (rows, e)), rng.uniform(-1500.0, 1500.0, (rows, e)))
    cells = np.clip(base[None] + spread, -1500.0, 1500.0)
    cells[:, ::4] = np.sort(cells[:, ::4], axis=0)            # ascending: every row is a new maximum
    if rows > 1:
        keep = rng.integers(rows, size=e)
        lone = np.arange(e) % 3 == 1
        mask = lone[None] & (np.arange(rows)[:, None] != keep[None])
        cells[mask] = -np.inf
    return cells


@pytest.mark.parametrize("e", [1, 64, 65, 4100])
@pytest.mark.parametrize("rows", [1, 2, 33, 257])
def test_lse_kernel_against_reference(rows, e):
    ld = np.longdouble
    cells = _lse_cells(rows, e, 100 * rows + e)
    c = cells.astype(ld)
    m = c.max(axis=0)
    cs = m + np.log(np.exp(c - m).sum(axis=0))
    ow = np.exp(c - cs)
    assert np.isfinite(cs).all()
    eng = _LseEngine(e, 0)
    ll, gcs, gow = eng.ll(cells, want=True)
    assert eng.ll(cells) == ll
    big = float(np.abs(cells[np.isfinite(cells)]).max())
    tcs = sm.tol_cell(rows, big)
    worst = Worst(f"lse_kernel rows={rows} E={e}")
    worst.add("cs", np.abs(gcs.astype(ld) - cs), tcs, "")
    worst.add("ow", np.abs(gow.astype(ld) - ow), tcs * ow.astype(np.float64) + 4.0 * sm.EPS, "")
    worst.add("ll", [abs(float(ld(ll) - cs.sum()))], sm.tol_ll(cs, tcs), "")
    if rows > 1:   # a lone finite entry is its column's cs, and its weight 1
        lone = np.arange(e) % 3 == 1
        assert np.array_equal(gcs[lone], cells.max(axis=0)[lone])
        assert np.array_equal(gow[:, lone], (cells[:, lone] == cells.max(axis=0)[lone]).astype(np.float64))
    worst.done()
