"""The case list of tests/ancestor_inputs.py covers what the device inverse
(ancestor_kernel) decides by S and by value (CPU only).

The GPU tests (test_gpu_ancestor.py) run the kernel on that list; this file
keeps the list from thinning out unnoticed.  Every chain is classified with
the host's own calls (test_gpu_ancestor._host: scipy's expit and inv): (a) inv
raises LinAlgError, (b) the inverse is finite, (c) it is non-finite and nothing
is raised.  Ties and swaps are counted with a plain numpy partial-pivot LU
(ancestor_inputs.lu_stats), which is exact on the ``sat`` family's entries
(0, -1/2, -1 and 1 under a permutation: every quotient and product is a dyadic
fraction of a few bits)."""
import functools

import numpy as np

import ancestor_inputs as ai
from test_gpu_ancestor import _host


@functools.lru_cache(maxsize=None)
def _survey():
    """Per (S, cap): [(family, index, class, W~, ancestor_x)]."""
    out = {}
    for s in ai.SIZES:
        for cap in ai.all_caps(s):
            labels = ai.batch(s, cap)[2]
            out[(s, cap)] = [(f, k) + c for (f, k), c in zip(labels, ai.classified(_host, s, cap))]
    return out


def _w01(s, cap, idx):
    """W~ of a chain whatever its class (a class-(a) chain has none from _host)."""
    from scipy.special import expit
    pos, w, _ = ai.batch(s, cap)
    m = ai.mask(pos[idx:idx + 1], cap)[0]
    sig = w[idx].copy()
    sig[m] = expit(sig[m])
    return sig


def test_every_size_has_finite_chains_in_every_family():
    sv = _survey()
    for s in ai.SIZES:
        for fam in ai.FAMILIES:
            if fam == "sat_stale":
                continue
            n = sum(f == fam and c == "b" for cap in ai.all_caps(s) for f, _, c, _, _ in sv[(s, cap)])
            assert n >= 1, (s, fam)
    counts = {}
    for rows in sv.values():
        for f, _, c, _, _ in rows:
            counts[(f, c)] = counts.get((f, c), 0) + 1
    print("chains per (family, class):", sorted(counts.items()))
    for fam in ("sat", "few", "edge"):
        assert counts.get((fam, "a"), 0) == 0 and counts.get((fam, "c"), 0) == 0, fam
    # batches of eight per family, one device call per (S, cap)
    for s in ai.SIZES:
        for cap in ai.caps(s):
            for fam in ai.FAMILIES[:-1]:
                assert sum(f == fam for f, *_ in sv[(s, cap)]) == ai.CHAINS
        for cap in ai.order_caps(s):
            assert [f for f, *_ in sv[(s, cap)]] == ["orders"] * 4
        assert set(ai.order_caps(s)) | set(ai.caps(s)) >= {c for c in (1, s - 2, s - 1, s + 5) if c > 0}


def test_sat_meets_pivot_ties_at_nearly_every_size():
    sv = _survey()
    for cap in (0, 3):
        sizes = [s for s in ai.SIZES if cap in ai.caps(s) and any(
            f == "sat" and ai.lu_stats(np.identity(s) - sig)[0] >= 1 for f, _, _, sig, _ in sv[(s, cap)])]
        print(f"cap {cap}: pivot ties in sat at {len(sizes)} sizes")
        if cap == 0:
            assert len(sizes) >= 55, sorted(set(ai.SIZES) - set(sizes))
    tied = {s for s in ai.SIZES for cap in ai.caps(s) for f, _, _, sig, _ in sv[(s, cap)]
            if f == "sat" and ai.lu_stats(np.identity(s) - sig)[0] >= 1}
    assert len(tied) >= 55


def test_swaps_onto_a_negative_pivot_at_most_sizes():
    sv = _survey()
    sizes = {s for s in ai.SIZES for cap in ai.caps(s) for _, _, c, sig, _ in sv[(s, cap)]
             if c == "b" and ai.lu_stats(np.identity(s) - sig)[1] >= 1}
    print(f"row swaps onto a negative pivot at {len(sizes)} sizes")
    assert len(sizes) >= 40, sorted(sizes)


def test_singular_chains_at_several_sizes_and_panels():
    sv = _survey()
    found = []
    for (s, cap), rows in sv.items():
        for idx, (f, k, c, _, _) in enumerate(rows):
            if c == "a" and f != "tiny_pivot":   # (those follow getf2's rule below DBL_MIN, not a plain LU)
                col = ai.lu_stats(np.identity(s) - _w01(s, cap, idx))[2]
                assert col is not None, (s, cap, f, k)
                found.append((s, cap, f, k, col))
    print("class (a): (S, cap, family, chain, first zero pivot's column):", found)
    assert len({s for s, *_ in found}) >= 3
    assert any(col < 8 for *_, col in found)
    assert any(2 * col >= s for s, *_, col in found)
    # the planted zero columns are met where they were put, and sat_stale has its own
    for s in ai.SINGULAR_SIZES:
        cols = [col for s_, _, f, _, col in found if s_ == s and f == "singular"]
        assert cols == list(ai.singular_columns(s)), (s, cols)
    assert any(f == "sat_stale" for _, _, f, _, _ in found)
    # S = 40 (panels of 20, 10 and 6) and S = 64 (32, 16, 8): the first, a middle and the last panel
    assert ai.singular_columns(40) == (1, 21, 39) and ai.singular_columns(64) == (1, 33, 63)


def test_pivots_below_dbl_min_in_every_class():
    """The tiny_pivot chains: scipy's own getrf leaves a non-zero |u_jj| below
    DBL_MIN on the diagonal of a chain whose inverse is finite at 30 or more
    sizes, S = 64 (the compile-time instance) among them; and some chains end in
    LinAlgError although getrf reports no zero pivot (getri's info)."""
    from scipy.linalg.lapack import dgetrf
    sv = _survey()
    tiny = np.finfo(np.float64).tiny
    sizes, by_getri, classes = set(), 0, {}
    for s in ai.SIZES:
        for idx, (f, k, c, _, _) in enumerate(sv[(s, 0)]):
            if f != "tiny_pivot":
                continue
            classes[c] = classes.get(c, 0) + 1
            lu, _, info = dgetrf(np.identity(s) - _w01(s, 0, idx))
            d = np.abs(np.diag(lu))
            if c == "b" and ((d > 0) & (d < tiny)).any():
                sizes.add(s)
            by_getri += c == "a" and info == 0
    print(f"tiny_pivot: classes {classes}; a finite inverse behind a pivot below DBL_MIN at {len(sizes)} sizes; "
          f"{by_getri} chains raise from getri")
    assert len(sizes) >= 30 and 64 in sizes and min(sizes) <= 8
    assert by_getri >= 1 and classes.get("c", 0) >= 1


def test_overflowing_chains_are_class_c():
    sv = _survey()
    for s in ai.OVERFLOW_SIZES:
        assert [c for f, _, c, _, _ in sv[(s, 0)] if f == "overflow"] == ["c"]
        pos, w = ai.overflow(s)
        assert np.isfinite(w).all() and np.array_equal(pos[0], np.arange(s))
    assert sum(c == "c" for rows in sv.values() for _, _, c, _, _ in rows) >= len(ai.OVERFLOW_SIZES)


def test_values_the_smooth_inputs_never_hold():
    sv = _survey()
    neg0 = sub = one = 0
    tiny = np.finfo(np.float64).tiny
    for rows in sv.values():
        for _, _, c, sig, anc in rows:
            if c != "b":
                continue
            neg0 += bool((np.signbit(anc) & (anc == 0)).any())
            sub += bool(((sig > 0) & (sig < tiny)).any())
            one += bool((sig == 1.0).any())
    print(f"class-(b) chains with a -0.0 in ancestor_x: {neg0}, a subnormal W~: {sub}, a W~ of exactly 1: {one}")
    assert neg0 >= 1 and sub >= 1 and one >= 1


def test_the_list_is_reproducible_and_read_only():
    pos, w, labels = ai.batch(40, 3)
    ai.batch.cache_clear()
    pos2, w2, labels2 = ai.batch(40, 3)
    assert np.array_equal(pos, pos2) and np.array_equal(w.view(np.uint64), w2.view(np.uint64)) and labels == labels2
    assert not w2.flags.writeable and not pos2.flags.writeable
