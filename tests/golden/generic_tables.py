"""Real-valued (generic) score tables of the exact_generic fixtures.

Shared by ``make_generic_goldens.py`` and the tests: a fixture stores only
the seed and a sha256 of the table bytes, and the tests regenerate the tables
here and check the hash before they compare anything.

Two kinds, entries ~ N(0, 1) from ``np.random.default_rng(seed)``:

* ``"shared"``: per-effect log-likelihood ratios R (S, E); every child shares
  parent j's row, T[i][j] = R[j], and U = [R; 0]
  (``nemo.nem.TableModel.from_log_ratios``);
* ``"own"``: every row T[i][j] and every row of U its own.
"""
import hashlib

import numpy as np

KINDS = ("shared", "own")


def generic_tables(kind, s, e, seed):
    """(U (S+1, E), T (S, S, E)) of one kind."""
    rng = np.random.default_rng(seed)
    if kind == "shared":
        r = rng.normal(0, 1, (s, e))
        t = np.empty((s, s, e))
        t[:] = r[None, :, :]
        return np.vstack([r, np.zeros((1, e))]), t
    if kind == "own":
        t = rng.normal(0, 1, (s, s, e))
        return rng.normal(0, 1, (s + 1, e)), t
    raise ValueError(kind)


def table_sha256(u, t):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(u, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(t, dtype=np.float64).tobytes())
    return h.hexdigest()


def step_inputs(s, seed):
    """(perm, raw W) of a step fixture: a random order and W ~ U(-3, 3) on its
    permissible entries (parent before child), 0 elsewhere."""
    rng = np.random.default_rng(1000 + seed)
    perm = rng.permutation(s)
    pos = np.argsort(perm)
    w = rng.uniform(-3, 3, (s, s))
    w[~(pos[:, None] > pos[None, :])] = 0.0
    return perm, w
