"""The models of the true-graph score fixtures (``real_score_<name>.npz``),
rebuilt identically by ``make_real_score_goldens.py`` and by the tests.

A bundled network is read from ``tests/golden/networks``; a synthetic one is
``generator.synthetic_nem(S, E, seed, edge_p=...)``.
"""
from __future__ import annotations

import os

HERE = os.path.dirname(os.path.abspath(__file__))

FIXTURES = {
    # name: bundled CSV, or (S, E, seed, edge_p)
    "net2": "network2.csv",                 # 11 x 184; the four values of net2_tables.npz
    "network5": "networks/network5.csv",    # 15 x 267; 5 and 4 sweeps
    "network17": "networks/network17.csv",  # 34 x 367; 561 pairs
    "network13": "networks/network13.csv",  # 34 x 285
    "65x70": (65, 70, 3, 0.1),              # S > 64: the forward with order weights changes kernels
    "3x5200": (3, 5200, 1, 0.6),            # E past the register pair kernels' 5120
    "2x1": (2, 1, 0, 0.9),                  # one pair, three elements
}


def network_inputs(name, utils, generator):
    """(adj, end_nodes, errors, S, E) of fixture ``name`` with the given
    ``utils.read_csv_to_adj`` and ``generator`` (the golden script passes the
    reference programme's utils, the tests the package's)."""
    f = FIXTURES[name]
    if isinstance(f, str):
        return utils.read_csv_to_adj(os.path.join(HERE, f))
    s, e, seed, edge_p = f
    net = generator.synthetic_network(s, e, seed, edge_p=edge_p)
    return net.adj.copy(), net.end_nodes, net.errors, s, e


def call_tables(nem, call):
    """(U, T) of the constructor's ``call`` ("real" / "obs"): the tables of
    that knockdown matrix, U's null row from the observed one (nem.py:62)."""
    import numpy as np
    k = nem.real_knockdown_mat if call == "real" else nem.observed_knockdown_mat
    t = np.array(nem.get_score_tensor(k))
    return nem.get_node_lr_table(t), t


def build_nem(name):
    """The package's NEM of fixture ``name``."""
    from nemo import NEM, generator, utils
    adj, end, err, s, e = network_inputs(name, utils, generator)
    return NEM(adj, end, err, s, e)
