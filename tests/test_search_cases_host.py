"""CPU side of the cell-grid search tests: the brute-force reference of tests/_search_cases.py must
show that every family reaches the edge it was built for (so the GPU comparisons of
tests/test_gpu_search.py cannot pass vacuously), and the oracle's own kNN-5 (oracle_mo.cpp's Grid,
and the reference's kd-tree where oracle/_ref is built) must equal the brute force on the finite
families.
"""
import numpy as np
import pytest

import _search_cases as sc
import oracle_py

F = np.float32


@pytest.fixture(scope="module")
def expected():
    """family -> (map, queries, idx, d2, found, sixth), computed once."""
    out = {}
    for name, (m, groups) in sc.knn_families().items():
        q = sc.all_queries(groups)
        out[name] = (m, q) + sc.knn5_expected(q, m)
    return out


def _group_slices(groups):
    at, out = 0, {}
    for k, v in groups.items():
        out[k] = slice(at, at + len(v))
        at += len(v)
    return out


def test_reference_rule_on_a_hand_case():
    """(d, index) order, the d < 1.0 cut-off, NaN never wins, an empty result."""
    pts = np.array([[0, 0, 0, 0], [0.5, 0, 0, 0], [-0.5, 0, 0, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0], [0, 0.5, 0, 0],
                    [0, 0, -0.5, 0], [0, 0, 0, 0]], F)
    q = np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 0]], F)
    idx, d2, found, sixth = sc.knn5_expected(q, pts)
    assert idx[0].tolist() == [0, 7, 1, 2, 5] and d2[0].tolist() == [0, 0, 0.25, 0.25, 0.25]
    assert found.tolist() == [True, False, False] and sixth[0] == F(0.25)
    assert (idx[1:] == sc.INT_MAX).all() and np.isinf(d2[1:]).all()
    D, I = sc.brute_nn1(q, pts)
    assert I.tolist() == [0, sc.INT_MAX, sc.INT_MAX] and D[0] == 0 and np.isinf(D[1:]).all()
    D, I = sc.brute_nn1(q, pts[:0])
    assert (I == sc.INT_MAX).all() and np.isinf(D).all()


def test_coordinates_stay_inside_the_tested_range():
    for name, (m, groups) in {**sc.knn_families(), "sparse": sc.sparse(), "nonfinite": sc.nonfinite()}.items():
        for a in (m, sc.all_queries(groups)):
            xyz = a[:, :3]
            assert np.abs(xyz[np.isfinite(xyz)]).max() <= 524288, name


@pytest.mark.parametrize("t", sc.TRANSLATIONS)
def test_lattice_reaches_its_ties(expected, t):
    name = "lattice%+d" % t if t else "lattice"
    m, q, idx, d2, found, sixth = expected[name]
    assert len(m) == 2197 and found.all()
    tied = float((d2[:, 4] == sixth).mean())
    print(f"{name}: fifth == sixth distance for {tied:.1%} of the queries")
    assert tied >= 0.5
    if t == 0.0:
        assert (np.signbit(m[:, :3]) & (m[:, :3] == 0)).any(), "no -0.0f in the map"
        assert (sc.cell_of(m) < 0).any() and (m[:, :3] == np.floor(m[:, :3])).any()


def test_unit_reaches_the_cut_off(expected):
    m, groups = sc.unit()
    _, q, idx, d2, found, sixth = expected["unit"]
    g = _group_slices(groups)
    d6, _ = sc.brute_knn5(q, m, 7)
    inside = (d6 < F(1)).sum(axis=1)
    assert not found[g["on"]].any() and (inside[g["on"]] == 1).all() and (d6[g["on"], 1:4] == F(1)).all()
    centre = found[g["centre"]]
    assert centre.any() and (~centre).any()
    assert len(groups["four_in"]) >= 64 + 10 and len(groups["fifth_below"]) >= 10
    assert (inside[g["four_in"]] == 4).all() and (d6[g["four_in"], 4] == F(1)).all() and not found[g["four_in"]].any()
    assert found[g["fifth_below"]].all() and (d2[g["fifth_below"], 4] == sc.ONE_BELOW).all()


def test_threshold_shares(expected):
    m, groups = sc.threshold()
    _, q, idx, d2, found, sixth = expected["threshold"]
    assert len(q) == 1000 and all(len(v) == 250 for v in groups.values())
    # distinct cell corners 3 m apart
    corner = np.round(q[:, :3].astype(np.float64) / 3.0) * 3.0
    assert len(np.unique(corner, axis=0)) == 1000
    frac = np.abs(q[:, :3].astype(np.float64) - np.round(q[:, :3].astype(np.float64)))
    g = _group_slices(groups)
    for k, kind in enumerate(sc.THRESHOLD_KINDS):
        assert ((frac[g[kind]] <= 1e-3 + 1e-6).sum(axis=1) == 3 - k).all(), kind
    share_found = float(found.mean())
    qc = sc.cell_of(q)[found]
    moved = (sc.cell_of(m)[idx[found]] != qc[:, None, :]).sum(axis=2)  # [found, 5]: axes on which the cell differs
    assert (moved <= 3).all() and (np.abs(sc.cell_of(m)[idx[found]] - qc[:, None, :]) <= 1).all()
    share_corner = float((moved == 3).any(axis=1).mean())
    share_edge = float((moved == 2).any(axis=1).mean())
    d5, _ = sc.brute_knn5(q, m, 5)
    share_fifth = float((np.abs(d5[:, 4].astype(np.float64) - 1.0) <= 1e-2).mean())
    print(f"threshold: found {share_found:.1%}, corner-neighbour cell {share_corner:.1%}, edge-neighbour cell "
          f"{share_edge:.1%}, fifth within 1e-2 of 1.0 {share_fifth:.1%}")
    assert 0.3 <= share_found <= 0.7
    assert share_corner >= 0.10
    assert share_edge >= 0.25
    assert share_fifth >= 0.5
    d8, _ = sc.brute_knn5(q, m, 9)  # the query's own eight, then nothing within 1.08 m
    assert d8[:, :8].min() >= 0.9699 and d8[:, :8].max() <= 1.0201 and d8[:, 8].min() > 1.08 ** 2


def test_sparse_shares():
    m, groups = sc.sparse()
    D, _ = sc.brute_nn1(sc.all_queries(groups), m)
    assert (D >= F(2.5 * 2.5)).all() and (D <= F(6.6 * 6.6)).all()
    far, near = float((D >= F(9)).mean()), float((D < F(25)).mean())
    print(f"sparse: d^2 >= 9 for {far:.1%}, d^2 < 25 for {near:.1%}")
    assert far >= 1 / 3 and near >= 1 / 3


def test_nonfinite_has_every_kind():
    m, groups = sc.nonfinite()
    for a in (m, groups["poisoned"]):
        xyz = a[:, :3]
        assert np.isnan(xyz).any() and (xyz == np.inf).any() and (xyz == -np.inf).any()
    assert np.isfinite(groups["finite"]).all()
    assert abs(int((~np.isfinite(m[:, :3])).any(axis=1).sum()) - 22) <= 1


def test_same_answers():
    for n in sc.SAME_SIZES:
        for alt in (False, True):
            m, groups = sc.same(n, alt)
            D, I = sc.brute_nn1(groups["all"], m)
            assert set(I.tolist()) <= ({0, 1} if alt and n > 1 else {0}), (n, alt)
            assert I[4] == 0 and (not alt or n == 1 or (I[1] == 1 and D[1] == 0))


def _oracle_equals(expected, name, knn):
    m, q, idx, d2, found, _ = expected[name]
    oi, od = oracle_py.knn5(m, q, knn)
    ofound = oi[:, 4] >= 0
    bad = np.flatnonzero(ofound != found)
    assert len(bad) == 0, f"{name}/{knn}: found differs at {bad[:5]}: d2 {d2[bad[:5]]}"
    bad = np.flatnonzero((od[found] != d2[found]).any(axis=1))
    assert len(bad) == 0, f"{name}/{knn}: d2 differs at {bad[:5]}"
    return oi[found], idx[found]


@pytest.mark.parametrize("name", list(sc.knn_families()))
def test_oracle_grid_equals_brute_force(expected, name):
    oi, bi = _oracle_equals(expected, name, "grid")
    np.testing.assert_array_equal(oi, bi)


@pytest.mark.parametrize("name", list(sc.knn_families()))
def test_reference_kdtree_agrees_on_distances(expected, name):
    """The kd-tree's order among equal distances is its own; d2 and found are not."""
    if oracle_py.ref_lib() is None:
        pytest.skip("oracle/_ref/libref_mo.so not built")
    oi, _ = _oracle_equals(expected, name, "kdtree")
    m, q, _, d2, found, _ = expected[name]
    # the indices it returns are points at those distances
    back = sc.dist2(q[found], m)
    np.testing.assert_array_equal(np.take_along_axis(back, oi.astype(np.int64), axis=1), d2[found])


def test_build_cases_cover_their_edges():
    cases = sc.build_cases()
    assert {f"n{n}" for n in sc.BUILD_SIZES} <= set(cases)
    a, b, P = cases["own_cells"]
    for g, n in ((a, 15), (b, 1023)):
        assert g["cap"] == n == len(np.unique(sc.cell_of(g["pts"]), axis=0))
    a, b, P = cases["one_cell"]
    assert len(np.unique(sc.cell_of(a["pts"]), axis=0)) == 1 and len(a["pts"]) > 1024
    a, b, P = cases["alternating_runs"]
    ca = sc.cell_of(a["pts"])[:, 0]
    assert (ca[1:] != ca[:-1]).all() and len(np.unique(ca)) == 2
    cb = sc.cell_of(b["pts"])[:, 0]
    runs = np.flatnonzero(np.diff(cb)) + 1
    assert (np.diff(runs) == 100).all() and (runs % 64 != 0).any() and len(cb) > 2048
    a, b, P = cases["ragged_P3"]
    assert P == 3 and np.diff(a["off"])[1] == 0 and np.diff(b["off"])[0] == 0
    a, b, P = cases["caps_apart"]
    assert a["cap"] > 4096 and b["cap"] <= 5
    a, b, P = cases["nonfinite"]
    assert not np.isfinite(a["pts"]).all() and not np.isfinite(b["pts"]).all()
