"""The register-resident DBSCAN merge (k_dbscan_merge, M <= kDbL) against a literal transcription
of DBSCAN_EdgeFeature's merge loop (featureAssociation.cpp:1342-1386) and of the cluster run-length
filter (featureAssociation.cpp:1281-1305), through llsr_debug_dbscan_merge: the production kernel
over a batch of neighbourhood relations given as bit rows. cluster, sharp and n_sharp are compared
exactly.

Sizes: every M at which the kernel's ownership (lane l owns l + 64 e) or its instantiation changes.
Families: four random ones (symmetric reflexive; reflexive asymmetric; diagonal kept with
probability 0.8; 10 % empty rows), a path i ~ i +- 1 and a "comb" (singletons first, then points that
are neighbours of three or more of them).

Coverage is asserted on the reference before the device is compared, so a pass is not vacuous. Each
random family, over its relations with M >= 63, must contain a visit that opens a new label, one
that merges >= 3 distinct labels, one that collapses unvisited zeros into min_label, and a kept and a
dropped run in the filter. The two constructed families cannot show all of that by construction and
assert what they are built for: the path carries ONE label across every 64-lane boundary (its
second visit collapses every unvisited point into label 1, so nothing else can happen), the comb
merges >= 3 distinct labels while 0 is in the list and has kept and dropped runs.

The host test pins the transcription itself against tests/test_dbscan_uf.py's reference_merge on
the same families at M <= 129, with no device.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_dbscan_uf import reference_merge

K_ADJ_CAP, K_ADJ_WORDS = 2048, 64  # llsr_device.h kAdjCap, kAdjWords
SIZES = {1024: (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 1023, 1024), 2048: (65, 1025, 2047, 2048)}
RANDOM_FAMILIES = ("symmetric", "asymmetric", "diag08", "empty_rows")
FAMILIES = RANDOM_FAMILIES + ("path", "comb")
COVER = ("opens", "merges3", "collapses", "kept", "dropped")


def literal_merge(adj):
    """FA:1342-1386 on a boolean relation adj[i, j] (eps(i, j) <= DBFr); returns cluster and what
    the run contained."""
    M = adj.shape[0]
    cluster = np.zeros(M, np.int64)
    label = 0
    seen = dict(opens=False, merges3=False, collapses=False, merges3_with_zero=False)
    for i in range(M):
        cluster[i] = 0
        in_idx = np.flatnonzero(adj[i])
        in_label_list = cluster[in_idx]
        min_label = 999999999
        for v in in_label_list:
            if v != 0 and v < min_label:
                min_label = int(v)
        if min_label <= label:
            in_label_list = np.unique(in_label_list)  # sort + unique + erase
            hit = np.isin(cluster, in_label_list)  # cluster[j] == in_label_list[k] for some k
            if np.count_nonzero(in_label_list) >= 3:
                seen["merges3"] = True
                seen["merges3_with_zero"] |= bool((in_label_list == 0).any())
            if (in_label_list == 0).any() and (cluster[i + 1:] == 0).any():
                seen["collapses"] = True
            cluster[hit] = min_label
            cluster[in_idx] = min_label
        else:
            label += 1
            cluster[in_idx] = label
            seen["opens"] = True
    return cluster, seen


def literal_filter(cluster):
    """FA:1281-1305: positions of the points whose label is in cluster_inlier, in order."""
    cluster_length = sorted(int(v) for v in cluster)
    cluster_num_list = []
    cluster_cnt = 1
    for i in range(len(cluster_length) - 1):
        if cluster_length[i + 1] - cluster_length[i] == 0:
            cluster_cnt += 1
        else:
            cluster_num_list.append(cluster_cnt)
            cluster_cnt = 1
    cluster_inlier = [i + 1 for i, n in enumerate(cluster_num_list) if n >= 4]
    sharp = [i for i in range(len(cluster)) if int(cluster[i]) in cluster_inlier]
    seen = dict(kept=bool(cluster_inlier), dropped=any(n < 4 for n in cluster_num_list))
    return np.asarray(sharp, np.int32), seen


def relation(family, M, rng):
    if family == "path":
        adj = np.zeros((M, M), bool)
        i = np.arange(M)
        adj[i, i] = True
        adj[i[1:], i[:-1]] = True
        adj[i[:-1], i[1:]] = True
        return adj
    if family == "comb":
        # the "even" points first, each only its own neighbour; then the "odd" points, each its own
        # neighbour and a neighbour of 3 to 5 earlier singletons (labels still distinct or merged)
        adj = np.zeros((M, M), bool)
        n1 = (M + 1) // 2
        adj[np.arange(M), np.arange(M)] = True
        if n1 >= 3:
            for i in range(n1, M):
                adj[i, rng.choice(n1, int(rng.integers(3, 6)), replace=False)] = True
        return adj
    # A sparse background (mean degree ~1: many small clusters, several merges). A uniform relation
    # alone almost never merges three labels: once a visit has a labelled neighbour and a zero in
    # its list (itself), every unvisited point takes that label, and only isolated points open new
    # ones. So at M >= 63 the first visits are six seeds of disjoint groups (each opens a label for
    # its four members) and then two bridges, each a neighbour of one member of three groups: the
    # bridge merges three distinct labels with 0 in its list and collapses the unvisited points.
    adj = rng.random((M, M)) < min(0.5, 1.0 / max(M, 1))
    structured = M >= 63
    if structured:
        adj[:8] = False
        adj[:, :8] = False
        members = 8 + rng.permutation(M - 8)[:24].reshape(6, 4)
        for g in range(6):
            adj[g, members[g]] = True
        adj[6, members[0:3, 0]] = True
        adj[7, members[3:6, 0]] = True
    if family != "asymmetric":
        adj = adj | adj.T
    np.fill_diagonal(adj, rng.random(M) < 0.8 if family == "diag08" else True)
    if family == "empty_rows":
        empty = rng.random(M) < 0.1
        if structured:
            empty[:8] = False
        adj[empty] = False
    return adj


@functools.lru_cache(maxsize=None)
def case(family, kDbL):
    """The batch of one family at one kDbL: relations, reference results, coverage. Computed once."""
    rng = np.random.default_rng([FAMILIES.index(family), kDbL])
    sizes = SIZES[kDbL]
    if family == "path" and kDbL == 1024:
        sizes = (129, 1024)
    rels = [relation(family, M, rng) for M in sizes]
    rels = [rels[-2]] + rels + [rels[-2]]  # the same relation at batch positions 0 and n - 1
    refs, cover = {}, dict.fromkeys(COVER + ("merges3_with_zero",), False)
    out = []
    for adj in rels:
        if id(adj) not in refs:
            cluster, s1 = literal_merge(adj)
            sharp, s2 = literal_filter(cluster)
            refs[id(adj)] = (cluster.astype(np.int32), sharp)
            if adj.shape[0] >= 63:
                for k, v in {**s1, **s2}.items():
                    cover[k] |= v
        out.append((adj,) + refs[id(adj)])
    return out, cover


def assert_coverage(family, cover, rels):
    if family in RANDOM_FAMILIES:
        missing = [k for k in COVER if not cover[k]]
    elif family == "comb":
        missing = [k for k in ("opens", "merges3", "merges3_with_zero", "collapses", "kept", "dropped") if not cover[k]]
    else:  # path: one label over the whole chain, so over every 64-lane boundary
        missing = [] if all((c == 1).all() for _, c, _ in rels if len(c) > 64) else ["one label"]
    assert not missing, f"{family}: the reference run lacks {missing}"


def pack_rows(adj, rng):
    """[kAdjCap][kAdjWords] bit rows as k_dbscan_adj leaves them: rows below M, both words of every
    64-point chunk below M; everything else is never written, so it is filled with noise here."""
    M = adj.shape[0]
    rows = rng.integers(0, 2**32, (K_ADJ_CAP, K_ADJ_WORDS), dtype=np.uint64).astype(np.uint32)
    if M:
        nw = 2 * ((M + 63) // 64)
        bits = np.zeros((M, nw * 32), bool)
        bits[:, :M] = adj
        rows[:M, :nw] = np.packbits(bits, axis=1, bitorder="little").view("<u4")
    return rows


def device_merge(rels, kDbL):
    from llsr import lib
    f = lib().llsr_debug_dbscan_merge
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(rels)
    rng = np.random.default_rng(99)
    adj = np.stack([pack_rows(r[0], rng) for r in rels])
    M = np.asarray([r[0].shape[0] for r in rels], np.int32)
    cluster = np.zeros((n, K_ADJ_CAP), np.int32)
    sharp = np.zeros((n, K_ADJ_CAP), np.int32)
    n_sharp = np.zeros(n, np.int32)
    assert f(adj.ctypes.data, M.ctypes.data, n, kDbL, cluster.ctypes.data, sharp.ctypes.data, n_sharp.ctypes.data) == 0
    return cluster, sharp, n_sharp


@pytest.mark.gpu
@pytest.mark.parametrize("kDbL", (1024, 2048))
@pytest.mark.parametrize("family", FAMILIES)
def test_merge_matches_literal_loop(require_gpu, family, kDbL):
    rels, cover = case(family, kDbL)
    assert_coverage(family, cover, rels)
    cluster, sharp, n_sharp = device_merge(rels, kDbL)
    bad = []
    for k, (adj, ref_cluster, ref_sharp) in enumerate(rels):
        M = adj.shape[0]
        ok = (np.array_equal(cluster[k, :M], ref_cluster) and n_sharp[k] == len(ref_sharp)
              and np.array_equal(sharp[k, :len(ref_sharp)], ref_sharp))
        if not ok:
            bad.append((k, M))
    assert not bad, f"{family}, kDbL {kDbL}: (batch position, M) {bad} differ from the literal loop"
    # batch independence: the same relation at positions 0 and n - 1
    assert np.array_equal(cluster[0], cluster[-1]) and np.array_equal(sharp[0], sharp[-1])
    assert n_sharp[0] == n_sharp[-1]


@pytest.mark.parametrize("family", FAMILIES)
def test_literal_loop_matches_reference_merge(family):
    rng = np.random.default_rng([FAMILIES.index(family), 7])
    for M in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        adj = relation(family, M, rng)
        cluster, _ = literal_merge(adj)
        assert cluster.tolist() == reference_merge(adj), (family, M)


def test_reference_coverage_holds_without_a_device():
    """The coverage conditions are properties of the seeded relations: checked on every machine."""
    for kDbL in SIZES:
        for family in FAMILIES:
            rels, cover = case(family, kDbL)
            assert_coverage(family, cover, rels)
