"""The cell-grid build (k_grid_clear / insert / alloc / scatter through the production grid_build,
both grids of a call) checked from the dumped tables against what the build promises
(llsr_grid.h): the occupied slots are exactly the cloud's distinct cells, each once, with its
population; the ranges partition [0, n); a range of the copy is a permutation of the cell's points
with their original indices; every key is reached by linear probing from its hash slot; an empty
problem's table is empty. cell_coord / cell_key / cell_hash / grid_log2_table are restated here in
numpy. The cases (tests/_search_cases.py build_cases) are the sizes and orders at which the insert's
wave runs, 1024-point chunks and LDS hash, the one-slot headroom of the table and the early returns
of the smaller grid's surplus blocks come into play.
"""
import ctypes as C

import numpy as np
import pytest

import _search_cases as sc
from llsr import lib

pytestmark = pytest.mark.gpu

SLOT = np.dtype([("key", "<u8"), ("start", "<i4"), ("count", "<i4")])
EMPTY = np.uint64(2**64 - 1)
SENTINEL = 1048500


def cell_coord(v):
    with np.errstate(invalid="ignore"):
        f = np.floor(np.asarray(v, np.float32))
        ok = (f > np.float32(-1048000.0)) & (f < np.float32(1048000.0))
        return np.where(ok, np.where(ok, f, 0).astype(np.int64), SENTINEL)


def cell_key(xyz):
    c = (cell_coord(xyz) + 1048576).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def cell_hash(key, log2T):
    return ((key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - log2T)).astype(np.int64)


def log2_table(cap):
    l = 4
    while (1 << l) <= max(cap, 1):
        l += 1
    return l


def grid_build(a, b, P):
    f = lib().llsr_debug_grid_build
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    keep, args, outs = [], [], []
    for g in (a, b):
        pts = np.ascontiguousarray(g["pts"], np.float32)
        off = np.ascontiguousarray(g["off"], np.int64)
        tab = np.zeros((P, 1 << log2_table(g["cap"])), SLOT)
        copy = np.zeros((P, g["cap"], 4), np.float32)
        keep += [pts, off]
        args += [pts.ctypes.data, off.ctypes.data, g["cap"]]
        outs += [tab, copy]
    log2T = np.zeros(2, np.int32)
    rc = f(*args, P, log2T.ctypes.data, *(o.ctypes.data for o in outs))
    assert rc == 0, f"llsr_debug_grid_build: {rc}"
    return log2T, outs


def check_grid(g, p, log2T, tab, copy):
    """One problem of one grid; returns a list of findings."""
    errs = []
    pts = np.asarray(g["pts"], np.float32)[g["off"][p]:g["off"][p + 1]][:g["cap"]]
    n = len(pts)
    if log2T != log2_table(g["cap"]) or len(tab) != 1 << log2T:
        return [f"log2T {log2T} for cap {g['cap']}"]
    used = np.flatnonzero(tab["key"] != EMPTY)
    if n == 0:
        if len(used) or tab["count"].any():
            errs.append("an empty problem's table is not empty")
        return errs
    keys = cell_key(pts[:, :3])
    want, pop = np.unique(keys, return_counts=True)
    have = tab["key"][used]
    order = np.argsort(have)
    if not np.array_equal(have[order], want):
        return [f"occupied keys are not the cloud's distinct cells, each once: {len(have)} slots, {len(want)} cells"]
    if not np.array_equal(tab["count"][used][order], pop):
        errs.append("count is not the cell's population")
    if tab["count"][tab["key"] == EMPTY].any():
        errs.append("an empty slot has a count")
    start, count = tab["start"][used].astype(np.int64), tab["count"][used].astype(np.int64)
    by_start = np.argsort(start)
    if start[by_start][0] != 0 or not np.array_equal(start[by_start][1:], (start + count)[by_start][:-1]) \
            or (start + count).max() != n:
        return errs + ["the ranges do not partition [0, n)"]
    # the copy: a range holds its cell's points, each with its original index, each once
    idx = copy[:n, 3].view(np.uint32).astype(np.int64)
    if not np.array_equal(np.sort(idx), np.arange(n)):
        return errs + ["the copy's index bits are not a permutation of [0, n)"]
    if not np.array_equal(copy[:n, :3].view(np.uint32), pts[idx, :3].view(np.uint32)):
        errs.append("a copied point differs from the original at its index")
    slot_of_pos = np.repeat(used[by_start], count[by_start])
    if not np.array_equal(tab["key"][slot_of_pos], keys[idx]):
        errs.append("a point lies in another cell's range")
    if (copy[n:].view(np.uint32) != 0xFFFFFFFF).any():
        errs.append("the copy was written past n")
    # linear probing from the hash slot reaches the key before an empty slot
    T = 1 << log2T
    gap = (used - cell_hash(have, log2T)) % T
    for s, d in zip(used, gap):
        if d and (tab["key"][(s - np.arange(1, d + 1)) % T] == EMPTY).any():
            errs.append(f"slot {s}: an empty slot between the hash slot and the key")
            break
    return errs


@pytest.mark.parametrize("name", list(sc.build_cases()))
def test_grid_build_invariants(require_gpu, name):
    a, b, P = sc.build_cases()[name]
    log2T, (ta, ca, tb, cb) = grid_build(a, b, P)
    errs = []
    for which, g, l2, tab, copy in (("a", a, log2T[0], ta, ca), ("b", b, log2T[1], tb, cb)):
        for p in range(P):
            errs += [f"{name} grid {which} problem {p}: {e}" for e in check_grid(g, p, int(l2), tab[p], copy[p])]
    assert not errs, "\n".join(errs)
    if name == "own_cells":  # the table is one slot short of full
        assert (ta["key"] != EMPTY).sum() == 15 == len(ta[0]) - 1 and (tb["key"] != EMPTY).sum() == 1023 == len(tb[0]) - 1


def test_grid_build_rejects_bad_arguments(require_gpu):
    a, b, P = sc.build_cases()["n5"]
    f = lib().llsr_debug_grid_build
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    pts, off, out = a["pts"], a["off"], np.zeros(4096, np.uint8)
    o = out.ctypes.data
    bad_off = np.array([0, 5, 3], np.int64)
    assert f(pts.ctypes.data, off.ctypes.data, 0, pts.ctypes.data, off.ctypes.data, 5, 1, o, o, o, o, o) != 0
    assert f(pts.ctypes.data, off.ctypes.data, 5, pts.ctypes.data, off.ctypes.data, 5, 0, o, o, o, o, o) != 0
    assert f(pts.ctypes.data, bad_off.ctypes.data, 5, pts.ctypes.data, bad_off.ctypes.data, 5, 2, o, o, o, o, o) != 0
    assert f(None, off.ctypes.data, 5, pts.ctypes.data, off.ctypes.data, 5, 1, o, o, o, o, o) != 0
