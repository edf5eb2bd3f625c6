"""The segmented VoxelGrid's exact sort (llsr_map.hip k_is_level / k_is_leaf) on adversarial voxel-id
sequences, through LocalMap.voxel_grid, bit for bit against the oracle's pcl::VoxelGrid.

* A cloud is built from a voxel-id sequence: point t sits at x = (id[t] + 0.5) * leaf with y, z inside
  one voxel, so points that share an id land in one voxel and their float sums depend on the order
  std::sort leaves equal ids in.
* Patterns from all-equal to the median-of-3 killer at every size where the code changes path: up to
  1024 a cloud is one leaf (a window of 64 / wave partitions), above it k_is_level partitions first
  and the leaves inherit their depth limit.
* The deep-stack cloud (8192 points, depth limit 26): its first partition cuts at 1000, and the left
  part is a McIlroy-style adversary against the left-first introsort loop, so the wave that finishes
  it holds one pending right part per level of its inherited depth limit, 25, more than the 24 that
  suffice for a ring's sort.
A CPU replay of the recursion shows which cases reach what: the deep-stack leaf's 25 pending right
parts, and the killer at 1000 and 1024 spending its depth limit in a leaf range above 64 (heap sort
by the wave).
"""
import numpy as np
import pytest

import oracle_py
from llsr import LocalMap
from test_gpu_vox_split import _killer, _sweep

pytestmark = pytest.mark.gpu
LEAF = 0.2
IS_LEAF = 1024  # llsr_map.hip kIsLeaf: ranges above it are partitioned in global memory, level by level
SIZES = (2, 16, 17, 64, 65, 128, 129, 1000, 1023, 1024, 1025, 2048, 4096)
DEEP_N, DEEP_LEAF = 8192, 1000


def _partition(v, f, l, lt):
    """One libstdc++ step on v[f, l): __move_median_to_first(first, first+1, mid, last-1), then
    __unguarded_partition; returns the cut."""
    a, b, c = f + 1, f + (l - f) // 2, l - 1
    if lt(v[a], v[b]):
        m = b if lt(v[b], v[c]) else (c if lt(v[a], v[c]) else a)
    else:
        m = a if lt(v[a], v[c]) else (c if lt(v[b], v[c]) else b)
    v[f], v[m] = v[m], v[f]
    p, i, j = v[f], f + 1, l
    while True:
        while lt(v[i], p):
            i += 1
        j -= 1
        while lt(p, v[j]):
            j -= 1
        if not i < j:
            return i
        v[i], v[j] = v[j], v[i]
        i += 1


def _replay(ids):
    """The recursion as the device runs it. Ranges above IS_LEAF: one partition per level, both parts
    pushed. A range at or below it: one wave, left part first while above 64 with depth left, every
    right part pending on its stack. Returns (the most right parts any wave holds at once, the sizes
    of the leaf ranges above 64 that reach depth limit 0)."""
    v = [int(x) for x in ids]
    n = len(v)
    lt = lambda x, y: x < y
    most, spent = 0, []
    level = [(0, n, 2 * (n.bit_length() - 1))] if n > 1 else []
    leaves = []
    while level:
        f, l, d = level.pop()
        if l - f <= IS_LEAF:
            leaves.append((f, l, d))
        elif d > 0:  # d == 0 above IS_LEAF: heap-sorted by one lane, no leaf
            cut = _partition(v, f, l, lt)
            level += [(f, cut, d - 1), (cut, l, d - 1)]
    for f, l, d in leaves:
        stack = [(f, l, d)]
        while stack:
            f, l, d = stack.pop()
            while l - f > 64 and d > 0:
                d -= 1
                cut = _partition(v, f, l, lt)
                stack.append((cut, l, d))
                l = cut
            most = max(most, len(stack))
            if l - f > 64:
                spent.append(l - f)
    return most, spent


def _adversary_leaf(n, depth):
    """Values 0..n-1 on which the left-first introsort loop with depth limit `depth` keeps its left
    part large at every step (McIlroy's adversary, mirrored): an unknown value compares below every
    frozen one; when two unknown values meet, the pivot candidate is frozen to the highest free
    value. Element 0 is frozen as the maximum beforehand."""
    val = [None] * n
    free = [n - 1]
    cand = [None]

    def freeze(x):
        val[x] = free[0]
        free[0] -= 1

    def lt(x, y):
        if val[x] is None and val[y] is None:
            freeze(x if x == cand[0] else y)
        if val[x] is None:
            cand[0] = x
            return val[y] is not None  # unknown < frozen
        if val[y] is None:
            cand[0] = y
            return False
        return val[x] < val[y]

    freeze(0)
    items = list(range(n))
    l = n
    for _ in range(depth):
        if l <= 64:
            break
        l = _partition(items, 0, l, lt)
    for x in range(n):
        if val[x] is None:
            freeze(x)
    return np.array(val, np.int64)


def _deep_stack_ids(rng):
    L = _adversary_leaf(DEEP_LEAF, 2 * (DEEP_N.bit_length() - 1) - 1)
    a = rng.integers(1000, 3000, DEEP_N)
    a[1:DEEP_LEAF] = L[1:]
    a[DEEP_N // 2] = L[0]  # the first pivot (the median of a[1], a[mid], a[last - 1]); cut = DEEP_LEAF
    return a


def _cases():
    rng = np.random.default_rng(77)
    cases = []
    for n in SIZES:
        cases += [("equal", np.full(n, 7)), ("two", rng.integers(0, 2, n)), ("ascending", np.arange(n)),
                  ("descending", np.arange(n)[::-1].copy()), ("sweep", _sweep(rng, n)),
                  ("killer", _killer(n + (n & 1), False)[:n]), ("killer ties", _killer(n + (n & 1), True)[:n])]
    cases.append(("deep stack", _deep_stack_ids(rng)))
    return [(name, np.asarray(ids, np.int64)) for name, ids in cases]


def _cloud(rng, ids):
    n = len(ids)
    c = np.empty((n, 4), np.float32)
    c[:, 0] = ((ids + 0.5) * LEAF).astype(np.float32)
    c[:, 1:3] = (rng.uniform(0.05, 0.95, (n, 2)) * LEAF).astype(np.float32)
    c[:, 3] = rng.uniform(0.0, 100.0, n).astype(np.float32)
    # PCL's key: floor(x * inverse_leaf_size), inverse_leaf_size = 1 / 0.2f as a float
    for inv in (np.float32(5.0), np.float32(1.0) / np.float32(LEAF)):
        assert np.array_equal(np.floor(c[:, 0] * inv).astype(np.int64), ids)
        assert (np.floor(c[:, 1:3] * inv) == 0).all()
    return c


def test_segmented_sort_adversarial_clouds(require_gpu):
    cases = _cases()
    most = {(name, len(ids)): _replay(ids) for name, ids in cases}
    deep = most[("deep stack", DEEP_N)][0]
    heaped = [k for k, (_, spent) in most.items() if k[0].startswith("killer") and spent]
    print("pending right parts, deep-stack cloud:", deep)
    print("depth limit spent in a leaf range above 64:", [(k, most[k][1]) for k in heaped])
    assert deep > 24, f"the deep-stack leaf reaches {deep} pending right parts, not more than 24"
    assert any(n in (1000, 1024) for _, n in heaped), "no killer case of 1000 or 1024 reaches the wave's heap sort"

    rng = np.random.default_rng(78)
    clouds = [_cloud(rng, ids) for _, ids in cases]
    m = LocalMap(0)
    outs = [g.detach().cpu().numpy() for g in m.voxel_grid(clouds, [LEAF] * len(clouds))]
    m.close()
    bad = []
    for (name, ids), c, got in zip(cases, clouds, outs):
        ref = oracle_py.voxel_grid(c, LEAF)
        if got.shape != ref.shape or not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
            bad.append((name, len(ids)))
    assert not bad, f"clouds {bad} differ from pcl::VoxelGrid"
