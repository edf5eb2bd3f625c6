"""The gfx950 compile of the shared numeric headers, call by call (csrc/llsr_math_debug.hip, where = 1:
one thread per case, the arithmetic is the header's) on the inputs of tests/_math_cases.py, whose
reach tests/test_math_cases_host.py shows on the CPU:

* every function of llsr_libm.h, llsr_eigen.h and of llsr_pg.h's double trigonometry and SO(3) charts
  gives in a kernel the bits the host compile gives (where = 0): every bit pattern, signed zeros
  included; any two NaNs are equal, as oracle/libm_check's same() has it, because the default NaN's
  sign differs between x86 and the GPU;
* and against the independent references directly: glibc's bits for the float ports, oracle_eigen.h's
  outputs and return codes for the Eigen restatement, at most 1 ulp from glibc for the double
  trigonometry on [-2 pi, 2 pi] / [-1, 1] (the bound and its reason: test_math_cases_host.py);
* ransac_k, the one place where the device's own log and pow decide a result (k_ground_elev_ransac's
  `iterations < k`): for every pair (K, cnt) of the domain the loop stops at the same iteration as
  with glibc's k. The number of pairs whose k differs in bits and the largest relative deviation are
  printed, not asserted; next to the margin test_math_cases_host.py asserts on the inputs they are the
  certificate DESIGN.md §2 quotes (deviation << margin). Measured on the MI355X: 903 941 of the
  11 185 126 pairs differ in bits, by at most 2.247e-13 relative (K = 1834, cnt = 145), against a
  margin of 1.508e-10.

One launch per function; the references and the host side are computed once per module."""
import numpy as np
import pytest

import _math_cases as mc

pytestmark = pytest.mark.gpu


def libm_inputs(fn):
    if mc.LIBM_FNS[fn] == "atan2f_":
        y, x = (np.concatenate(p) for p in zip(mc.atan2_grid(), mc.atan2_gaps()))
        return x, y
    return mc.libm_unary(fn), None


@pytest.fixture(scope="module")
def libm(require_gpu):
    out = {}
    for fn, name in enumerate(mc.LIBM_FNS):
        x, y = libm_inputs(fn)
        out[name] = {"x": x, "y": y, "dev": mc.debug_libm(fn, 1, x, y), "host": mc.debug_libm(fn, 0, x, y),
                     "ref": mc.ref_libm32(fn, x, y)}
    return out


@pytest.mark.parametrize("other", ["host", "ref"])
@pytest.mark.parametrize("name", mc.LIBM_FNS)
def test_libm_kernel_bits(libm, name, other):
    r = libm[name]
    bad = ~mc.same_bits(r["dev"], r[other])
    cols = (r["x"].view(np.uint32),) + (() if r["y"] is None else (r["y"].view(np.uint32),)) + (r["dev"], r[other])
    what = "the host compile" if other == "host" else "glibc"
    assert not bad.any(), (f"{name}: {bad.sum()} of {len(bad)} differ from {what}, first (x [y] device {other}, bits): "
                           + mc.first_inputs(bad, *cols))


def test_libm_trig_is_loud_from_120_on_the_device(require_gpu):
    x = mc.libm_loud()
    for fn in (4, 5, 6):
        assert np.isnan(mc.debug_libm(fn, 1, x).view(np.float32)).all(), mc.LIBM_FNS[fn]


@pytest.fixture(scope="module")
def eigen(require_gpu):
    out = {}
    for op, name in enumerate(mc.EIGEN_OPS):
        inp = mc.eigen_cases(op)
        out[name] = {"in": inp, "dev": mc.debug_eigen(op, 1, inp), "host": mc.debug_eigen(op, 0, inp), "ref": mc.ref_eigen(op, inp)}
    return out


@pytest.mark.parametrize("other", ["host", "ref"])
@pytest.mark.parametrize("name", mc.EIGEN_OPS)
def test_eigen_kernel_bits(eigen, name, other):
    r = eigen[name]
    (got, ginfo), (want, winfo) = r["dev"], r[other]
    same = mc.same_bits(got.view(np.uint32), want.view(np.uint32))
    bad = ~same.all(1) | (ginfo != winfo)
    what = "the host compile" if other == "host" else "oracle_eigen"
    j = np.flatnonzero(bad)[:5]
    assert not bad.any(), (f"{name}: {bad.sum()} of {len(bad)} cases differ from {what}; first cases {j}, their first differing "
                           f"outputs {[int(np.argmin(same[k])) for k in j]}, codes {ginfo[j]} / {winfo[j]}, inputs {r['in'][j]!r}")


@pytest.fixture(scope="module")
def pg(require_gpu):
    return {name: (mc.debug_pg(fn, 1, mc.pg_cases(fn)), mc.debug_pg(fn, 0, mc.pg_cases(fn))) for fn, name in enumerate(mc.PG_FNS)}


@pytest.mark.parametrize("name", mc.PG_FNS)
def test_pg_kernel_bits_equal_host_compile(pg, name):
    dev, host = pg[name]
    bad = ~mc.same_bits(dev, host).all(1)
    inp = mc.pg_cases(mc.PG_FNS.index(name))
    assert not bad.any(), (f"{name}: {bad.sum()} of {len(bad)} cases differ from the host compile, first (input device host): "
                           + mc.first_inputs(bad, inp, dev.view(np.float64), host.view(np.float64)))


@pytest.mark.parametrize("name", list(mc.PG_REF))
def test_pg_trig_kernel_within_one_ulp_of_glibc(require_gpu, name):
    assert (msg := mc.check_pg_trig(name, 1)) is None, msg


def test_ransac_k_kernel_stops_where_glibc_does(require_gpu):
    K, cnt = mc.ransac_pairs()
    dev, want = mc.debug_ransac_k(1, K, cnt), mc.ref_ransac_k(K, cnt)
    differ = dev.view(np.uint64) != want.view(np.uint64)
    dom = want <= 10002
    rel = np.abs(dev[dom] - want[dom]) / want[dom]
    j = np.argmax(rel)
    print(f"ransac_k: {differ.sum()} of {len(K)} pairs differ from glibc in bits ({(differ & dom).sum()} of {dom.sum()} with "
          f"k <= 10002); largest relative deviation there {rel[j]:.3e} at K = {K[dom][j]}, cnt = {cnt[dom][j]}")
    bad = mc.stop_count(dev) != mc.stop_count(want)
    assert not bad.any(), f"{bad.sum()} stopping counts differ, first (K cnt device glibc): " + mc.first_inputs(bad, K, cnt, dev, want)
    host = mc.debug_ransac_k(0, K, cnt)
    assert np.array_equal(mc.stop_count(dev), mc.stop_count(host))
