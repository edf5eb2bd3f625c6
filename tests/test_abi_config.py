"""CPU tests of llsr_create's configuration validation (include/llsr.h, next to llsr_config): the
configurations the reference's arithmetic does not define are refused with LLSR_EINVAL before the
device query, so this runs without a device; every other value passes the validation (LLSR_OK with a
device, LLSR_ENODEV without one)."""
import ctypes as C

import pytest

import llsr
from llsr import _abi

LLSR_ENODEV = -19


def _create_rc(**fields):
    """llsr_create's return code for the VLP-16 block with `fields` set (a handle is destroyed)."""
    cfg = llsr.default_config("vlp16")
    for k, v in fields.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = llsr.lib().llsr_create(C.byref(cfg), 0, 1, 1000, C.byref(h))
    if h.value:
        llsr.lib().llsr_destroy(h)
    return rc


_FLOAT_FIELDS = [n for n, t in _abi.Config._fields_ if t is C.c_float]
_RANGED = ("vertical_angle_bottom", "vertical_angle_top", "segment_theta")  # 3.4e38 is no neighbour of theirs
_INF, _NAN = float("inf"), float("nan")


def test_every_float_field_is_covered():
    assert len(_FLOAT_FIELDS) == 13 and set(_RANGED) <= set(_FLOAT_FIELDS)


@pytest.mark.parametrize("refused,accepted", [
    # (a configuration the reference's arithmetic does not define, an accepted neighbour of it)
    (dict(vertical_angle_top=-15.0), dict(vertical_angle_top=-14.99)),   # top == bottom: resolution 0
    (dict(vertical_angle_top=-20.0), dict(vertical_angle_bottom=-20.0)),  # top < bottom
    (dict(scan_period=0.0), dict(scan_period=1e-6)),
    (dict(scan_period=-0.1), dict(scan_period=0.05)),
    (dict(segment_theta=0.0), dict(segment_theta=0.001)),
    (dict(segment_theta=90.0), dict(segment_theta=89.99)),
    (dict(segment_theta=-60.0), dict(segment_theta=30.0)),
    (dict(segment_theta=120.0), dict(segment_theta=75.0)),
    (dict(num_vertical_scans=1), dict(num_vertical_scans=2)),
    (dict(num_vertical_scans=65), dict(num_vertical_scans=64)),
    (dict(num_horizontal_scans=15), dict(num_horizontal_scans=16)),
    (dict(num_horizontal_scans=2049), dict(num_horizontal_scans=2048)),
] + [({f: bad}, {} if f in _RANGED else {f: 3.4e38}) for f in _FLOAT_FIELDS for bad in (_NAN, _INF, -_INF)])
def test_create_refuses_undefined_configurations(refused, accepted):
    assert _create_rc(**refused) == _abi.LLSR_EINVAL, refused
    assert _create_rc(**accepted) in (_abi.LLSR_OK, LLSR_ENODEV), accepted


@pytest.mark.parametrize("fields", [
    dict(ground_scan_index=16), dict(ground_scan_index=1000), dict(ground_scan_index=-1),
    dict(edge_threshold=0.0), dict(surf_threshold=-1.0), dict(DBFr=0.0), dict(RatioXY=-1.0),
    dict(segment_valid_point_num=40), dict(segment_valid_line_num=0), dict(use_kitti=1),
    dict(nearest_feature_search_distance=0.0), dict(sensor_mount_angle=1e30),
])
def test_create_accepts_every_other_value(fields):
    assert _create_rc(**fields) in (_abi.LLSR_OK, LLSR_ENODEV), fields
