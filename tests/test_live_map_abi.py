"""CPU: the live map's entry points (kh_live_map_*, kh_mapper_set_scan_pose) are declared with prototypes, refuse NULL handles,
and -- there is no CPU fallback -- answer KH_ERR_NO_DEVICE where no device is visible."""
import ctypes as C

from slam_toolbox_amd import capi

NEW = ("kh_live_map_create", "kh_live_map_destroy", "kh_live_map_update", "kh_live_map_info", "kh_live_map_read", "kh_live_map_stats",
       "kh_mapper_set_scan_pose")


def test_new_entry_points_are_bound(kartohip_lib):
    for name in NEW:
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name


def test_null_handles_are_refused(kartohip_lib):
    L = kartohip_lib
    assert L.kh_live_map_update(None, 2, 0.1) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_read(None, None, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_info(None, C.byref(capi.KhLiveMapInfo())) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_stats(None, C.byref(capi.KhLiveMapStats())) == capi.KH_ERR_INVALID_ARG
    assert L.kh_live_map_create(None, 0.05, None, -1.0, None) == capi.KH_ERR_INVALID_ARG
    L.kh_live_map_destroy(None)


def test_create_without_a_device_is_no_device(kartohip_lib):
    h = C.c_void_p()
    rc = kartohip_lib.kh_live_map_create(None, 0.05, None, -1.0, C.byref(h))
    if kartohip_lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL mapper is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in kartohip_lib.kh_last_error()
    assert not h.value
